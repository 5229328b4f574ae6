"""GPU: the sparse lidar term (csrc/sparse_depth.hip through mdx.functional.sparse_depth_loss) against the float64 yardstick of
tests/sparse_depth_cases.py, with the project's own bars -- terms: assert_close(rel=1e-4); gradients: assert_close(rel=1e-4,
elem=1e-4); the valid count: exact -- and: the sum of a scale's whole gradient against the float64 sum of the per-pixel coefficients
(the taps' weights add up to 1: a footprint that misses or doubles a pixel shows here without the yardstick's interpolation); no
valid pixel; the NaN rule, both ways; bit-equal launches; a captured forward + backward pair replayed on new data; a descent; and
the trainer with --depth_supervision, captured against eager and fused against op by op, under tests/test_gpu_driver.py's rules.

The coefficient-sum bar: every gradient element is a float64 sum rounded once to float32 (2^-24 of its own value), and the test adds
the elements in float64, so the sum is off by at most 2^-24 * sum|element|; the cases' coefficients keep sum|.| / |sum| far below
the 1e-4 / 2^-24 ~ 1700 at which the bar would be reached (the test asserts that ratio too, so a case that cancels says so)."""
import functools
import importlib

import numpy as np
import pytest
import torch

import sparse_depth_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gpu_util
    return gpu_util


def _loss(F, disps, gt, **kw):
    return F.sparse_depth_loss(disps, gt, cases.MIN_DEPTH, cases.MAX_DEPTH, eps=cases.EPS, **kw)


def _device(G, disps, gt, misaligned=None):
    """The case on the GPU, a misaligned base kept misaligned (a view one float into its buffer, as the case builds it).
    misaligned = True / False: assert that every base on the device is 4 bytes past / on a 16-byte boundary."""
    def up(t):
        if t.data_ptr() % 16 == 0:
            return t.to(G.DEV)
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=G.DEV)
        buf[1:] = t.reshape(-1).to(G.DEV)
        v = buf[1:].view(t.shape)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v
    xs, g = [up(d).requires_grad_(True) for d in disps], up(gt)
    if misaligned is not None:
        assert all(t.is_contiguous() and t.data_ptr() % 16 == (4 if misaligned else 0) for t in xs + [g]), \
            [t.data_ptr() % 16 for t in xs + [g]]
    return xs, g


def _run(G, disps, gt, weights, misaligned=None):
    from mdx import functional as F
    xs, g = _device(G, disps, gt, misaligned)
    res = _loss(F, xs, g)
    (res["loss"] * torch.tensor(weights, device=G.DEV)).sum().backward()
    return res, [x.grad for x in xs]


@pytest.mark.parametrize("nscales, one_image", cases.VARIANTS, ids=cases.VARIANT_IDS)
@pytest.mark.parametrize("name", cases.NAMES)
def test_the_kernels_follow_the_yardstick(G, name, nscales, one_image):
    disps, gt, extra, want = cases.reference(name, nscales, one_image)
    res, grads = _run(G, disps, gt, cases.WEIGHTS[:nscales], misaligned=(name == "C1"))
    loss, n = res["loss"].detach().cpu().numpy(), float(res["valid"])
    print("%s %s: n %d (want %d), loss %s, want %s" % (name, (nscales, one_image), n, want["n"], loss, want["loss"]))
    assert res["loss"].dtype == torch.float32 and tuple(res["loss"].shape) == (nscales,) and res["valid"].dim() == 0
    assert n == want["n"] and ("n" not in extra or extra["n"] == want["n"])
    G.assert_close(loss, want["loss"], "%s: terms" % name, rel=1e-4)
    for k, (g, ref) in enumerate(zip(grads, want["grads"])):
        assert g.dtype == torch.float32 and g.shape == ref.shape and bool(torch.isfinite(g).all())
        # (an all-zero reference -- no valid pixel -- has no significant entry to hold entry by entry: the max-norm bar asks zeros)
        G.assert_close(g, ref.numpy(), "%s: gradient of scale %d" % (name, k), rel=1e-4, elem=1e-4 if want["n"] else None)
        total, mass = float(g.double().sum()), float(g.double().abs().sum())
        print("  scale %d: sum of the gradient %.9g, coefficient sum %.9g, sum|.| %.9g" % (k, total, want["coef"][k], mass))
        if want["n"]:
            assert mass <= 100.0 * abs(want["coef"][k]), "the case's coefficients cancel: the bar below does not hold by construction"
        G.assert_close(np.float64(total), np.float64(want["coef"][k]), "%s: sum of the gradient of scale %d" % (name, k), rel=1e-4)


def test_no_valid_pixel_gives_zeros_and_no_nan(G):
    disps, gt, _ = cases.build("D")
    res, grads = _run(G, disps, gt, cases.WEIGHTS)
    assert float(res["valid"]) == 0.0 and torch.equal(res["loss"].detach().cpu(), torch.zeros(4))
    assert all(torch.equal(g.cpu(), torch.zeros(g.shape)) for g in grads)


def test_one_pixel_in_the_corner_reaches_the_last_taps_only(G):
    disps, gt, _, want = cases.reference("E")
    res, grads = _run(G, disps, gt, cases.WEIGHTS)
    assert float(res["valid"]) == 1.0
    for k, g in enumerate(grads):
        g = g.cpu()
        assert float(g[-1, 0, -1, -1]) != 0.0 and int((g != 0).sum()) == 1, k          # both taps clamp onto the corner element
        G.assert_close(np.float64(g[-1, 0, -1, -1]), np.float64(want["coef"][k]), "corner element of scale %d" % k, rel=1e-4)


def test_the_nan_rule_both_ways(G):
    disps, gt, extra = cases.build("F")
    clean, clean_grads = _run(G, disps, gt, cases.WEIGHTS)
    assert float(clean["valid"]) == extra["n"] and bool(torch.isfinite(clean["loss"]).all())
    under_invalid = [d.clone() for d in disps]
    for d in under_invalid:
        d[:, 0, 0, 0] = float("nan")                       # column 0: no valid pixel has a tap on it
    res, grads = _run(G, under_invalid, gt, cases.WEIGHTS)
    assert torch.equal(res["loss"], clean["loss"]) and torch.equal(res["valid"], clean["valid"])
    assert all(torch.equal(g, c) for g, c in zip(grads, clean_grads))
    for value in (float("nan"), -1.0, float("inf")):       # the last column lies under valid pixels: sd NaN, negative, infinite
        under_valid = [d.clone() for d in disps]
        under_valid[1][:, 0, :, -1] = value
        res, grads = _run(G, under_valid, gt, cases.WEIGHTS)
        loss = res["loss"].detach()
        assert bool(torch.isnan(loss[1])), (value, loss)
        assert torch.equal(loss[[0, 2, 3]], clean["loss"].detach()[[0, 2, 3]]) and torch.equal(res["valid"], clean["valid"])
        assert bool(torch.isnan(grads[1]).any())
        assert all(torch.equal(grads[k], clean_grads[k]) for k in (0, 2, 3))


@pytest.mark.parametrize("name", ["C", "C1", "Cd"])
def test_two_launches_give_the_same_bits(G, name):
    disps, gt, _ = cases.build(name)
    a, ga = _run(G, disps, gt, cases.WEIGHTS, misaligned=(name == "C1"))
    b, gb = _run(G, disps, gt, cases.WEIGHTS, misaligned=(name == "C1"))
    G.assert_bitexact(a["loss"], b["loss"].detach().cpu().numpy(), "terms")
    G.assert_bitexact(a["valid"], b["valid"].cpu().numpy(), "valid count")
    for k, (x, y) in enumerate(zip(ga, gb)):
        G.assert_bitexact(x, y.cpu().numpy(), "gradient of scale %d" % k)


def test_forward_only_under_no_grad(G):
    from mdx import functional as F
    disps, gt, _, want = cases.reference("A")
    xs, g = _device(G, disps, gt)
    with torch.no_grad():
        res = _loss(F, xs, g)
    assert not res["loss"].requires_grad and res["loss"].grad_fn is None
    G.assert_close(res["loss"], want["loss"], "terms under no_grad", rel=1e-4)


def test_what_is_refused(G):
    from mdx import functional as F
    from mdx._lib import MdxError
    disps, gt, _ = cases.build("A")
    xs, g = _device(G, disps, gt)
    for bad in (lambda: _loss(F, [], g), lambda: _loss(F, xs + xs[:1], g), lambda: _loss(F, xs, g[:1]),
                lambda: _loss(F, xs, g[:, :, :4]), lambda: _loss(F, xs, g[:, 0]), lambda: _loss(F, xs, g, lo=5.0, hi=5.0),
                lambda: F.sparse_depth_loss(xs, g, 0.0, 100.0), lambda: F.sparse_depth_loss(xs, g, 0.1, 100.0, eps=0.0),
                lambda: _loss(F, [x.detach().cpu() for x in xs], g)):
        with pytest.raises(MdxError):
            bad()


def test_a_captured_pair_replays_on_new_data(G):
    """Forward and backward captured into one graph over static inputs; new data copied in, one replay: the bits of the eager call
    on that data."""
    from mdx import functional as F
    disps, gt, _ = cases.build("C")
    other_d, other_gt, _ = cases.build("Cd")
    xs, g = _device(G, disps, gt)
    weights = torch.tensor(cases.WEIGHTS, device=G.DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        res = _loss(F, xs, g)
        torch.autograd.grad((res["loss"] * weights).sum(), xs)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = _loss(F, xs, g)
        grads = torch.autograd.grad((res["loss"] * weights).sum(), xs)
    with torch.no_grad():
        for x, d in zip(xs, other_d):
            x.copy_(0.5 * d.to(G.DEV) + 0.1)
        g.copy_(torch.where(other_gt > 40.0, other_gt, torch.zeros_like(other_gt)).to(G.DEV))
    graph.replay()
    torch.cuda.synchronize()
    eager = _loss(F, xs, g)
    eager_grads = torch.autograd.grad((eager["loss"] * weights).sum(), xs)
    assert 0 < float(eager["valid"]) < gt.numel()
    G.assert_bitexact(res["loss"], eager["loss"].detach().cpu().numpy(), "replayed terms")
    G.assert_bitexact(res["valid"], eager["valid"].cpu().numpy(), "replayed valid count")
    for k, (a, b) in enumerate(zip(grads, eager_grads)):
        G.assert_bitexact(a, b.cpu().numpy(), "replayed gradient of scale %d" % k)


def test_adam_on_the_term_alone_descends(G):
    """Four leaf disparities of case A's sizes, 200 steps of torch's Adam on the mean of the terms: it falls below a tenth of its
    start.  A departure from the issue's wording, which names case A: the ground truth here is NOT case A's but one every scale
    can represent -- one depth per image, a third of the pixels valid.  Case A's depths are random per pixel, and a 1 x 2 or
    2 x 4 disparity cannot follow them, so with them the mean of the four terms could not fall tenfold whatever the kernels do."""
    from mdx import functional as F
    gen = torch.Generator().manual_seed(7)
    B, (gh, gw) = 2, (19, 37)
    depth = torch.tensor([0.25, 0.4]).view(B, 1, 1, 1).expand(B, 1, gh, gw)
    gt = torch.where(torch.rand(B, 1, gh, gw, generator=gen) < 0.33, depth, torch.zeros(B, 1, gh, gw)).to(G.DEV)
    xs = [(0.85 + 0.1 * torch.rand(B, 1, h, w, generator=gen)).to(G.DEV).requires_grad_(True) for h, w in cases.SIZES_A]
    opt = torch.optim.Adam(xs, lr=0.01)
    history = []
    for _ in range(200):
        opt.zero_grad(set_to_none=True)
        term = _loss(F, xs, gt)["loss"].mean()
        term.backward()
        opt.step()
        history.append(term.detach())
    history = torch.stack(history).cpu().tolist()
    print("descent: start %g, after 200 steps %g" % (history[0], history[-1]))
    assert all(np.isfinite(history)) and history[0] > 0.5 and history[-1] < 0.1 * history[0], (history[0], history[-1])


# ---- the trainer at the smallest size tests/test_gpu_driver.py uses -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _trainer_run(graph, fused=True, n=6):
    """Six steps of the trainer with --depth_supervision 0.05 -> (losses, per-scale terms, valid counts, the batches, the trainer);
    run once per setting and shared."""
    bench = importlib.import_module("bench")
    from model_train import trainer
    torch.manual_seed(0)
    opt = bench.make_opt(2, height=64, width=96)
    opt.use_automasking, opt.graph, opt.synthetic_length, opt.max_steps, opt.miopen_find = False, graph, 16, 0, False
    opt.fused, opt.depth_supervision = fused, 0.05
    tr = trainer(opt)
    tr.setting.set_train()
    batches = list(tr.setting.train_dataloader)[:n]
    torch.manual_seed(1)
    losses, terms, valid = [], [], []
    for b in batches:
        o = tr.train_step(dict(b))
        losses.append(o["loss"].detach().clone())
        terms.append(o["loss_depth"].clone())
        valid.append(o["depth_valid"].clone())
    return [float(v) for v in losses], [t.cpu() for t in terms], [float(v) for v in valid], batches, tr


def _valid_counts(opt, batches):
    lo, hi = np.float32(opt.min_depth), np.float32(opt.max_depth)
    return [float(((b[("depth", 0)] > lo) & (b[("depth", 0)] < hi)).sum()) for b in batches]


def test_trainer_with_depth_supervision_captured_equals_eager(G):
    from test_gpu_driver import _same_trajectory
    eager, terms_e, valid_e, batches, tr_e = _trainer_run(False)
    graph, terms_g, valid_g, _, tr_g = _trainer_run(True)
    assert tr_g._graphed is not None and tr_e._graphed is None
    assert ("depth", 0) in tr_g._graphed.copied                                    # a static buffer, copied per replay
    print("eager %s\ngraph %s" % (eager, graph))
    _same_trajectory(graph, eager)
    want = _valid_counts(tr_e.opt, batches)                                        # the valid pixels of every batch, exactly
    assert valid_e == want and valid_g == want and min(want) > 0 and len(set(want)) > 1
    assert all(t.shape == (4,) and bool(torch.isfinite(t).all()) and float(t.min()) > 0 for t in terms_e + terms_g)
    np.testing.assert_allclose(torch.stack(terms_g).numpy()[:3], torch.stack(terms_e).numpy()[:3], rtol=2e-4)
    # the epoch line: sums kept on the device, read once
    tr_g._depth_acc, tr_g._depth_steps = None, 0
    for b in batches[:2]:
        tr_g.depth_supervision_add(tr_g.train_step(dict(b)))
    line = tr_g.depth_supervision_report()
    assert line.startswith("depth supervision: weight 0.05, mean term ") and line.endswith(" over 2 steps"), line
    assert "%.1f valid pixels per image" % ((want[0] + want[1]) / 4) in line, line
    assert tr_g._depth_steps == 0 and float(tr_g._depth_acc.abs().sum()) == 0.0


def test_trainer_with_depth_supervision_fused_equals_op_by_op(G):
    from test_gpu_driver import _same_trajectory
    eager, terms_e, _, batches, tr_e = _trainer_run(False)
    op_by_op, terms_o, valid_o, _, tr_o = _trainer_run(False, fused=False)
    assert tr_e.compute.fused and not tr_o.compute.fused
    print("fused %s\nop by op %s" % (eager, op_by_op))
    assert valid_o == _valid_counts(tr_e.opt, batches)
    _same_trajectory(op_by_op, eager)
    # the term is part of the loss on both paths: the same validation step with and without the weight differs by W * mean_k L_k
    for tr in (tr_e, tr_o):
        tr.setting.set_valid()
        with torch.no_grad():
            with_term = tr.batch_process(dict(batches[0]))
            tr.compute.depth_supervision = 0.0
            without = tr.batch_process(dict(batches[0]))
            tr.compute.depth_supervision = 0.05
        assert "loss_depth" not in without and "depth_valid" not in without
        a, b, term = float(with_term["loss"]), float(without["loss"]), float(with_term["loss_depth"].double().mean())
        assert term > 0 and abs(a - b - 0.05 * term) <= 2e-6 * abs(a), (a, b, term)
