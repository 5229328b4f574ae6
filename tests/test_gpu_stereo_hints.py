"""GPU: the stereo matcher (csrc/stereo_hints.hip through mdx.functional.stereo_hints) against the numpy restatement of
tests/stereo_hint_cases.py: S, the valid map and the integer disparities exactly, disp and depth bit for bit -- at sizes narrower
than D, at two disparities per lane with winners beyond 64, on a constant image, on flat five-level blocks (ties), with a dead
sample beside a live one.  Then: a batch of 3 against the three singles; two calls; other images in the same workspace; a captured
call replayed on new data; the hint through sparse_depth_loss at the disparity's own size against the float64 yardstick of
tests/sparse_depth_cases.py within that file's bars; and the trainer with --stereo_hints 0.05 on the geometry set with "s",
captured against eager and fused against op by op, under tests/test_gpu_driver.py's trajectory rule; with W = 0 nothing of it is
made."""
import functools
import importlib

import numpy as np
import pytest
import torch

import sparse_depth_cases
import stereo_hint_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gpu_util
    return gpu_util


def _hints(G, t, p, K, T, D, **kw):
    """-> the outputs as numpy arrays (volume: a copy of S, taken before another call can overwrite the workspace)"""
    from mdx import functional as F
    out = F.stereo_hints(*(G.t(np.array(a)) for a in (t, p, K, T)), max_disp=D, return_volume=True, **kw)
    assert out["depth"].dtype == out["disp"].dtype == torch.float32 and out["valid"].dtype == torch.uint8
    assert out["volume"].dtype == torch.int16 and tuple(out["volume"].shape) == (t.shape[0],) + t.shape[2:] + (D,)
    assert not out["depth"].requires_grad
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


def _assert_same(G, out, ref, what):
    assert out["volume"].min() >= 0
    bad = out["volume"].astype(np.int64) != ref["S"].astype(np.int64)
    assert not bad.any(), "%s: S differs in %d of %d elements, first at %s" % (what, bad.sum(), bad.size, np.argwhere(bad)[0])
    assert np.array_equal(out["valid"], ref["valid"]), "%s: valid differs in %d pixels" % (what, (out["valid"] != ref["valid"]).sum())
    live = ref["valid"].astype(bool)[:, 0]
    assert (np.abs(out["disp"][:, 0][live] - ref["d0"][live]) <= 0.5).all(), what + ": the parabola moves d0 by half a pixel at the most"
    G.assert_bitexact(out["disp"], ref["disp"], what + ": disp")
    G.assert_bitexact(out["depth"], ref["depth"], what + ": depth")


@pytest.mark.parametrize("name", cases.SHAPE_CASES)
def test_the_kernels_follow_the_restatement(G, name):
    t, p, K, T, D = cases.case(name)
    out = _hints(G, t, p, K, T, D)
    _assert_same(G, out, cases.reference(name), name)
    assert out["disp"].shape == out["depth"].shape == out["valid"].shape == (t.shape[0], 1) + t.shape[2:]


def test_other_penalties(G):
    t, p, K, T, D = cases.case("n13x37")
    _assert_same(G, _hints(G, t, p, K, T, D, p1=3, p2=190), cases.restate(t, p, K, T, D, 3, 190), "P1 3, P2 190")


def test_a_batch_of_three_equals_the_three_singles(G):
    t, p, K, T, D = cases.case("b3")
    whole = _hints(G, t, p, K, T, D)
    _assert_same(G, whole, cases.reference("b3"), "b3")
    for b in range(3):
        one = _hints(G, t[b:b + 1], p[b:b + 1], K[b:b + 1], T[b:b + 1], D)
        for k in ("volume", "valid", "disp", "depth"):
            assert np.array_equal(one[k][0].view(np.uint8), np.ascontiguousarray(whole[k][b]).view(np.uint8)), (b, k)


def test_two_calls_give_the_same_bits_and_other_images_in_the_same_workspace_equal_a_fresh_call(G):
    from mdx import functional as F
    t, p, K, T, D = cases.case("n24x80")
    first = _hints(G, t, p, K, T, D)
    again = _hints(G, t, p, K, T, D)
    for k in first:
        assert np.array_equal(first[k].view(np.uint8), again[k].view(np.uint8)), k
    # other images of the same shape: the workspace (S of the calls above in it) is found again, and S is written, not added to
    t2, p2 = cases.shifted_pair(77, 24, 80, (1, -1), noise=0.05)
    key = (0, 2, 24, 80, D)
    assert key in F.stereo_hints_workspaces()
    before = F._hint_workspaces[key].data_ptr()
    other = _hints(G, t2, p2, K, T, D)
    assert F._hint_workspaces[key].data_ptr() == before
    _assert_same(G, other, cases.restate(t2, p2, K, T, D), "other images in the used workspace")
    assert not np.array_equal(other["volume"], first["volume"])
    # and a workspace full of ones
    F._hint_workspaces[key].fill_(255)
    _assert_same(G, _hints(G, t, p, K, T, D), cases.reference("n24x80"), "a workspace of 0xff bytes")


def test_a_captured_call_replays_on_new_data(G):
    from mdx import functional as F
    t, p, K, T, D = cases.case("n24x80")
    t2, p2 = cases.shifted_pair(78, 24, 80, (1, -1), noise=0.03)
    T2 = T.copy()
    T2[:, 0, 3] = -T2[:, 0, 3]                               # the signs change too: read on the device at every replay
    st, sp, sK, sT = (G.t(np.array(a)) for a in (t, p, K, T))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        F.stereo_hints(st, sp, sK, sT, max_disp=D)           # the warm-up allocates the workspace
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = F.stereo_hints(st, sp, sK, sT, max_disp=D, return_volume=True)
    st.copy_(G.t(t2)), sp.copy_(G.t(p2)), sT.copy_(G.t(T2))
    graph.replay()
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy().copy() for k, v in res.items()}
    _assert_same(G, got, cases.restate(t2, p2, K, T2, D), "replayed on new data")
    eager = _hints(G, t2, p2, K, T2, D)
    for k in got:
        assert np.array_equal(got[k].view(np.uint8), eager[k].view(np.uint8)), k


def test_the_hint_through_the_sparse_depth_term_agrees_with_its_yardstick(G):
    """The hint map as the `gt` of mdx.functional.sparse_depth_loss at the disparity's OWN size at scale 0 (the element itself, no
    resampling) and resampled at the others, against the float64 yardstick of tests/sparse_depth_cases.py, with that file's bars:
    terms assert_close(rel=1e-4), gradients assert_close(rel=1e-4, elem=1e-4), the valid count exact."""
    from mdx import functional as F
    name = "n24x80"
    t, p, K, T, D = cases.case(name)
    hint = F.stereo_hints(*(G.t(np.array(a)) for a in (t, p, K, T)), max_disp=D)["depth"]
    G.assert_bitexact(hint, cases.reference(name)["depth"], "hint depth")
    gen = torch.Generator().manual_seed(5)
    disps = [0.02 + 0.9 * torch.rand(2, 1, 24 >> k, 80 >> k, generator=gen) for k in range(4)]
    weights = sparse_depth_cases.WEIGHTS
    want = sparse_depth_cases.yardstick(disps, hint.cpu(), weights)
    assert want["n"] == int(((hint > sparse_depth_cases.LO) & (hint < sparse_depth_cases.HI)).sum()) > 0.5 * 2 * 24 * 80
    xs = [d.to(G.DEV).requires_grad_(True) for d in disps]
    res = F.sparse_depth_loss(xs, hint, sparse_depth_cases.MIN_DEPTH, sparse_depth_cases.MAX_DEPTH, eps=sparse_depth_cases.EPS)
    (res["loss"] * torch.tensor(weights, device=G.DEV)).sum().backward()
    assert float(res["valid"]) == want["n"]
    G.assert_close(res["loss"], want["loss"], "terms against the hint")
    for k, x in enumerate(xs):
        G.assert_close(x.grad, want["grads"][k].numpy(), "gradient of scale %d against the hint" % k, elem=1e-4)


# ---- the trainer at the smallest size tests/test_gpu_driver.py uses, on the geometry set with "s" ----------------------------------
@functools.lru_cache(maxsize=None)
def _trainer_run(graph, fused=True, weight=0.05, n=6, lr_change_at=4):
    """Six steps as tests/test_gpu_driver.py's _trainer_losses runs them -- the run its trajectory rule is stated for: the same size,
    seeds and options, the learning rate taken down to 1e-6 at step 4 as StepLR does at an epoch boundary -- with the geometry set,
    the stereo partner and --stereo_hints -> (losses, per-scale terms, hint counts, the batches, the trainer); run once per setting."""
    bench = importlib.import_module("bench")
    from model_train import trainer
    torch.manual_seed(0)
    opt = bench.make_opt(2, height=64, width=96, frame_ids=(0, -1, 1, "s"))
    opt.use_automasking, opt.graph, opt.synthetic_length, opt.max_steps, opt.miopen_find = False, graph, 16, 0, False
    opt.synthetic_geometry = True
    opt.fused, opt.stereo_hints = fused, weight
    tr = trainer(opt)
    tr.setting.set_train()
    batches = list(tr.setting.train_dataloader)[:n]
    torch.manual_seed(1)
    losses, terms, valid = [], [], []
    for i, b in enumerate(batches):
        if i == lr_change_at:
            for g in tr.setting.optim["optimizer"].param_groups:
                if torch.is_tensor(g["lr"]):
                    g["lr"].fill_(1e-6)
                else:
                    g["lr"] = 1e-6
        o = tr.train_step(dict(b))
        losses.append(o["loss"].detach().clone())
        if weight > 0:
            terms.append(o["loss_hint"].clone())
            valid.append(o["hint_valid"].clone())
        else:
            assert "loss_hint" not in o and "hint_valid" not in o
    return [float(v) for v in losses], [t.cpu() for t in terms], [float(v) for v in valid], batches, tr


def _hint_counts(opt, batches):
    """The pixels of every batch whose restated hint depth lies inside (min_depth, max_depth)."""
    lo, hi = np.float32(opt.min_depth), np.float32(opt.max_depth)
    counts = []
    for b in batches:
        ref = cases.restate(b[("color", 0, 0)].numpy(), b[("color", "s", 0)].numpy(), b[("K", 0)].numpy(), b["stereo"].numpy(), 64)
        counts.append(float(((ref["depth"] > lo) & (ref["depth"] < hi)).sum()))
    return counts


def test_with_the_weight_at_zero_nothing_of_it_is_made(G):
    """The same run with W = 0: no module, no entry in the outputs, and the workspaces held are those held before -- none of the
    run's shape unless a run with the option on made it earlier in the session."""
    from mdx import functional as F
    held = {k: v.data_ptr() for k, v in F._hint_workspaces.items()}
    losses, terms, valid, _, tr = _trainer_run(True, weight=0.0)
    assert tr._graphed is not None and tr.compute.stereo_hints == 0.0 and tr.compute._hint_loss is None
    assert terms == [] and valid == [] and tr._hint_acc is None and tr._hint_steps == 0
    assert {k: v.data_ptr() for k, v in F._hint_workspaces.items()} == held
    assert all(np.isfinite(losses))


def test_trainer_with_stereo_hints_captured_equals_eager(G):
    from test_gpu_driver import _same_trajectory
    eager, terms_e, valid_e, batches, tr_e = _trainer_run(False)
    graph, terms_g, valid_g, _, tr_g = _trainer_run(True)
    assert tr_g._graphed is not None and tr_e._graphed is None
    print("eager %s\ngraph %s" % (eager, graph))
    _same_trajectory(graph, eager)
    want = _hint_counts(tr_e.opt, batches)                                         # the hint pixels of every batch, exactly
    assert valid_e == want and valid_g == want and min(want) > 0.3 * 2 * 64 * 96, (valid_e, valid_g, want)
    assert all(t.shape == (4,) and bool(torch.isfinite(t).all()) and float(t.min()) > 0 for t in terms_e + terms_g)
    # the per-scale terms of the FIRST step: the two runs hold the same weights there and differ by float32 summation order alone (the
    # rule's first bar).  Later steps are held to the rule through the loss above: it is stated for the loss, and a single coarse
    # scale's term -- 8 x 12 disparities under 6144 hints -- moves far more under Adam's amplification than the loss it is a part of
    np.testing.assert_allclose(torch.stack(terms_g).numpy()[0], torch.stack(terms_e).numpy()[0], rtol=2e-4)
    # the epoch line: sums kept on the device, read once
    tr_g._hint_acc, tr_g._hint_steps = None, 0
    for b in batches[:2]:
        tr_g.stereo_hints_add(tr_g.train_step(dict(b)))
    line = tr_g.stereo_hints_report()
    assert line.startswith("stereo hints: weight 0.05, 64 disparities, mean term ") and line.endswith(" over 2 steps"), line
    assert "valid share %.4f per image" % ((want[0] + want[1]) / (4 * 64 * 96)) in line, line
    assert tr_g._hint_steps == 0 and float(tr_g._hint_acc.abs().sum()) == 0.0


def test_trainer_with_stereo_hints_fused_equals_op_by_op(G):
    from test_gpu_driver import _same_trajectory
    eager, _, _, batches, tr_e = _trainer_run(False)
    op_by_op, _, valid_o, _, tr_o = _trainer_run(False, fused=False)
    assert tr_e.compute.fused and not tr_o.compute.fused
    print("fused %s\nop by op %s" % (eager, op_by_op))
    assert valid_o == _hint_counts(tr_e.opt, batches)
    _same_trajectory(op_by_op, eager)
    # the term is part of the loss on both paths: the same validation step with and without the weight differs by W * mean_k L_k
    for tr in (tr_e, tr_o):
        tr.setting.set_valid()
        with torch.no_grad():
            with_term = tr.batch_process(dict(batches[0]))
            tr.compute.stereo_hints = 0.0
            without = tr.batch_process(dict(batches[0]))
            tr.compute.stereo_hints = 0.05
        assert "loss_hint" not in without and "hint_valid" not in without
        a, b, term = float(with_term["loss"]), float(without["loss"]), float(with_term["loss_hint"].double().mean())
        assert term > 0 and abs(a - b - 0.05 * term) <= 2e-6 * abs(a), (a, b, term)
