"""GPU: the depth-hint selection (csrc/hint_select.hip through mdx.functional.hint_select) against the CPU restatement of
tests/hint_select_cases.py -- l_hint, l_pred, sel and counts bit for bit; the restatement in its machine-independent form,
restate_pinned(), which tests/test_hint_select_cpu.py holds equal to restate() -- and against the chain of the project's own fine-grained
GPU ops, at a full-resolution disparity with opposite baseline signs, through the upsample path, at 2 x 3 (every window is all
reflection), at 37 x 150 (more than one 64 x 8 tile each way, partial last tiles, interior halos) and at 16 x 128 with an 8 x 64 disparity
(the 16-byte target loads of whole tiles, the separable upsample of H + W > 128).  The rule apart from the float
parity: keep is (hint > 0) & (l_hint < l_pred) of the kernel's own two maps.  Then ties, a batch of three against its singles, two
calls, a workspace of 0xff bytes, a captured call replayed on new data, one NaN / +inf in disp and in hint, and the trainer with
--stereo_hints 0.05 --stereo_hints_select: captured against eager, fused against op by op (tests/test_gpu_driver.py's trajectory
rule, run as tests/test_gpu_stereo_hints.py runs it), and nothing of it with the flag off.

KNOWN MISS: test_trainer_with_the_selection_captured_equals_eager missed _same_trajectory's 2e-4 bar at the third step in two of its
three runs (3.2e-4: 0.323240 against 0.323137; 2.9e-4).  Measured over four more captured / eager pairs: the third loss differs by 3.0e-4
in two and by 5e-6 / 9e-6 in two (it takes one of two values in either mode), later steps by up to 1.2e-3 (bar 1e-2), and the kept
masks of the two runs are identical at steps 1-3 in every pair (one pixel differs at step 4 in two).  So the selection does not flip
pixels there; what moves the third step was not found.  The bar is the issue's and stays."""
import functools
import importlib

import numpy as np
import pytest
import torch

import hint_select_cases as cases

pytestmark = pytest.mark.gpu

MAPS = ("l_hint", "l_pred", "sel")


@pytest.fixture(scope="module")
def G():
    import gpu_util
    return gpu_util


def _dev(G, c, **over):
    return [t.to(G.DEV) for t in cases.args(dict(c, **over))]


def _select(G, c, **over):
    from mdx import functional as F
    out = F.hint_select(*_dev(G, c, **over), cases.MIN_DEPTH, cases.MAX_DEPTH, return_losses=True)
    assert out["sel"].dtype == torch.float32 and out["counts"].dtype == torch.int32 and not out["sel"].requires_grad
    return {k: v.cpu() for k, v in out.items()}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b, keys=MAPS + ("counts",)):
    return [k for k in keys if not torch.equal(_bits(a[k]), _bits(b[k]))]


@pytest.mark.parametrize("name", cases.NAMES)
def test_the_kernel_follows_the_restatement(G, name):
    c, ref = cases.case(name), cases.reference(name, pinned=True)
    out = _select(G, c)
    B, _, H, W = c["target"].shape
    assert out["sel"].shape == out["l_hint"].shape == out["l_pred"].shape == (B, 1, H, W) and out["counts"].shape == (B, 2)
    for k in MAPS:
        G.assert_bitexact(out[k], ref[k].numpy(), "%s: %s" % (name, k))
    assert torch.equal(out["counts"], ref["counts"]), (out["counts"], ref["counts"])
    # the rule, from the kernel's own two maps
    keep = (c["hint"] > 0) & (out["l_hint"] < out["l_pred"])
    assert torch.equal(out["sel"] != 0, keep) and torch.equal(_bits(out["sel"])[keep], _bits(c["hint"])[keep])
    assert out["counts"].tolist() == [[int((c["hint"][b] > 0).sum()), int(keep[b].sum())] for b in range(B)]


@pytest.mark.parametrize("name", cases.NAMES)
def test_the_two_losses_are_those_of_the_fine_grained_ops(G, name):
    from mdx import functional as F
    c = cases.case(name)
    target, partner, K, invK, T, hint, disp = _dev(G, c)
    B, _, H, W = target.shape
    out = F.hint_select(target, partner, K, invK, T, hint, disp, cases.MIN_DEPTH, cases.MAX_DEPTH, return_losses=True)
    up = disp if tuple(disp.shape[2:]) == (H, W) else F.interpolate_bilinear(disp, H, W)
    P = F.compose_projection(K, T)
    for key, depth in (("l_hint", hint), ("l_pred", F.disparity2depth(up, cases.MIN_DEPTH, cases.MAX_DEPTH)[1])):
        warped = F.grid_sample_border(partner, F.project(F.backproject(depth, invK), P, H, W))
        G.assert_bitexact(out[key], F.reprojection_loss(warped, target).cpu().numpy(), "%s: %s" % (name, key))


@pytest.mark.parametrize("name", ["n13x37", "up16x40"])
def test_a_tie_keeps_nothing_on_the_device(G, name):
    c = cases.case(name)
    B, _, H, W = c["target"].shape
    out = _select(G, c, hint=cases.predicted_depth(c["disp"], H, W))
    assert torch.equal(_bits(out["l_hint"]), _bits(out["l_pred"]))
    assert not out["sel"].any() and out["counts"].tolist() == [[H * W, 0]] * B


def test_a_batch_of_three_equals_its_three_singles(G):
    c = cases.case("b3")
    whole = _select(G, c)
    assert _same(whole, cases.reference("b3", pinned=True)) == []
    for b in range(3):
        one = _select(G, {k: v[b:b + 1] for k, v in c.items()})
        assert _same(one, {k: v[b:b + 1] for k, v in whole.items()}) == [], b


def test_two_calls_give_the_same_bits_and_the_workspace_may_hold_anything(G):
    from mdx import functional as F
    c = cases.case("n37x150")
    first, again = _select(G, c), _select(G, c)
    assert _same(first, again) == []
    key = (0, 2, 37, 150, 37, 150)
    assert key in F.hint_select_workspaces()
    before = F._select_workspaces[key].data_ptr()
    F._select_workspaces[key].fill_(255)
    assert _same(_select(G, c), first) == []
    assert F._select_workspaces[key].data_ptr() == before


def test_a_target_that_is_not_16_byte_aligned_is_copied_by_the_binding(G):
    """The C entry point refuses such a target (tests/test_hint_select_abi.py); mdx.functional.hint_select hands it a copy."""
    from mdx import functional as F
    c = cases.case("up16x128")
    dev = _dev(G, c)
    room = torch.empty(dev[0].numel() + 1, device=G.DEV)
    view = room[1:].view_as(dev[0])
    view.copy_(dev[0])
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    out = F.hint_select(view, *dev[1:], cases.MIN_DEPTH, cases.MAX_DEPTH, return_losses=True)
    assert _same({k: v.cpu() for k, v in out.items()}, cases.reference("up16x128", pinned=True)) == []


def test_a_captured_call_replays_on_new_data(G):
    from mdx import functional as F
    c, other = cases.case("n13x37"), cases.case("b3")
    new = {k: v[1:3].clone() for k, v in other.items()}                      # signs (-1, +1): T changes too, read on the device at every replay
    static = _dev(G, c)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        F.hint_select(*static, cases.MIN_DEPTH, cases.MAX_DEPTH, return_losses=True)      # the warm-up allocates the workspace
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = F.hint_select(*static, cases.MIN_DEPTH, cases.MAX_DEPTH, return_losses=True)
    for s, n in zip(static, cases.args(new)):
        s.copy_(n.to(G.DEV))
    graph.replay()
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in res.items()}
    assert _same(got, _select(G, new)) == []
    assert _same(got, cases.restate_pinned(*cases.args(new))) == []
    assert not torch.equal(got["sel"], cases.reference("n13x37")["sel"])


def test_a_non_finite_value_stays_within_one_pixel(G):
    """One NaN and one +inf in disp and in hint (mdx_device.hpp's make_tap clamps a sampling position with fminf(fmaxf(.)) before it
    is converted, so a NaN samples pixel 0 and no index leaves the image): the outputs more than one pixel away are those of the
    clean run, and sel is 0 or the hint everywhere."""
    c = cases.case("n37x150")
    clean = _select(G, c)
    for which in ("disp", "hint"):
        bad = c[which].clone()
        bad[0, 0, 7, 63], bad[0, 0, 20, 100], bad[1, 0, 0, 0], bad[1, 0, 36, 149] = float("nan"), float("inf"), float("inf"), float("nan")
        out = _select(G, c, **{which: bad})
        hint = bad if which == "hint" else c["hint"]
        near = torch.nn.functional.max_pool2d((~torch.isfinite(bad)).float(), 3, 1, 1) > 0
        assert int(near.sum()) == 2 * 9 + 2 * 4
        for k in MAPS:
            assert torch.equal(_bits(out[k])[~near], _bits(clean[k])[~near]), (which, k)
        assert bool(((_bits(out["sel"]) == 0) | (_bits(out["sel"]) == _bits(hint))).all()), which


# ---- the trainer, as tests/test_gpu_stereo_hints.py runs it ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _trainer_run(graph, fused=True, select=True, n=6, lr_change_at=4):
    """Six steps with the learning rate taken down to 1e-6 at step 4 (tests/test_gpu_stereo_hints._trainer_run, whose docstring has the
    reason) with --stereo_hints 0.05 and --stereo_hints_select -> (losses, hint counts, kept counts, the trainer)."""
    bench = importlib.import_module("bench")
    from mdx import functional as F
    from model_train import trainer
    calls = []
    real = F.hint_select
    F.hint_select = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        torch.manual_seed(0)
        opt = bench.make_opt(2, height=64, width=96, frame_ids=(0, -1, 1, "s"))
        opt.use_automasking, opt.graph, opt.synthetic_length, opt.max_steps, opt.miopen_find = False, graph, 16, 0, False
        opt.synthetic_geometry = True
        opt.fused, opt.stereo_hints, opt.stereo_hints_select = fused, 0.05, select
        tr = trainer(opt)
        tr.setting.set_train()
        batches = list(tr.setting.train_dataloader)[:n]
        torch.manual_seed(1)
        losses, valid, kept = [], [], []
        for i, b in enumerate(batches):
            if i == lr_change_at:
                for g in tr.setting.optim["optimizer"].param_groups:
                    if torch.is_tensor(g["lr"]):
                        g["lr"].fill_(1e-6)
                    else:
                        g["lr"] = 1e-6
            o = tr.train_step(dict(b))
            losses.append(o["loss"].detach().clone())
            valid.append(o["hint_valid"].clone())
            if select:
                kept.append(o["hint_kept"].clone())
            else:
                assert "hint_kept" not in o
    finally:
        F.hint_select = real
    return [float(v) for v in losses], [float(v) for v in valid], [float(v) for v in kept], len(calls), tr


def test_with_the_flag_off_nothing_of_it_is_made(G):
    from mdx import functional as F
    held = {k: v.data_ptr() for k, v in F._select_workspaces.items()}
    losses, valid, kept, ncalls, tr = _trainer_run(True, select=False)
    assert tr._graphed is not None and tr.compute.stereo_hints_select is False
    assert kept == [] and ncalls == 0 and all(np.isfinite(losses))
    assert {k: v.data_ptr() for k, v in F._select_workspaces.items()} == held
    tr.stereo_hints_add(tr.train_step(dict(next(iter(tr.setting.train_dataloader)))))
    assert "kept share" not in tr.stereo_hints_report()


def test_trainer_with_the_selection_captured_equals_eager(G):
    from test_gpu_driver import _same_trajectory
    eager, valid_e, kept_e, calls_e, tr_e = _trainer_run(False)
    graph, valid_g, kept_g, calls_g, tr_g = _trainer_run(True)
    assert tr_g._graphed is not None and tr_e._graphed is None
    print("eager %s\ngraph %s\nhints %s\nkept eager %s\nkept graph %s" % (eager, graph, valid_e, kept_e, kept_g))
    assert calls_e == 6 and 1 <= calls_g < 6                                  # captured: the warm-up and the capture call it, the replays do not
    _same_trajectory(graph, eager)
    assert valid_g == valid_e                                                  # the hints are a function of the batches alone
    for valid, kept in ((valid_e, kept_e), (valid_g, kept_g)):
        assert all(0 < k <= v for k, v in zip(kept, valid)), (kept, valid)
    # the epoch line carries the kept share
    tr_g._hint_acc, tr_g._hint_steps = None, 0
    batches = list(tr_g.setting.train_dataloader)[:2]
    outs = [tr_g.train_step(dict(b)) for b in batches]
    want = []
    for o in outs:
        want.append((float(o["hint_valid"]), float(o["hint_kept"])))
        tr_g.stereo_hints_add(o)
    line = tr_g.stereo_hints_report()
    assert line.startswith("stereo hints: weight 0.05, 64 disparities, mean term "), line
    assert line.endswith(" over 2 steps, kept share %.4f of the hints" % (sum(k for _, k in want) / sum(v for v, _ in want))), line


def test_trainer_with_the_selection_fused_equals_op_by_op(G):
    from test_gpu_driver import _same_trajectory
    eager, valid_e, kept_e, _, tr_e = _trainer_run(False)
    op_by_op, valid_o, kept_o, calls_o, tr_o = _trainer_run(False, fused=False)
    assert tr_e.compute.fused and not tr_o.compute.fused and calls_o == 6
    print("fused %s\nop by op %s" % (eager, op_by_op))
    _same_trajectory(op_by_op, eager)
    assert valid_o == valid_e
    assert all(0 < k <= v for k, v in zip(kept_o, valid_o)), (kept_o, valid_o)
