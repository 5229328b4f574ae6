"""GPU: the train-time depth monitor (csrc/monitor.hip) through mdx.functional.depth_monitor against the float64 reference
of tests/monitor_cases.py, at the sizes where its seven launches change their path: the median's rank on two-level inputs
(one pair of levels per radix pass), window geometry, the bilinear forms, the clamp's ends, more than 1024 blocks, one
workspace reused across geometries, NaN predictions, and the refusals of the C entry point.
tests/test_monitor_reference.py (CPU) checks the reference and what the case builders claim."""
import ctypes as C

import numpy as np
import pytest
import torch

import monitor_cases as mc

pytestmark = pytest.mark.gpu

REL = 2e-5           # the four error numbers (tests/test_gpu_golden_r2.py's figure for them), per number
ABS_ZERO = 1e-7      # ... where the reference is exactly 0
ABS_A = 1e-7         # a1..a3 against count / n (the float32 result rounds by up to 6e-8)
MARGIN = 1e-5        # no masked pixel's max(g/p, p/g) this close (relative) to a threshold: then the counts must agree


@pytest.fixture(scope="module")
def G():
    import gpu_util
    return gpu_util


def run(G, c, pred=None, workspace=None):
    pred = (c.pred if pred is None else pred).to(G.DEV)
    gt = c.gt.to(G.DEV)
    if workspace is None:
        return G.F.depth_monitor(pred, gt, c.window, c.lo, c.hi).cpu().numpy()
    from mdx import _lib
    B, _, h, w = pred.shape
    gh, gw = gt.shape[-2:]
    r0, r1, c0, c1 = c.window
    out = torch.empty(8, device=G.DEV)
    nws = _lib.api.mdx_depth_monitor_workspace_bytes(B, r0, r1, c0, c1)
    assert nws <= workspace.numel() * 8
    _lib.api.mdx_depth_monitor(_lib.ptr(pred), B, h, w, _lib.ptr(gt), gh, gw, r0, r1, c0, c1, c.lo, c.hi, _lib.ptr(out),
                               _lib.ptr(workspace, torch.float64), workspace.numel() * 8, _lib.stream())
    return out.cpu().numpy()


def check(got, ref, what):
    print("%s: n %d  got %s  reference %s  margin %.3g" % (what, ref.n, got[:7], ref.metrics, ref.margin))
    assert got.dtype == np.float32 and got.shape == (8,)
    assert got[7] == ref.n, (what, got[7], ref.n)
    if np.isnan(ref.metrics).all():
        assert np.isnan(got[:7]).all(), (what, got)
        return
    assert ref.margin > MARGIN, (what, ref.margin)
    for q in range(4):
        tol = REL * abs(ref.metrics[q]) if ref.metrics[q] != 0 else ABS_ZERO
        assert abs(float(got[q]) - ref.metrics[q]) <= tol, "%s: number %d: %r against %r (relative %.3g)" % (
            what, q, got[q], ref.metrics[q], abs(float(got[q]) - ref.metrics[q]) / max(abs(ref.metrics[q]), 1e-300))
    for q in range(4, 7):
        assert abs(float(got[q]) - ref.metrics[q]) <= ABS_A, "%s: a%d: %r against %r" % (what, q - 3, got[q], ref.metrics[q])


@pytest.mark.parametrize("name", list(mc.CASES))
def test_case_vs_reference(G, name):
    """Every case of tests/monitor_cases.py.  The two-level cases pin the median's rank: each puts rank (n - 1) // 2 on one
    side of an array's only boundary, and a neighbouring rank lands > 10x outside these bounds (checked on the CPU)."""
    c = mc.case(name)
    if name in mc.MANY_BLOCKS:
        assert mc.valid_in_high_blocks(c) > 100
    got = run(G, c)
    check(got, mc.ref(name), name)
    if name == "val-constant":
        assert np.array_equal(got[:7], np.array([0, 0, 0, 0, 1, 1, 1], np.float32)), got
    if name == "empty":
        assert got[7] == 0 and np.isnan(got[:7]).all()


REUSE = ["two_level-top11-n131073-gt_h-pred_l", "two_level-top11-n1-gt_l-pred_l", "empty", "two_level-low10-n5-gt_l-pred_h",
         "geo-37x53"]


def test_one_workspace_across_geometries(G):
    """Large n, then n = 1, then an empty mask, then n = 5, then a random window, back to back on ONE workspace (its
    layout moves with the block count, so each call finds the previous calls' counters, histograms and compact arrays
    under its own): each against its reference, and bit-equal to the same call in the reversed order."""
    from mdx import _lib
    cases = [mc.case(n) for n in REUSE]
    nbytes = max(_lib.api.mdx_depth_monitor_workspace_bytes(c.gt.shape[0], *c.window) for c in cases)
    ws = torch.full((nbytes // 8 + 1,), float("nan"), dtype=torch.float64, device=G.DEV)
    forward = [run(G, c, workspace=ws) for c in cases]
    backward = [run(G, c, workspace=ws) for c in reversed(cases)][::-1]
    for name, a, b in zip(REUSE, forward, backward):
        check(a, mc.ref(name), name + " (forward)")
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, a, b)
    # the allocator's reuse, as functional.depth_monitor runs it
    again = [run(G, c) for c in cases]
    for name, a, b in zip(REUSE, forward, again):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, a, b)


def _valid_pixel(c, b):
    r0, r1, c0, c1 = c.window
    ys, xs = np.nonzero(c.gt[b, 0, r0:r1, c0:c1].numpy() > 0)
    k = len(ys) // 2
    return r0 + int(ys[k]), c0 + int(xs[k])


@pytest.mark.parametrize("name", ["up-12x40-75x248", "up-6x20-37x53-premul", "up-37x53-37x53-shortcut"])
def test_nan_prediction(G, name):
    """One NaN that reaches a valid window pixel -- through a bilinear tap or the same-size shortcut -- gives seven NaNs and
    the count; a NaN that reaches none (outside the window, or under invalid ground truth only) changes nothing."""
    c, ref = mc.case(name), mc.ref(name)
    B, _, h, w = c.pred.shape
    gh, gw = c.gt.shape[-2:]
    r0, r1, c0, c1 = c.window
    b = B - 1
    y, x = _valid_pixel(c, b)
    pred = c.pred.clone()
    pred[b, 0, y * h // gh, x * w // gw] = float("nan")              # the source pixel that holds (y, x)'s centre: a tap of it
    hit = mc.reference(pred, c.gt, c.window, c.lo, c.hi)
    assert hit.n == ref.n and np.isnan(hit.metrics).all(), "the reference sees the NaN at a valid pixel"
    got = run(G, c, pred=pred)
    assert got[7] == ref.n and np.isnan(got[:7]).all(), got
    # all NaN: a diverged network
    got = run(G, c, pred=torch.full_like(c.pred, float("nan")))
    assert got[7] == ref.n and np.isnan(got[:7]).all(), got
    # a NaN whose taps all lie outside the window (the first prediction row: ground-truth rows well above r0)
    pred = c.pred.clone()
    pred[:, 0, 0, :] = float("nan")
    miss = mc.reference(pred, c.gt, c.window, c.lo, c.hi)
    assert np.array_equal(miss.metrics, ref.metrics), "the case's window must not reach the first prediction row"
    got_miss = run(G, c, pred=pred)
    check(got_miss, ref, name + ", NaN outside the window")
    assert np.array_equal(got_miss.view(np.uint32), run(G, c).view(np.uint32))
    if (h, w) == (gh, gw):
        # under invalid ground truth only, inside the window
        pred = c.pred.clone()
        pred[:, :, r0:r1, c0:c1][c.gt[:, :, r0:r1, c0:c1] <= 0] = float("nan")
        assert np.array_equal(mc.reference(pred, c.gt, c.window, c.lo, c.hi).metrics, ref.metrics)
        check(run(G, c, pred=pred), ref, name + ", NaN under invalid ground truth")


def test_refusals_leave_out_untouched(G):
    """mdx_depth_monitor refuses a window past the image, an empty or inverted window, a depth range that is not
    0 < min < max, a workspace one byte short and one aligned to 4 bytes only -- and writes nothing."""
    from mdx import _lib
    c = mc.case("geo-37x53")
    pred, gt = c.pred.to(G.DEV), c.gt.to(G.DEV)
    B, _, h, w = pred.shape
    gh, gw = gt.shape[-2:]
    r0, r1, c0, c1 = c.window
    nws = _lib.api.mdx_depth_monitor_workspace_bytes(B, r0, r1, c0, c1)
    buf = torch.zeros(nws // 4 + 4, device=G.DEV)                   # float32: buf[1:] is aligned to 4 bytes, not to 8
    assert buf.data_ptr() % 8 == 0
    out = torch.full((8,), -7.0, device=G.DEV)

    def call(window=(r0, r1, c0, c1), lo=c.lo, hi=c.hi, ws_ptr=buf.data_ptr(), ws_bytes=nws):
        return _lib.api.mdx_depth_monitor(_lib.ptr(pred), B, h, w, _lib.ptr(gt), gh, gw, window[0], window[1], window[2],
                                          window[3], lo, hi, _lib.ptr(out), C.c_void_p(ws_ptr), ws_bytes, _lib.stream())
    bad = {
        "rows past the image": dict(window=(r0, gh + 1, c0, c1)),
        "columns past the image": dict(window=(r0, r1, c0, gw + 1)),
        "negative row": dict(window=(-1, r1, c0, c1)),
        "r1 == r0": dict(window=(r0, r0, c0, c1)),
        "r1 < r0": dict(window=(r1, r0, c0, c1)),
        "c1 <= c0": dict(window=(r0, r1, c1, c0)),
        "min_depth 0": dict(lo=0.0),
        "min_depth negative": dict(lo=-1.0),
        "max_depth == min_depth": dict(lo=1.0, hi=1.0),
        "max_depth < min_depth": dict(lo=2.0, hi=1.0),
        "workspace one byte short": dict(ws_bytes=nws - 1),
        "workspace aligned to 4": dict(ws_ptr=buf.data_ptr() + 4),
    }
    for what, kw in bad.items():
        with pytest.raises(_lib.MdxError):
            call(**kw)
            pytest.fail("accepted: " + what)
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == -7.0).all(), what
    call()                                                           # the same call without the fault runs
    check(out.cpu().numpy(), mc.ref("geo-37x53"), "geo-37x53 after the refusals")
