"""CPU: tests/monitor_cases.py checked against the project's torch-op form of the depth monitor, and the claims of its case
builders checked against the cases they build.  What tests/test_gpu_monitor.py asserts on the GPU rests on these."""
import numpy as np
import pytest
import torch

import monitor_cases as mc

GPU_REL = 2e-5            # tests/test_gpu_monitor.py's bound on the four error numbers
GPU_ABS_A = 1e-7          # ... and on a1..a3
MARGIN = 1e-5


def torch_op_form(c, monkeypatch):
    import model_loss.model_metric as mm
    monkeypatch.setattr(mm, "METRIC_CAPACITY", 1.0)
    out = mm.compute_depth_metric({("depth", 0): c.gt}, {("depth", 0, 0): c.pred}, "torch")
    return np.array([float(v) for v in out])


QUALIFY = [n for n, b in mc.CASES.items()
           if n not in mc.MANY_BLOCKS and n != "val-depth_range_0.1_100" and (n in mc.TWO_LEVEL or n.startswith(("up-", "val-")))]


def test_enough_cases_reach_the_torch_op_form():
    assert len(QUALIFY) == len(mc.TWO_LEVEL) + 8


@pytest.mark.parametrize("name", QUALIFY)
def test_reference_vs_torch_op_form(name, monkeypatch):
    """The cases whose window is the crop compute_depth_metric derives itself (and whose clamp is 1e-3 .. 80): the float64
    reference against the float32 torch ops, 1e-5 relative (1e-7 absolute where the reference is exactly 0).
    One number of one family cannot meet that in float32 and is bounded by the format instead: rmse_log of the low10
    levels, where prediction and ground truth agree to 1e-4 after scaling and torch.log(g) - torch.log(p) is the
    difference of two logarithms rounded to eps * |log g| each."""
    c = mc.case(name)
    assert tuple(c.window) == mc.garg_window(*c.gt.shape[-2:]) and (c.lo, c.hi) == (mc.LO, mc.HI)
    ref = mc.ref(name)
    got = torch_op_form(c, monkeypatch)
    for q in range(7):
        tol = 1e-5 * abs(ref.metrics[q]) if ref.metrics[q] != 0 else 1e-7
        if q == 3 and "low10" in name:
            gm, _ = mc.masked(c.pred, c.gt, c.window, c.lo, c.hi)
            tol += 2 * np.finfo(np.float32).eps * float(np.abs(np.log(gm.astype(np.float64))).max())
        assert abs(got[q] - ref.metrics[q]) <= tol, (name, q, got[q], ref.metrics[q])


def test_reference_nan_and_empty(monkeypatch):
    """An empty mask and a NaN prediction at a valid pixel: seven NaNs from the reference (the torch ops' four error numbers
    are NaN as well; their a1..a3 count a failed comparison as a miss); a NaN under invalid ground truth changes nothing."""
    c = mc.case("empty")
    ref = mc.ref("empty")
    assert ref.n == 0 and np.isnan(ref.metrics).all()
    c = mc.case("up-37x53-37x53-shortcut")
    r0, r1, c0, c1 = c.window
    ys, xs = np.nonzero(c.gt[1, 0].numpy() > 0)
    inside = [(y, x) for y, x in zip(ys, xs) if r0 <= y < r1 and c0 <= x < c1]
    y, x = inside[len(inside) // 2]
    pred = c.pred.clone()
    pred[1, 0, y, x] = float("nan")
    bad = mc.reference(pred, c.gt, c.window)
    assert bad.n == mc.ref("up-37x53-37x53-shortcut").n and np.isnan(bad.metrics).all()
    assert np.isnan(torch_op_form(mc.Case(pred, c.gt, c.window, c.lo, c.hi), monkeypatch)[:4]).all()
    ys, xs = np.nonzero(c.gt[0, 0].numpy() <= 0)
    pred = c.pred.clone()
    pred[0, 0, ys[0], xs[0]] = float("nan")
    same = mc.reference(pred, c.gt, c.window)
    assert np.array_equal(same.metrics, mc.ref("up-37x53-37x53-shortcut").metrics)


@pytest.mark.parametrize("name", list(mc.CASES))
def test_case_claims(name):
    """Valid counts, the medians the value cases promise, valid pixels in blocks >= 1024, and the condition under which
    a1..a3 can be compared exactly: no masked pixel's max(g/p, p/g) within 1e-5 relative of a threshold."""
    c, ref = mc.case(name), mc.ref(name)
    r0, r1, c0, c1 = c.window
    B, _, gh, gw = c.gt.shape
    assert 0 <= r0 < r1 <= gh and 0 <= c0 < c1 <= gw
    assert c.pred.dtype == torch.float32 and c.gt.dtype == torch.float32
    nwin = B * (r1 - r0) * (c1 - c0)
    assert ref.n == int((c.gt[:, 0, r0:r1, c0:c1] > 0).sum())
    assert (c.gt == 0).any() and (c.gt < 0).any(), "zeros and negative values in the ground truth"
    if nwin < c.gt.numel():
        out = c.gt.clone()
        out[:, 0, r0:r1, c0:c1] = 0
        assert (out > 0).any(), "positive ground truth outside the window"
    assert ref.margin > MARGIN, (name, ref.margin)
    if name in mc.TWO_LEVEL or name in mc.MANY_BLOCKS:
        n = int(name.split("-n")[1].split("-")[0]) if name in mc.TWO_LEVEL else mc.MANY_BLOCKS_N
        lv = mc.LEVELS[name.split("-")[1]] if name in mc.TWO_LEVEL else mc.LEVELS["top11"]
        assert ref.n == n
        assert ref.med_gt == np.float32(lv[1] if "gt_h" in name else lv[0])
        assert ref.med_pred == np.float32(lv[3] if "pred_h" in name else lv[2])
        assert c.pred.shape == c.gt.shape
    if name in mc.MANY_BLOCKS:
        assert (nwin + mc.BLOCK - 1) // mc.BLOCK == 1037
        assert mc.valid_in_high_blocks(c) > 100
    if name == "empty":
        assert ref.n == 0
    if name == "geo-one_pixel":
        assert nwin == 1 and ref.n == 1
    if name == "geo-2048":
        assert nwin == mc.BLOCK
    if name == "geo-2049":
        assert nwin == mc.BLOCK + 1
    if name == "geo-whole_image":
        assert nwin == c.gt.numel()
    if name.startswith("geo-") and name != "geo-one_pixel":
        gm, _ = mc.masked(c.pred, c.gt, c.window, c.lo, c.hi)
        assert gm.min() < c.lo * 100 and gm.max() > c.hi, "ground truth beyond both ends of the clamp"
    if name == "geo-last_batch_only":
        assert ref.n > 0 and not (c.gt[:2, 0, r0:r1, c0:c1] > 0).any()
    if name == "geo-last_block_only":
        flat = (c.gt[:, 0, r0:r1, c0:c1] > 0).reshape(-1)
        first = (nwin - 1) // mc.BLOCK * mc.BLOCK
        assert first > 0 and nwin % mc.BLOCK and ref.n > 0 and not flat[:first].any()
    if name == "val-constant":
        assert ref.n > 100 and np.array_equal(ref.metrics, [0, 0, 0, 0, 1, 1, 1])
    if name == "val-median_at_hi":
        assert ref.med_pred == np.float32(80.0)
    if name == "val-median_at_lo":
        assert ref.med_pred == np.float32(1e-3)
    if name == "val-depth_range_0.1_100":
        _, pm = mc.masked(c.pred, c.gt, c.window, c.lo, c.hi)
        assert (c.lo, c.hi) == (0.1, 100.0) and (pm == np.float32(0.1)).any() and (pm == np.float32(100.0)).any()
    if name.startswith("up-"):
        h, w = (int(v) for v in name.split("-")[1].split("x"))
        assert tuple(c.pred.shape[-2:]) == (h, w)
        assert (gh + gw <= 128) == (name != "up-12x40-75x248")


def differs(a, b):
    """Some of the seven numbers differs by more than 10x what the GPU test tolerates."""
    err = np.abs(a - b)
    return bool((err[:4] > 10 * GPU_REL * np.abs(b[:4])).any() or (err[4:] > 10 * GPU_ABS_A).any())


def crossings(name, n, shift):
    """The arrays whose median moves to the other level when the rank is read at r + shift.  A two-level array has one
    boundary, so it tells rank r from ONE neighbour: with k = r + 1 low values the element at r is the last low one and
    r + 1 is high (r - 1 is low as well: the same median); with k = r the element at r is the first high one, r - 1 is low."""
    r = (n - 1) // 2
    if not 0 <= r + shift < n:
        return []
    tag = "_l" if shift > 0 else "_h"
    return [a for a in ("gt", "pred") if a + tag in name]


@pytest.mark.parametrize("name", list(mc.TWO_LEVEL) + list(mc.MANY_BLOCKS))
def test_two_level_cases_separate_the_ranks(name):
    """A kernel that reads a neighbouring rank must land outside the GPU test's tolerance, or the case proves nothing:
    reference(rank_shift = -1 / +1) must differ from reference() by more than 10x that tolerance wherever the shifted
    rank exists and lies across the boundary of an array.  (Where it lies on the same level of both arrays nothing can
    differ; that is asserted too.)

    One family cannot show a shift that crosses BOTH boundaries, and is not asked to: the low10 levels.  There every
    error is first order in the level steps, the pixels fall into four groups (g low / high x p low / high) of a quarter
    each, and moving both medians only swaps which groups carry which error: the means agree to second order (measured:
    3e-5 relative).  The same holds for n = 2 (one pixel per ground-truth level).  The two arrays are selected
    independently (one grid row each), and the mixed cases gt_h-pred_l / gt_l-pred_h of the same n cross one boundary
    per shift: test_every_n_separates_each_array_and_direction checks that these cover every array and direction."""
    c, ref = mc.case(name), mc.ref(name)
    for shift in (-1, +1):
        cross = crossings(name, ref.n, shift)
        if not 0 <= (ref.n - 1) // 2 + shift < ref.n:
            continue
        other = mc.reference(c.pred, c.gt, c.window, c.lo, c.hi, rank_shift=shift)
        if not cross:
            assert other.med_gt == ref.med_gt and other.med_pred == ref.med_pred
        elif "low10" in name and (len(cross) == 2 or ref.n == 2):
            assert (other.med_gt != ref.med_gt) == ("gt" in cross) and (other.med_pred != ref.med_pred) == ("pred" in cross)
        else:
            assert differs(other.metrics, ref.metrics), (name, shift, other.metrics, ref.metrics)


def test_every_n_separates_each_array_and_direction():
    """Over the four (k_gt, k_pred) cases of one n and level pair: for each array and each neighbouring rank that exists,
    a case in which that shift crosses that array's boundary ALONE (so that the test above demands separation of it)."""
    for lv in mc.LEVELS:
        for n in mc.TWO_LEVEL_N:
            names = [k for k in mc.TWO_LEVEL if k.startswith("two_level-%s-n%d-" % (lv, n))]
            assert len(names) == 4
            r = (n - 1) // 2
            for shift in (-1, +1):
                if not 0 <= r + shift < n or (n == 2 and lv == "low10"):
                    continue
                for arr in ("gt", "pred"):
                    assert any(crossings(k, n, shift) == [arr] for k in names), (lv, n, shift, arr)
    for shift in (-1, +1):
        for arr in ("gt", "pred"):
            assert any(crossings(k, mc.MANY_BLOCKS_N, shift) == [arr] for k in mc.MANY_BLOCKS)
