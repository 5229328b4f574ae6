"""Reference and inputs for the train-time depth monitor (csrc/monitor.hip, mdx.functional.depth_monitor).

reference() is the plain statement of model_loss/model_metric.py:70-105 in numpy: bilinear resize and both clamps in
float32 (the values the medians select from are float32 values), exact medians by sorting, the seven numbers in float64.
The builders return small inputs at the sizes where the kernel chain changes its path: one wave, one 2048-pixel block of the
counting / compacting passes, one 8192-element trip of a radix block, the 16 x 8192 elements after which the radix blocks'
slice loop starts its second trip, and more than 1024 blocks.  Nothing here touches a GPU; tests/test_monitor_reference.py
checks this file against the project's torch-op form and checks the builders' own claims, tests/test_gpu_monitor.py runs
the kernel on every case.
"""
import collections
import functools

import numpy as np
import torch

LO, HI = 1e-3, 80.0
BLOCK = 2048                 # window pixels per block of the counting and compacting passes (monitor.hip: NT * MON_PIX)
THRESH = (1.25, 1.25 ** 2, 1.25 ** 3)

Case = collections.namedtuple("Case", "pred gt window lo hi")
Ref = collections.namedtuple("Ref", "metrics n med_gt med_pred margin")
Ref.__doc__ = """metrics: float64 [7] abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3; n: valid window pixels; the two float32 medians;
margin: the smallest relative distance of any masked pixel's max(g/p, p/g) from one of the three thresholds."""


def garg_window(gh, gw):
    """The crop compute_depth_metric derives from the ground truth's size."""
    return (int(0.40810811 * gh), int(0.99189189 * gh), int(0.03594771 * gw), int(0.96405229 * gw))


def masked(pred, gt, window, lo, hi):
    """(gt, clamped resized prediction) of the valid window pixels, float32, in pixel order (batch, row, column)."""
    gh, gw = gt.shape[-2:]
    up = torch.nn.functional.interpolate(pred.float(), [gh, gw], mode="bilinear", align_corners=False).numpy()
    up = np.clip(up, np.float32(lo), np.float32(hi))                   # NaN stays NaN
    r0, r1, c0, c1 = window
    g = gt.numpy()[:, 0, r0:r1, c0:c1]
    m = g > 0
    return g[m], up[:, 0, r0:r1, c0:c1][m]


def reference(pred, gt, window, lo=LO, hi=HI, rank_shift=0):
    """-> Ref.  rank_shift moves the rank both medians are read at away from torch.median's (n - 1) // 2: what a kernel
    with a wrong rank rule, or one that is off by one after a radix pass, would compute."""
    nan7 = np.full(7, np.nan)
    gm, pm = masked(pred, gt, window, lo, hi)
    n = int(gm.size)
    if n == 0:
        return Ref(nan7, 0, np.float32(np.nan), np.float32(np.nan), np.inf)
    r = (n - 1) // 2 + rank_shift
    med_gt = np.sort(gm)[r]
    if np.isnan(pm).any():
        return Ref(nan7, n, med_gt, np.float32(np.nan), np.inf)
    med_pred = np.sort(pm)[r]
    ratio = np.float32(med_gt) / np.float32(med_pred)
    ps = np.clip(pm * ratio, np.float32(lo), np.float32(hi))
    assert ratio.dtype == np.float32 and ps.dtype == np.float32
    g, p = gm.astype(np.float64), ps.astype(np.float64)
    t = np.maximum(g / p, p / g)
    d = g - p
    metrics = np.array([np.mean(np.abs(d) / g), np.mean(d * d / g), np.sqrt(np.mean(d * d)),
                        np.sqrt(np.mean((np.log(g) - np.log(p)) ** 2))] + [np.mean(t < k) for k in THRESH])
    margin = min(float(np.abs(t / k - 1.0).min()) for k in THRESH)
    return Ref(metrics, n, med_gt, med_pred, margin)


# ---- two-level rank cases -------------------------------------------------------------------------------------------
def _f(bits):
    return float(np.array([bits], np.uint32).view(np.float32)[0])


# (gt low, gt high, pred low, pred high): the radix pass that has to tell the two levels of an array apart
LEVELS = {
    "top11": (2.0, 40.0, 3.0, 30.0),                                            # differ in the first pass's 11 bits
    "mid11": (_f(0x41040000), _f(0x41180000), _f(0x40420000), _f(0x405c0000)),  # 8.25 / 9.5, 3.03125 / 3.4375: second pass
    "low10": (_f(0x41600000), _f(0x416003ff), _f(0x40400000), _f(0x404003ff)),  # 14 and 3, low bits 0x000 / 0x3ff: third pass
}
# low10: the two levels of an array are ~1e-4 apart (7.0e-5 of 14 = 1.75 * 2^3, 8.1e-5 of 3 = 1.5 * 2^1), so after median
# scaling p ~ g and every error number is of that order -- small, but a median on the wrong level of ONE array moves the
# ratio by a whole step and the numbers by a large share of themselves (tests/test_monitor_reference.py).
# (B, gh, gw): the window is the Garg crop of that size, so that compute_depth_metric's torch-op form sees the same case
TWO_LEVEL_SIZES = [
    ((1, 2, 3, 4, 5, 63, 64, 65), (2, 20, 16)),            # 330 window pixels
    ((2047, 2048, 2049), (2, 50, 48)),                     # 2610: two blocks
    ((8191, 8192, 8193), (3, 80, 70)),                     # 9165: five blocks
    ((131071, 131072, 131073), (2, 330, 380)),             # 136258: 67 blocks
]
TWO_LEVEL_N = [n for ns, _ in TWO_LEVEL_SIZES for n in ns]


def two_level_geometry(n):
    B, gh, gw = next(g for ns, g in TWO_LEVEL_SIZES if n in ns)
    return B, gh, gw, garg_window(gh, gw)


def rank_ks(n):
    """(k that puts the lower median on the high level, k that puts it on the low level) for n valid pixels."""
    r = (n - 1) // 2
    return r, r + 1


def two_level(n, k_gt, k_pred, geometry, seed, levels="top11"):
    """Exactly n valid window pixels at positions drawn by a seeded permutation; k_gt of them carry the low ground-truth
    level, the rest the high one; independently k_pred of their predictions carry the low prediction level.  The
    prediction has the ground truth's size, so its values reach the kernel as they are.  The rest of the window holds
    zeros and negative values, the image outside the window positive values that a wrong window edge would let in."""
    B, gh, gw, (r0, r1, c0, c1) = geometry
    g_lo, g_hi, p_lo, p_hi = LEVELS[levels]
    rng = np.random.RandomState(seed)
    nwin = B * (r1 - r0) * (c1 - c0)
    assert 0 <= k_gt <= n <= nwin and 0 <= k_pred <= n
    gt = np.where(rng.rand(B, 1, gh, gw) < 0.5, 7.0, 0.0).astype(np.float32)          # outside: valid-looking values
    pred = rng.uniform(0.5, 50.0, (B, 1, gh, gw)).astype(np.float32)
    win = rng.choice(np.array([0.0, -0.0, -2.5], np.float32), nwin)
    pos = rng.permutation(nwin)[:n]
    win[pos[:k_gt]] = g_lo
    win[pos[k_gt:]] = g_hi
    gt[:, 0, r0:r1, c0:c1] = win.reshape(B, r1 - r0, c1 - c0)
    pwin = pred[:, 0, r0:r1, c0:c1].reshape(-1).copy()
    ppos = pos[rng.permutation(n)]
    pwin[ppos[:k_pred]] = p_lo
    pwin[ppos[k_pred:]] = p_hi
    pred[:, 0, r0:r1, c0:c1] = pwin.reshape(B, r1 - r0, c1 - c0)
    return Case(torch.from_numpy(pred), torch.from_numpy(gt), (r0, r1, c0, c1), LO, HI)


# ---- geometry, upsampling and value cases ---------------------------------------------------------------------------
def _log_uniform(rng, lo, hi, shape):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), shape)).astype(np.float32)


def random_case(B, gh, gw, window, seed, pred_hw=None, only=None, lo=LO, hi=HI, density=0.2):
    """Ground truth at ~20 % density, log-uniform over 1e-2 .. 2e2 (it is not clamped: values beyond both ends occur),
    zeros and negatives elsewhere.  Prediction gt * U(0.5, 2) at the ground truth's size, or random (log-uniform over
    3e-4 .. 2e2) at pred_hw.  only = "last_batch" / "last_block": valid pixels in batch item B - 1 only / in the window's
    last, partial block only."""
    rng = np.random.RandomState(seed)
    r0, r1, c0, c1 = window
    vals = _log_uniform(rng, 1e-2, 2e2, (B, 1, gh, gw))
    hole = rng.choice(np.array([0.0, -1.0], np.float32), (B, 1, gh, gw))
    gt = np.where(rng.rand(B, 1, gh, gw) < density, vals, hole)
    if only is not None:
        wh, ww = r1 - r0, c1 - c0
        idx = np.arange(B * wh * ww).reshape(B, wh, ww)
        if only == "last_batch":
            keep = idx >= (B - 1) * wh * ww
        else:
            assert (B * wh * ww) % BLOCK, "the window's last block must be a partial one"
            keep = idx >= (B * wh * ww - 1) // BLOCK * BLOCK
        w = gt[:, 0, r0:r1, c0:c1]
        gt[:, 0, r0:r1, c0:c1] = np.where(keep, w, np.minimum(w, 0.0))
    if pred_hw is None:
        pred = np.abs(vals) * rng.uniform(0.5, 2.0, vals.shape).astype(np.float32)
    else:
        pred = _log_uniform(rng, 3e-4, 2e2, (B, 1) + tuple(pred_hw))
    return Case(torch.from_numpy(pred.astype(np.float32)), torch.from_numpy(gt.astype(np.float32)), tuple(window), lo, hi)


def one_pixel_case(seed):
    c = random_case(1, 37, 53, (17, 18, 29, 30), seed)
    c.gt[0, 0, 17, 29] = 12.5
    return c


def empty_case(seed):
    """No valid pixel inside the window, plenty outside."""
    c = random_case(2, 37, 53, (5, 33, 3, 50), seed)
    w = c.gt[:, 0, 5:33, 3:50]
    c.gt[:, 0, 5:33, 3:50] = torch.minimum(w, torch.zeros(()))
    return c


def constant_case(seed):
    """Every valid ground truth 5.0 and every prediction 7.0: after median scaling p == g."""
    c = random_case(2, 37, 53, garg_window(37, 53), seed)
    gt = torch.where(c.gt > 0, torch.full_like(c.gt, 5.0), c.gt)
    return Case(torch.full_like(c.pred, 7.0), gt, c.window, LO, HI)


def clamped_case(seed, end):
    """More than half of the predictions beyond one end of the clamp: their median is that end, exactly."""
    c = random_case(2, 37, 53, garg_window(37, 53), seed)
    rng = np.random.RandomState(seed + 1000)
    shape = tuple(c.pred.shape)
    beyond = rng.uniform(90.0, 150.0, shape) if end == "hi" else rng.uniform(1e-5, 9e-4, shape)
    pred = np.where(rng.rand(*shape) < 0.6, beyond, rng.uniform(0.5, 70.0, shape)).astype(np.float32)
    return Case(torch.from_numpy(pred), c.gt, c.window, LO, HI)


MANY_BLOCKS_GEOMETRY = (2, 1030, 1030, (0, 1030, 0, 1030))     # 2,121,800 window pixels: 1037 blocks
MANY_BLOCKS_N = 106090                                          # ~5 %; of a random permutation ~1.2 % lie in blocks >= 1024


def many_blocks_case(k_gt, k_pred, seed=5):
    """More than 1024 blocks: the strided count loop of the first radix pass and the `before` loop of high block indices.
    Some valid pixels lie in blocks >= 1024 (asserted by the tests through valid_in_high_blocks)."""
    return two_level(MANY_BLOCKS_N, k_gt, k_pred, MANY_BLOCKS_GEOMETRY, seed, "top11")


def valid_in_high_blocks(case, first_block=1024):
    r0, r1, c0, c1 = case.window
    flat = (case.gt[:, 0, r0:r1, c0:c1] > 0).reshape(-1)
    return int(flat[first_block * BLOCK:].sum())


# ---- the registry ---------------------------------------------------------------------------------------------------
def _two_level_entries():
    out = collections.OrderedDict()
    for lv_i, lv in enumerate(LEVELS):
        for n in TWO_LEVEL_N:
            hi_k, lo_k = rank_ks(n)
            for a, kg in (("h", hi_k), ("l", lo_k)):
                for b, kp in (("h", hi_k), ("l", lo_k)):
                    seed = 100 * lv_i + len(out)
                    out["two_level-%s-n%d-gt_%s-pred_%s" % (lv, n, a, b)] = functools.partial(
                        two_level, n, kg, kp, two_level_geometry(n), seed, lv)
    return out


TWO_LEVEL = _two_level_entries()
_MH, _ML = rank_ks(MANY_BLOCKS_N)
MANY_BLOCKS = collections.OrderedDict([
    ("many_blocks-gt_h-pred_l", functools.partial(many_blocks_case, _MH, _ML)),
    ("many_blocks-gt_l-pred_h", functools.partial(many_blocks_case, _ML, _MH)),
])
W37 = garg_window(37, 53)
OTHER = collections.OrderedDict([
    # window geometry
    ("geo-37x53", functools.partial(random_case, 3, 37, 53, (5, 33, 3, 50), 11)),                      # 3948 pixels, 2 blocks
    ("geo-whole_image", functools.partial(random_case, 3, 37, 53, (0, 37, 0, 53), 12)),
    ("geo-one_pixel", functools.partial(one_pixel_case, 13)),
    ("geo-2048", functools.partial(random_case, 2, 37, 53, (2, 34, 10, 42), 14)),                      # exactly one block
    ("geo-2049", functools.partial(random_case, 3, 4, 690, (2, 3, 5, 688), 15)),                       # one block + a pixel
    ("geo-last_batch_only", functools.partial(random_case, 3, 37, 53, (5, 33, 3, 50), 16, only="last_batch")),
    ("geo-last_block_only", functools.partial(random_case, 3, 37, 53, (5, 33, 3, 50), 17, only="last_block")),
    # upsampling taps (the window is the Garg crop: the torch-op form sees the same case)
    ("up-6x20-37x53-premul", functools.partial(random_case, 2, 37, 53, W37, 21, pred_hw=(6, 20))),
    ("up-12x40-75x248", functools.partial(random_case, 2, 75, 248, garg_window(75, 248), 22, pred_hw=(12, 40))),
    ("up-37x20-37x53-same_height", functools.partial(random_case, 2, 37, 53, W37, 23, pred_hw=(37, 20))),
    ("up-50x70-37x53-larger", functools.partial(random_case, 2, 37, 53, W37, 24, pred_hw=(50, 70))),
    ("up-37x53-37x53-shortcut", functools.partial(random_case, 2, 37, 53, W37, 25, pred_hw=(37, 53))),
    # values
    ("val-constant", functools.partial(constant_case, 31)),
    ("val-median_at_hi", functools.partial(clamped_case, 32, "hi")),
    ("val-median_at_lo", functools.partial(clamped_case, 33, "lo")),
    ("val-depth_range_0.1_100", functools.partial(random_case, 2, 37, 53, (5, 33, 3, 50), 34, pred_hw=(37, 53),
                                                  lo=0.1, hi=100.0)),
])
EMPTY = collections.OrderedDict([("empty", functools.partial(empty_case, 41))])
CASES = collections.OrderedDict()
for _d in (TWO_LEVEL, MANY_BLOCKS, OTHER, EMPTY):
    CASES.update(_d)


@functools.lru_cache(maxsize=8)
def case(name):
    """The case's tensors; shared between tests, which leave them unchanged."""
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def ref(name):
    c = case(name)
    return reference(c.pred, c.gt, c.window, c.lo, c.hi)
