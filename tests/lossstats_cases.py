"""What tests/test_loss_stats_abi.py (CPU) and tests/test_gpu_loss_stats.py (GPU) share: the reference for a (scale, image)'s record
and for a scale's history, the special values, and the six-pass history sequence.  Nothing here is imported from the product but the
two ctypes structures the records are read through, whose layout test_loss_stats_abi.py holds to the header's as gcc lays them out.

The reference is plain torch and numpy on the CPU: counts by bincount, sums by math.fsum of float64 terms.  A disparity and its
square are exact in float64, so disp_sum and disp_sumsq are sums in double of exact terms and the code under test differs from the
reference only in the order of its additions:

    |got - want| <= n * 2**-52 * sum(|term|),    n = the element count of the image

which is twice the worst-case bound of any summation order and covers the reference's own rounding.  Counts are exact; disp_min and
disp_max are equal by value; max_masked_share and min_disp_range are bit-equal to Python's `masked / pixels` and
`float(max) - float(min)`, each one correctly rounded double operation on exact inputs."""
import math

import numpy as np
import torch

NANS = (0x7FC12345, -0x003EDCBA, 0x7F800001)   # a positive quiet NaN with a payload, a negative one (0xFFC12346), a signalling one
POS_INF, NEG_INF = 0x7F800000, -0x00800000
DENORMAL, NEG_DENORMAL = 0x00000001, -0x7FFFFFFF
BINS = 8


def limit(S, automask):
    return 2 * S if automask else S


def index_map(B, H, W, S, automask, gen, illegal=True, dtype=torch.uint8):
    """[B,H,W]: every legal value, and (illegal) a few that are not: the first one past the legal ones, 2S + 3, and 255."""
    top = limit(S, automask)
    m = torch.randint(0, top, (B, H, W), generator=gen)
    flat = m.view(B, -1)
    n = flat.shape[1]
    for b in range(B):
        for c in range(top):                                  # every legal value at least once where there is room
            if c < n:
                flat[b, (c * 7 + b) % n] = c
    if illegal:
        for b in range(B):
            for k, v in enumerate((top, 2 * S + 3, 255)):
                flat[b, (n - 1 - 5 * k - b) % n] = v
    return m.to(dtype)


def disparity(B, h, w, gen, specials=True):
    """[B,1,h,w] in (0, 1) with (specials) +-Inf, NaNs of three payloads and denormals of both signs, in every image, placed at the
    first and the last element, around the middle and at the chunk edge where the image has one."""
    d = torch.rand(B, 1, h, w, generator=gen)
    if specials:
        bits = d.view(torch.int32).view(B, -1)
        n = bits.shape[1]
        places = [(n // 2, POS_INF), (n // 3, NEG_INF), (n - 2, DENORMAL), (n - 3, NEG_DENORMAL), (4095, NANS[2]), (4096, NEG_INF),
                  (1, NANS[1]), (0, NANS[0]), (n - 1, NANS[1])]
        for i, v in places:
            if 0 <= i < n:
                bits[:, i] = v
    return d


def reference(idx, disp, S, automask):
    """The record of one image ([H,W] index map or None, [1,h,w] disparity or None) as a dict of the header's field names;
    `_abs_sum` and `_abs_sumsq` are the sums of the terms' magnitudes, for the tolerance."""
    r = dict(disp_sum=0.0, disp_sumsq=0.0, disp_min=0.0, disp_max=0.0, winner=[0] * BINS, bad_index=0, disp_nonfinite=0,
             index_present=int(idx is not None), disp_present=int(disp is not None), _abs_sum=0.0, _abs_sumsq=0.0, _n=0)
    if idx is not None:
        v = idx.detach().cpu().reshape(-1).numpy().astype(np.int64)
        legal = (v >= 0) & (v < limit(S, automask))
        r["winner"] = np.bincount(v[legal], minlength=BINS)[:BINS].tolist()
        r["bad_index"] = int((~legal).sum())
        assert sum(r["winner"]) + r["bad_index"] == v.size
    if disp is not None:
        x = disp.detach().cpu().reshape(-1).contiguous()
        bits = x.view(torch.int32).numpy().view(np.uint32)
        finite = (bits & np.uint32(0x7F800000)) != np.uint32(0x7F800000)
        kept = x.numpy()[finite].astype(np.float64)
        r["disp_sum"], r["disp_sumsq"] = math.fsum(kept.tolist()), math.fsum((kept * kept).tolist())
        r["_abs_sum"], r["_abs_sumsq"], r["_n"] = math.fsum(np.abs(kept).tolist()), r["disp_sumsq"], int(x.numel())
        if kept.size:
            r["disp_min"], r["disp_max"] = float(kept.min()), float(kept.max())
        r["disp_nonfinite"] = int((~finite).sum())
    return r


def reference_history(passes, B, H, W, S, automask, static_share):
    """passes: per pass the list of one scale's reference records (one per image) -> the scale's history as a dict."""
    pixels = H * W
    h = dict(passes=0, images=0, winner_total=[0] * BINS, bad_passes=0, first_bad_pass=0, static_images=0, first_static_pass=0,
             last_static_pass=0, max_masked_share=0.0, max_masked_pass=0, min_disp_range=0.0, min_disp_range_pass=0)
    for k, recs in enumerate(passes, start=1):
        h["passes"] = k
        if any(r["bad_index"] > 0 or r["disp_nonfinite"] > 0 for r in recs):
            h["bad_passes"] += 1
            h["first_bad_pass"] = h["first_bad_pass"] or k
        for r in recs:
            if r["index_present"]:
                h["images"] += 1
                h["winner_total"] = [a + b for a, b in zip(h["winner_total"], r["winner"])]
                if automask:
                    masked = sum(r["winner"][:S])
                    if masked >= static_share * pixels:
                        h["static_images"] += 1
                        h["first_static_pass"] = h["first_static_pass"] or k
                        h["last_static_pass"] = k
                    if masked / pixels > h["max_masked_share"]:
                        h["max_masked_share"], h["max_masked_pass"] = masked / pixels, k
            if r["disp_present"] and r["disp_nonfinite"] < r["_n"]:
                rng = float(r["disp_max"]) - float(r["disp_min"])
                if h["min_disp_range_pass"] == 0 or rng < h["min_disp_range"]:
                    h["min_disp_range"], h["min_disp_range_pass"] = rng, k
    return h


def references(stats, idx_list, disp_list):
    """[scale][image] reference records for the lists compute() was given."""
    return [[reference(None if i is None else i[b], None if d is None else d[b], stats.S, stats.automask) for b in range(stats.B)]
            for i, d in zip(idx_list, disp_list)]


def records(stats):
    """The object's record buffer, read through the ctypes structure: [scale][image]."""
    from mdx.loss_stats import LossStatsRecord
    n, B = len(stats.scales_hw), stats.B
    buf = stats._records
    assert buf.dtype == torch.int64 and tuple(buf.shape) == (n * B, 9)
    recs = (LossStatsRecord * (n * B)).from_buffer_copy(buf.cpu().numpy().tobytes())
    return [[recs[s * B + b] for b in range(B)] for s in range(n)]


def check(stats, idx_list, disp_list):
    """Every field of every record of the last pass against the reference, and host() against the records.  -> the references."""
    want_all = references(stats, idx_list, disp_list)
    got_all = records(stats)
    host = stats.host()
    pixels = stats.H * stats.W
    for s, (gots, wants) in enumerate(zip(got_all, want_all)):
        for b, (r, want) in enumerate(zip(gots, wants)):
            where = "scale %d image %d" % (s, b)
            for key, mag in (("disp_sum", "_abs_sum"), ("disp_sumsq", "_abs_sumsq")):
                got = getattr(r, key)
                assert abs(got - want[key]) <= want["_n"] * 2.0 ** -52 * want[mag], (where, key, got, want[key])
            assert r.disp_min == want["disp_min"] and r.disp_max == want["disp_max"], (where, r.disp_min, r.disp_max, want)
            assert list(r.winner) == want["winner"], (where, list(r.winner), want["winner"])
            for key in ("bad_index", "disp_nonfinite", "index_present", "disp_present"):
                assert getattr(r, key) == want[key], (where, key, getattr(r, key), want[key])
            h = host[s][b]
            masked = sum(want["winner"][:stats.S]) if stats.automask else 0
            assert h["masked_share"] == masked / pixels and list(h["shares"]) == stats.channel_names
            assert [h["shares"][n] for n in stats.channel_names] == [c / pixels for c in want["winner"][:len(stats.channel_names)]]
            assert (h["disp_min"], h["disp_max"], h["bad_index"], h["disp_nonfinite"], h["index_present"], h["disp_present"]) == \
                   (r.disp_min, r.disp_max, r.bad_index, r.disp_nonfinite, r.index_present, r.disp_present)
            finite = want["_n"] - want["disp_nonfinite"]
            if finite:
                mean = r.disp_sum / finite
                assert h["disp_mean"] == mean and h["disp_std"] == math.sqrt(max(r.disp_sumsq / finite - mean * mean, 0.0))
            else:
                assert h["disp_mean"] == 0.0 and h["disp_std"] == 0.0
    return want_all


INT_FIELDS = ("passes", "images", "winner_total", "bad_passes", "first_bad_pass", "static_images", "first_static_pass",
              "last_static_pass", "max_masked_pass", "min_disp_range_pass")


def check_history(stats, want):
    """stats.history() against one reference history per scale: the integer fields exactly, the two doubles bit for bit."""
    got = stats.history()
    assert len(got) == len(want) == len(stats.scales_hw)
    for s, (g, w) in enumerate(zip(got, want)):
        assert {k: g[k] for k in INT_FIELDS} == {k: w[k] for k in INT_FIELDS}, (s, g, w)
        assert g["max_masked_share"].hex() == w["max_masked_share"].hex(), (s, g["max_masked_share"], w["max_masked_share"])
        assert g["min_disp_range"].hex() == w["min_disp_range"].hex(), (s, g["min_disp_range"], w["min_disp_range"])
        total = w["images"] * stats.H * stats.W
        masked = sum(w["winner_total"][:stats.S]) if stats.automask else 0
        assert g["masked_share"] == (masked / total if total else 0.0)


# ---- the history sequence: B = 2, 4 x 4 = 16 pixels, S = 2 with the auto-mask, two scales (4 x 4 and 2 x 2), static_share = 0.5 -----
# MASKED[k - 1][b]: the masked pixels of image b at pass k.  7 of 16 is just below the threshold, 8 of 16 is exactly on it and counts;
# the largest share, 8 / 16, comes at pass 2 and again at pass 3: the first pass of the tie stays.  Pass 4 has a NaN in the disparity
# of scale 0, pass 5 two illegal indices (4 = 2S and 255), which both scales see since the index maps are the same at every scale.
# SPAN[k - 1]: the disparities of pass k are 0.25 + base * SPAN -- the smallest range of scale 0 is at pass 3; at pass 6 image 1 of
# scale 1 is a constant, range 0.
HISTORY_SHAPE = dict(B=2, H=4, W=4, S=2, scales_hw=[(4, 4), (2, 2)], automask=True, static_share=0.5)
MASKED = ((7, 3), (8, 2), (8, 0), (5, 1), (2, 2), (6, 0))
SPAN = (0.5, 0.25, 0.0625, 0.75, 0.5, 0.125)
WANT_HISTORY = [
    dict(passes=6, images=12, bad_passes=2, first_bad_pass=4, static_images=2, first_static_pass=2, last_static_pass=3,
         max_masked_share=0.5, max_masked_pass=2, min_disp_range_pass=3),
    dict(passes=6, images=12, bad_passes=1, first_bad_pass=5, static_images=2, first_static_pass=2, last_static_pass=3,
         max_masked_share=0.5, max_masked_pass=2, min_disp_range=0.0, min_disp_range_pass=6),
]


def history_sequence():
    """-> per pass (idx_list, disp_list) of CPU tensors (uint8 index maps, float32 disparities)."""
    gen = torch.Generator().manual_seed(33)
    base = [torch.rand(2, 1, h, w, generator=gen) for h, w in HISTORY_SHAPE["scales_hw"]]
    for b in base:                                             # every image spans exactly 0 .. 1
        b.view(2, -1)[:, 0], b.view(2, -1)[:, 1] = 0.0, 1.0
    out = []
    for k, (masked, span) in enumerate(zip(MASKED, SPAN), start=1):
        idx = torch.empty(2, 16, dtype=torch.uint8)
        for b, m in enumerate(masked):
            vals = [c % 2 for c in range(m)] + [2 + c % 2 for c in range(16 - m)]         # m identity wins, 16 - m source wins
            idx[b] = torch.tensor(vals, dtype=torch.uint8)[torch.randperm(16, generator=gen)]
        if k == 5:
            pos = [i for i in range(16) if idx[0, i] >= 2][:2]                              # masked count unchanged
            idx[0, pos[0]], idx[0, pos[1]] = 4, 255
        idx = idx.view(2, 4, 4)
        disps = [0.25 + b * span for b in base]
        if k == 4:
            disps[0][1, 0, 2, 3] = float("nan")
        if k == 6:
            disps[1][1] = 0.375
        out.append(([idx, idx.clone()], disps))
    return out


def run_history_sequence(device, dtype=torch.uint8):
    """-> (the LossStats object after the six passes, the reference histories).  Nothing is read from the object in between."""
    from mdx.loss_stats import LossStats
    stats = LossStats(device=device, **HISTORY_SHAPE)
    per_scale = [[], []]
    for idx_list, disp_list in history_sequence():
        stats.compute([i.to(device, dtype) for i in idx_list], [d.to(device) for d in disp_list])
        for s, recs in enumerate(references(stats, idx_list, disp_list)):
            per_scale[s].append(recs)
    shape = {k: HISTORY_SHAPE[k] for k in ("B", "H", "W", "S", "automask", "static_share")}
    want = [reference_history(p, **shape) for p in per_scale]
    for w, fixed in zip(want, WANT_HISTORY):                   # the reference itself against the sequence as it was designed
        assert {k: w[k] for k in fixed} == fixed, (w, fixed)
    return stats, want


def check_reset(stats):
    stats.reset_history()
    for h in stats.history():
        assert all(h[k] == (0 if k != "winner_total" else [0] * BINS) for k in INT_FIELDS)
        assert h["max_masked_share"] == 0.0 and h["min_disp_range"] == 0.0 and h["masked_share"] == 0.0
