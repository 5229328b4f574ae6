"""What tests/test_gradstats_abi.py (CPU) and tests/test_gpu_gradstats.py (GPU) share: the reference for a tensor's record, the special
values, and the six-pass history sequence.  Nothing here is imported from the product but the two ctypes structures the records are
read through, whose layout test_gradstats_abi.py holds to the header's as gcc lays it out.

The reference.  The sum of squares of a tensor's finite elements is math.fsum of their float64 squares: a float32 squared is exact
in float64 and fsum rounds the exact sum once.  The code under test adds the same n non-negative doubles in some fixed order; each of
its n - 1 additions is off by at most 2^-53 of a partial sum that is no larger than the total, so

    |got - want| <= n * 2**-53 * want.

Counts, maxima and grad_present have no tolerance."""
import math

import numpy as np
import torch

NAN_A, NAN_B = 0x7FC12345, -0x003EDCBA         # two NaNs: a positive quiet one with a payload, a negative one (0xFFC12346)
POS_INF, NEG_INF = 0x7F800000, -0x00800000
POS_ZERO, NEG_ZERO = 0, -0x80000000
DENORMAL, NEG_DENORMAL = 0x00000001, -0x7FFFFFFF
CHUNK = 4096


def storage(t):
    """The tensor's dense storage as a flat float32 host tensor, in storage order."""
    return torch.as_strided(t.detach(), (t.numel(),), (1,)).cpu().contiguous()


def put_specials(t):
    """Write the special values into the (host, float32) tensor's storage: NaNs of two payloads at the first and the last element,
    +-0, +-Inf in the middle, denormals before the end, and -- where the tensor has them -- the last element of the first chunk
    and the first element of the tensor's tail behind its last whole chunk.  In place; later writes win on tiny tensors."""
    w = torch.as_strided(t.detach(), (t.numel(),), (1,)).view(torch.int32)
    n = t.numel()
    tail = (n // CHUNK) * CHUNK
    places = [(1, POS_ZERO), (2, NEG_ZERO), (n // 2, POS_INF), (n // 2 + 1, NEG_INF), (n - 2, DENORMAL), (n - 3, NEG_DENORMAL),
              (CHUNK - 1, NEG_INF), (tail, NAN_B), (tail + 1, NEG_ZERO), (0, NAN_A), (n - 1, NAN_B)]
    for i, v in places:
        if 0 <= i < n:
            w[i] = v
    return t


def half(t, zeros):
    """-> (sumsq over finite elements by fsum, largest finite magnitude, non-finite count, zero count or 0) of one tensor."""
    x = storage(t)
    bits = x.view(torch.int32).numpy().view(np.uint32)
    finite = (bits & np.uint32(0x7F800000)) != np.uint32(0x7F800000)
    kept = x.numpy().astype(np.float64)[finite]
    sumsq = math.fsum((kept * kept).tolist())
    absmax = float(np.abs(kept).max()) if kept.size else 0.0
    nzero = int(((bits & np.uint32(0x7FFFFFFF)) == 0).sum()) if zeros else 0
    return sumsq, absmax, int((~finite).sum()), nzero


def reference(w, g):
    """The record of one (weight, gradient or None) pair, as a dict of the header's field names."""
    wsum, wmax, wnf, _ = half(w, False)
    gsum, gmax, gnf, gz = half(g, True) if g is not None else (0.0, 0.0, 0, 0)
    return dict(grad_sumsq=gsum, weight_sumsq=wsum, grad_absmax=gmax, weight_absmax=wmax, grad_nonfinite=gnf, weight_nonfinite=wnf,
                grad_zeros=gz, grad_present=int(g is not None))


def records(stats):
    """The object's record buffer, read through the ctypes structure."""
    from mdx.optim import TensorStats
    buf = stats._records
    assert buf.dtype == torch.int64 and tuple(buf.shape) == (len(stats.names), 5)
    return (TensorStats * len(stats.names)).from_buffer_copy(buf.cpu().numpy().tobytes())


def check(stats, weights, grads):
    """Every field of every record of the last pass against the reference, and host() / total_norm() against the records."""
    recs = records(stats)
    host = stats.host()
    assert list(host) == stats.names
    worst = 0.0
    for name, r, w, g in zip(stats.names, recs, weights, grads):
        want = reference(w, g)
        n = w.numel()
        for key in ("grad_sumsq", "weight_sumsq"):
            got = getattr(r, key)
            assert abs(got - want[key]) <= n * 2.0 ** -53 * want[key], (name, key, got, want[key])
            if want[key]:
                worst = max(worst, abs(got - want[key]) / want[key])
        for key in ("grad_absmax", "weight_absmax", "grad_nonfinite", "weight_nonfinite", "grad_zeros", "grad_present"):
            assert getattr(r, key) == want[key], (name, key, getattr(r, key), want[key])
        h = host[name]
        assert h["grad_norm"] == math.sqrt(r.grad_sumsq) and h["weight_norm"] == math.sqrt(r.weight_sumsq) and h["numel"] == n
        assert all(h[k] == getattr(r, k) for k in ("grad_absmax", "weight_absmax", "grad_nonfinite", "weight_nonfinite",
                                                   "grad_zeros", "grad_present"))
    assert stats.total_norm() == math.sqrt(math.fsum(r.grad_sumsq for r in recs))
    return worst


# ---- the history sequence: three tensors, six passes -----------------------------------------------------------------------------
# tensor 0 has a NaN in its gradient at passes 2 and 4; tensor 1 an Inf in its WEIGHT from pass 5 on; tensor 2 is never touched.
# The gradients of pass k are `base * SCALES[k - 1]`: the largest norm is at pass 3 for every tensor, neither the first pass nor
# the last, and not one of tensor 0's bad passes.
SCALES = (1.0, 2.0, 5.0, 4.0, 0.5, 3.0)
HISTORY_SIZES = (4097, 33, 5000)
WANT_HISTORY = [
    dict(passes=6, bad_passes=2, first_bad_pass=2, last_bad_pass=4, first_bad_weight_pass=0, max_grad_pass=3),
    dict(passes=6, bad_passes=0, first_bad_pass=0, last_bad_pass=0, first_bad_weight_pass=5, max_grad_pass=3),
    dict(passes=6, bad_passes=0, first_bad_pass=0, last_bad_pass=0, first_bad_weight_pass=0, max_grad_pass=3),
]


def run_history_sequence(device):
    """-> (the GradStats object after the six passes, the float64 norm of each tensor's pass-3 gradient).  Nothing is read from
    the object in between: one history() at the end is the caller's."""
    from mdx.optim import GradStats
    gen = torch.Generator().manual_seed(21)
    params = [torch.randn(n, generator=gen).to(device).requires_grad_(True) for n in HISTORY_SIZES]
    base = [torch.randn(n, generator=gen) for n in HISTORY_SIZES]
    stats = GradStats(params, names=["nan-grad", "inf-weight", "clean"])
    for k, scale in enumerate(SCALES, start=1):
        grads = [(b * scale).to(device) for b in base]
        if k in (2, 4):
            grads[0][4096] = float("nan")                  # the scalar tail behind a whole chunk
        if k == 5:
            with torch.no_grad():
                params[1][32] = float("inf")
        for p, g in zip(params, grads):
            p.grad = g
        stats.compute()
    return stats, [math.sqrt(math.fsum((b * 5.0).double().pow(2).tolist())) for b in base]


def check_history(stats, norms3):
    hist = stats.history()
    assert list(hist) == stats.names
    for h, want, norm, n in zip(hist.values(), WANT_HISTORY, norms3, HISTORY_SIZES):
        assert {k: h[k] for k in want} == want, (h, want)
        # the sum within n * 2^-53 (above); a square root halves a relative error and adds one rounding on either side
        assert abs(h["max_grad_norm"] - norm) <= (n / 2 + 2) * 2.0 ** -53 * norm
    stats.reset_history()
    zero = dict(passes=0, bad_passes=0, first_bad_pass=0, last_bad_pass=0, first_bad_weight_pass=0, max_grad_norm=0.0, max_grad_pass=0)
    assert all(h == zero for h in stats.history().values())
