"""GPU: the noise csrc/photo_prologue.hip draws in the kernel, value by value against tests/philox_ref.py (numpy:
Philox4x32-10 + Box-Muller in float64 on the kernel's float32 uniforms).  tests/test_gpu_prologue.py holds the
distribution; this file holds the STREAM: which counter and key words a pixel's normals come from, which word pair and
which of (cos, sin) normal j = scale * S + frame is, how the offset advances, how ranks derive their seeds.  A resume or
a refactor of the prologue that draws other numbers for the same {seed, offset} fails here.

Tolerance.  The integer part (Philox, the uniforms) is exact; what differs from the float64 reference is the hardware
log2 / sqrt / sin / cos, a few float32 roundings, and the float32 product 1e-5f * n the normals are read back through.
Measured on an MI355X over the five single-frame cases below (22 520 normals), yardstick the float64 reference: worst
|n_dev - n_ref| / max(1, |n_ref|) = 2.63e-7 (case 2,12,72; the other four 1.2e-7 .. 2.5e-7; the other tests of this
file, which draw further seeds and offsets, stay below 2.7e-7).  T = four times 2.63e-7 = 1.05e-6, rounded up to one
significant digit = 2e-6 (the margin is for seeds the table does not hold); the condition T <= 1e-3 holds with a factor
of 500 to spare.  A wrong word moves a normal by O(1).
"""
import functools

import numpy as np
import pytest
import torch

import philox_ref as R
from test_gpu_prologue import _drawn
from test_gpu_train import _synth_images

pytestmark = pytest.mark.gpu

T = 2e-6
assert T <= 1e-3      # the issue's condition on T, whatever is measured

BID = float(np.float32(1e-5))     # the kernel's 1e-5f


@pytest.fixture(scope="module")
def G():
    import gpu_util
    return gpu_util


@functools.lru_cache(maxsize=None)
def _ref(B, H, W, S, nscales, seed, offset):
    """the reference's normals [nscales, S, B, H, W], computed once per argument set and read-only."""
    n = R.normals(B, H, W, S, nscales, seed, offset)
    n.setflags(write=False)
    return n


def _state(G, seed, offset=0):
    """a generator state with exactly these two words on the device (noise_state itself reduces the seed mod 2^63)."""
    st = G.F.noise_state(G.DEV, seed=0)
    st.tensor.copy_(torch.tensor([seed, offset], dtype=torch.int64))
    return st


def _draw(G, B, H, W, S, nscales, st, advance=False):
    """-> (bid / 1e-5f as float64 [nscales, B, H, W], fi int64 [nscales, B, H, W]) on the host."""
    n, fi = _drawn(G, S, nscales, st, B=B, H=H, W=W, advance=advance)
    return n.cpu().numpy(), fi.cpu().numpy().astype(np.int64)


def _dev(n, ref):
    return np.abs(n - ref) / np.maximum(1.0, np.abs(ref))


def _assert_values(n, ref, what):
    assert n.shape == ref.shape
    d = _dev(n, ref)
    print("%s: worst |n_dev - n_ref| / max(1, |n_ref|) = %.3e over %d values (T = %g)" % (what, d.max(), d.size, T))
    assert d.max() <= T, "%s: %d of %d values off by more than T = %g, worst %g" % (what, (d > T).sum(), d.size, T, d.max())


# B, H, W, nscales, seed, offset: the 64x8 tile edge, W % 4 != 0 (the loader without 16-byte loads), B > 1 (the pixel index
# runs on across images), every nscales, high words of seed and offset
SINGLE = [
    (2, 10, 70, 4, 1234, 0),
    (1, 4, 4, 1, 5, 0),
    (3, 8, 64, 3, (1 << 40) + 5, (1 << 32) + 3),
    (2, 12, 72, 2, (1 << 63) - 1, (1 << 63) - 1),
    (1, 17, 130, 4, 9, 7),
]


@pytest.mark.parametrize("B,H,W,nscales,seed,offset", SINGLE)
def test_every_drawn_normal_equals_the_reference(G, B, H, W, nscales, seed, offset):
    st = _state(G, seed, offset)
    n, fi = _draw(G, B, H, W, 1, nscales, st)
    assert (fi == 0).all()
    _assert_values(n, _ref(B, H, W, 1, nscales, seed, offset)[:, 0], "B %d %dx%d, %d scales" % (B, H, W, nscales))
    assert st.tensor.tolist() == [seed, offset]              # advance=False: the state is read, not written


def test_advanced_offset_carries_into_the_counters_high_word(G):
    B, H, W, nscales, seed, off = 2, 10, 70, 4, 1234, (1 << 32) - 1
    st = _state(G, seed, off)
    n0, _ = _draw(G, B, H, W, 1, nscales, st, advance=True)
    assert st.tensor.tolist() == [seed, 1 << 32]
    n1, _ = _draw(G, B, H, W, 1, nscales, st, advance=True)
    assert st.tensor.tolist() == [seed, (1 << 32) + 1]
    _assert_values(n0, _ref(B, H, W, 1, nscales, seed, off)[:, 0], "offset 2^32 - 1")
    _assert_values(n1, _ref(B, H, W, 1, nscales, seed, off + 1)[:, 0], "offset 2^32, after the advance")


def test_an_images_noise_does_not_depend_on_the_batch(G):
    H, W, nscales, seed = 10, 70, 4, 1234
    one, _ = _draw(G, 1, H, W, 1, nscales, _state(G, seed))
    two, _ = _draw(G, 2, H, W, 1, nscales, _state(G, seed))
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)     # noqa: E731
    assert np.array_equal(bits(one[:, 0]), bits(two[:, 0]))
    assert np.abs(two[:, 1] - two[:, 0]).mean() > 0.5                                   # the second image: its own pixels


def test_rank_streams_are_the_documented_seeds(G):
    B, H, W, nscales = 2, 10, 70, 4
    st = G.F.noise_state(G.DEV, seed=1234, stream=1)
    seed1 = (1234 + 0x9E3779B97F4A7C15) % (1 << 63)
    assert st.tensor.tolist() == [seed1, 0]
    n, _ = _draw(G, B, H, W, 1, nscales, st)
    _assert_values(n, _ref(B, H, W, 1, nscales, seed1, 0)[:, 0], "stream 1 of seed 1234")
    assert np.abs(n - _ref(B, H, W, 1, nscales, 1234, 0)[:, 0]).mean() > 0.5            # and not rank 0's


def _left_out(gap, tol, what):
    """entries whose two smallest candidates lie within `tol` of each other: the winner there is rounding's choice.
    At most 1 % of a case's (scale, pixel) entries may be left out of an index comparison."""
    out = gap <= tol
    print("%s: %d of %d (scale, pixel) entries left out of the index comparison (%.3f %%)" % (what, out.sum(), out.size, 100.0 * out.mean()))
    assert out.mean() <= 0.01, "%s: %.3f %% of the entries are near-ties" % (what, 100.0 * out.mean())
    return out


# B, H, W, S, nscales, seed, offset: two, three and four Philox calls per pixel; with S > 1 only the minimum over the
# frames and its index are observable
SEVERAL = [
    (1, 9, 65, 2, 4, 77, 0),
    (3, 8, 64, 3, 3, (1 << 40) + 5, (1 << 32) + 3),
    (1, 17, 130, 4, 4, 9, 7),
    (2, 4, 4, 4, 1, 5, 0),
]


@pytest.mark.parametrize("B,H,W,S,nscales,seed,offset", SEVERAL)
def test_minimum_and_winner_over_several_frames(G, B, H, W, S, nscales, seed, offset):
    what = "B %d %dx%d, %d frames, %d scales" % (B, H, W, S, nscales)
    m, fi = _draw(G, B, H, W, S, nscales, _state(G, seed, offset))
    ref = _ref(B, H, W, S, nscales, seed, offset)
    _assert_values(m, ref.min(axis=1), what)
    two = np.sort(ref, axis=1)[:, :2]
    out = _left_out(two[:, 1] - two[:, 0], 2 * T, what)
    wrong = (fi != ref.argmin(axis=1)) & ~out
    assert not wrong.any(), "%s: %d winners differ from the reference's" % (what, wrong.sum())


@pytest.mark.parametrize("B,H,W,S", [(1, 9, 65, 2), (2, 16, 128, 3)])
def test_drawn_noise_on_real_images_equals_the_same_normals_injected(G, B, H, W, S):
    """noise reaches the training kernel through bidfi alone: with real, differing images, the prologue that draws
    {seed, offset} and the prologue that is handed the reference's normals of {seed, offset} write the same maps."""
    nscales, seed, offset = 4, 4242, 3
    what = "B %d %dx%d, %d frames, real images" % (B, H, W, S)
    colors = _synth_images(B, H, W, S, seed=11)[0]
    tgt, srcs = G.t(colors[0]), [G.t(x) for x in colors[1:]]
    ref = _ref(B, H, W, S, nscales, seed, offset)
    n32 = [np.ascontiguousarray(ref[s].transpose(1, 0, 2, 3)).astype(np.float32) for s in range(nscales)]     # [B, S, H, W]
    a = G.F.photometric_prologue(tgt, srcs, nscales, rng=_state(G, seed, offset), need_ident=True)
    b = G.F.photometric_prologue(tgt, srcs, nscales, noises=[G.t(x) for x in n32], need_ident=True)
    assert torch.equal(a["tstat"], b["tstat"]) and torch.equal(a["ident"], b["ident"])
    ident = b["ident"].cpu().numpy().astype(np.float64)
    assert len(np.unique(ident)) > ident.size // 2                    # real images: the identity losses take part
    gaps, tols, wrongs = [], [], []
    for s in range(nscales):
        bid_a, bid_b = (x["bidfi"][s][..., 0].cpu().numpy() for x in (a, b))
        fi_a, fi_b = (x["bidfi"][s][..., 1].contiguous().view(torch.int32).cpu().numpy().astype(np.int64)[:, None] for x in (a, b))
        n = n32[s].astype(np.float64)
        # per candidate: 1e-5 * T * max(1, |n|) + one float32 ulp of bid
        tol = BID * T * np.maximum(1.0, np.abs(n)) + np.spacing(np.abs(bid_b))[:, None].astype(np.float64)
        v = ident + BID * n                                           # the injected run's candidates
        order = np.argsort(v, axis=1)[:, :2]
        pair_tol = np.take_along_axis(tol, order, 1).max(axis=1)
        gaps.append(np.diff(np.take_along_axis(v, order, 1), axis=1)[:, 0])
        tols.append(2 * pair_tol)
        wrongs.append(fi_a[:, 0] != fi_b[:, 0])
        # |min_f a_f - min_f b_f| <= the larger deviation of the two runs' winners (the same candidate wherever fi agrees)
        bound = np.maximum(np.take_along_axis(tol, fi_a, 1), np.take_along_axis(tol, fi_b, 1))[:, 0]
        err = np.abs(bid_a.astype(np.float64) - bid_b.astype(np.float64))
        print("%s, scale %d: worst |bid drawn - bid injected| / bound = %.3g" % (what, s, (err / bound).max()))
        assert (err <= bound).all(), "%s, scale %d: %d best identity values differ" % (what, s, (err > bound).sum())
    out = _left_out(np.stack(gaps), np.stack(tols), what)
    wrong = np.stack(wrongs) & ~out
    assert not wrong.any(), "%s: %d winners differ between drawn and injected noise" % (what, wrong.sum())
