"""The stream of csrc/photo_prologue.hip's in-kernel noise, written out in numpy (no GPU): Philox4x32-10 (Salmon et al.,
SC'11) keyed by the 64-bit seed, counter (pixel, call, offset_lo, offset_hi), Box-Muller in float64 on the float32
uniforms the kernel forms.  tests/test_philox_ref.py holds philox4x32_10 to the Random123 known-answer vectors; the GPU
tests (tests/test_gpu_noise_pin.py) hold every normal the kernel draws to normals()."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # key increments (Weyl sequence)
MASK = 0xFFFFFFFF
STREAM_STRIDE = 0x9E3779B97F4A7C15       # mdx.functional.noise_state: seed + STREAM_STRIDE * stream, mod 2^63


def philox4x32_10(counter_words, k0, k1):
    """counter_words: four uint64 arrays (or scalars) holding 32-bit words, broadcast against each other; k0, k1: the
    key's words.  -> tuple of four uint64 arrays holding the 32-bit output words."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) for c in counter_words])
    k0, k1 = int(k0) & MASK, int(k1) & MASK
    m0, m1, mask, sh = np.uint64(M0), np.uint64(M1), np.uint64(MASK), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                    # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ np.uint64(k0), p1 & mask, (p0 >> sh) ^ c3 ^ np.uint64(k1), p0 & mask
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def box_muller(a, b):
    """two words -> (r cos 2 pi u2, r sin 2 pi u2), r = sqrt(-2 ln u1), in float64 on the kernel's float32 uniforms:
    u1 = float32((a >> 8) 2^-24 + 2^-25) (one rounding: the kernel's fma), u2 = float32((b >> 8) 2^-24) (exact)."""
    sh = np.uint64(8)
    u1 = ((a >> sh).astype(np.float64) * 2.0 ** -24 + 2.0 ** -25).astype(np.float32).astype(np.float64)
    u2 = ((b >> sh).astype(np.float64) * 2.0 ** -24).astype(np.float32).astype(np.float64)
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)


def normals(B, H, W, S, nscales, seed, offset):
    """-> float64 [nscales, S, B, H, W]: normal j = scale * S + frame of pixel pix = b H W + y W + x is entry j % 4 of
    call j // 4, a call's entries being (cos, sin) of words (x, y), then (cos, sin) of words (z, w)."""
    seed, offset = int(seed), int(offset)
    pix = np.arange(B * H * W, dtype=np.uint64)
    ncalls = (nscales * S + 3) // 4
    entries = []
    for c in range(ncalls):
        x, y, z, w = philox4x32_10((pix, c, offset & MASK, (offset >> 32) & MASK), seed & MASK, (seed >> 32) & MASK)
        entries += list(box_muller(x, y)) + list(box_muller(z, w))
    out = np.empty((nscales, S, B, H, W), np.float64)
    for s in range(nscales):
        for f in range(S):
            out[s, f] = entries[s * S + f].reshape(B, H, W)
    return out


def stream_seed(seed, stream):
    """the seed mdx.functional.noise_state puts on the device for a data-parallel rank."""
    return (int(seed) + STREAM_STRIDE * int(stream)) % (1 << 63)
