"""CPU: the numpy reference of the in-kernel noise (tests/philox_ref.py) against the Random123 known-answer vectors of
Philox4x32-10, its layout conventions against a scalar evaluation, and mdx.functional.noise_state's seed derivation."""
import importlib
import math

import numpy as np
import pytest
import torch

import philox_ref as R

importlib.import_module("digging-into-self-supervised-monocular-depth-estimation_amd")
from mdx import functional as F  # noqa: E402

# Random123 (kat_vectors, philox4x32 10): counter, key, output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    got = R.philox4x32_10(ctr, *key)
    assert tuple(int(x) for x in got) == want


def test_philox_is_vectorised_elementwise():
    """an array of counters gives what the counters give one by one (the three vectors' counters under the third's key)."""
    ctrs = np.array([k[0] for k in KAT], dtype=np.uint64)
    got = R.philox4x32_10(tuple(ctrs[:, i] for i in range(4)), 0xa4093822, 0x299f31d0)
    for n in range(3):
        one = R.philox4x32_10(KAT[n][0], 0xa4093822, 0x299f31d0)
        assert [int(g[n]) for g in got] == [int(x) for x in one]
    assert [int(g[2]) for g in got] == list(KAT[2][2])


def _scalar_normal(B, H, W, S, seed, offset, s, f, b, y, x):
    """one normal, from the layout's definition and Python's own math (no numpy broadcasting)."""
    j = s * S + f
    pix = b * H * W + y * W + x
    w = [int(v) for v in R.philox4x32_10((pix, j // 4, offset & 0xffffffff, offset >> 32), seed & 0xffffffff, seed >> 32)]
    a, bb = w[2 * ((j % 4) // 2)], w[2 * ((j % 4) // 2) + 1]
    u1 = float(np.float32((a >> 8) * 2.0 ** -24 + 2.0 ** -25))
    u2 = float(np.float32((bb >> 8) * 2.0 ** -24))
    r = math.sqrt(-2.0 * math.log(u1))
    return r * (math.cos if j % 2 == 0 else math.sin)(2.0 * math.pi * u2)


def test_normals_layout():
    B, H, W, S, nscales, seed, offset = 2, 5, 7, 3, 4, (1 << 40) + 5, (1 << 32) + 3
    n = R.normals(B, H, W, S, nscales, seed, offset)
    assert n.shape == (nscales, S, B, H, W) and n.dtype == np.float64
    for (s, f, b, y, x) in [(0, 0, 0, 0, 0), (0, 1, 0, 0, 1), (1, 0, 1, 0, 0), (1, 2, 0, 4, 6), (3, 2, 1, 4, 6), (2, 1, 1, 2, 3)]:
        assert abs(n[s, f, b, y, x] - _scalar_normal(B, H, W, S, seed, offset, s, f, b, y, x)) < 1e-14
    # fewer scales / another batch size are prefixes of the same stream; every word of seed and offset matters
    assert np.array_equal(R.normals(1, H, W, S, 2, seed, offset), n[:2, :, :1])
    for other in [(seed + 1, offset), (seed + (1 << 32), offset), (seed, offset + 1), (seed, offset + (1 << 32))]:
        assert np.abs(R.normals(B, H, W, S, nscales, *other) - n).mean() > 0.5
    # N(0,1), roughly: a layout mistake that repeats words would show here
    big = R.normals(1, 64, 64, 4, 4, 1, 0)
    assert abs(big.mean()) < 5 / np.sqrt(big.size) and abs(big.var() - 1) < 5 * np.sqrt(2.0 / big.size)
    assert len(np.unique(big)) == big.size


def test_extreme_words_give_finite_normals():
    """u1 never reaches 0 (the log stays finite); the largest word's 1 - 2^-25 rounds to float32 1.0: r = 0, no NaN."""
    c, s = R.box_muller(np.array([0, 0xffffffff, 0xfffffeff], np.uint64), np.array([0, 0, 0], np.uint64))
    assert np.isfinite(c).all() and np.isfinite(s).all() and (s == 0).all()
    assert abs(c[0] - math.sqrt(-2.0 * math.log(2.0 ** -25))) < 1e-12
    assert c[1] == 0.0
    assert abs(c[2] - math.sqrt(-2.0 * math.log(1.0 - 2.0 ** -23))) < 1e-12   # 1 - 3 * 2^-25 -> 1 - 2^-23 (ties to even)


@pytest.mark.parametrize("stream", [0, 1, 7])
def test_noise_state_seed_derivation(stream):
    for seed in (0, 1234, (1 << 63) + 12345, (1 << 64) - 1):       # torch.seed() sets values up to 2^64 - 1
        st = F.noise_state("cpu", seed=seed, stream=stream)
        want = (seed + 0x9E3779B97F4A7C15 * stream) % (1 << 63)
        assert st.tensor.dtype == torch.int64 and st.tensor.tolist() == [want, 0]
        assert R.stream_seed(seed, stream) == want


@pytest.mark.parametrize("stream", [0, 1, 7])
def test_noise_state_reads_torchs_initial_seed(stream):
    before = torch.initial_seed()
    try:
        for seed in (4321, (1 << 63) + 99):
            torch.manual_seed(seed)
            assert torch.initial_seed() == seed
            st = F.noise_state("cpu", stream=stream)
            assert st.tensor.tolist() == [(seed + 0x9E3779B97F4A7C15 * stream) % (1 << 63), 0]
    finally:
        torch.manual_seed(before)
