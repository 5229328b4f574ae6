"""CPU, float64: the identity csrc/upconv_nhwc.hip rests on, stated in plain torch.

    conv3x3(ReflectionPad2d(1)(nearest_x2(a)), W)[2Y+py, 2X+px] = sum over (dy, dx) of Wq[py][px][dy][dx] @ a[clamp(Y+dy), clamp(X+dx)]

with off(p, k) = floor((p + k - 1) / 2) the low-resolution offset kernel tap k reads in phase p, Wq the sum of the taps with the
same offsets, and the reflection pad of the x2 map a clamp of the low-resolution index; and its transpose for the weight:
gweight[ky][kx] = sum over the phases of G[py][px][off(py, ky)][off(px, kx)], G the 16 phase/offset outer-product sums."""
import pytest
import torch
import torch.nn.functional as TF

SHAPES = [(1, 1, 4), (2, 2, 4), (1, 3, 8), (2, 5, 12), (3, 7, 20), (1, 33, 36), (2, 24, 80)]


def off(p, k):
    return (p + k - 1) // 2


def op_sequence(raw, bias, weight):
    a = TF.elu(raw + bias.view(1, -1, 1, 1))
    return TF.conv2d(TF.pad(TF.interpolate(a, scale_factor=2, mode="nearest"), (1, 1, 1, 1), mode="reflect"), weight)


def shifted(a, dy, dx):
    """a[clamp(Y + dy), clamp(X + dx)] for every (Y, X)."""
    h, w = a.shape[2:]
    ys = (torch.arange(h) + dy).clamp(0, h - 1)
    xs = (torch.arange(w) + dx).clamp(0, w - 1)
    return a[:, :, ys][:, :, :, xs]


def phase_weights(weight):
    """{(py, px, dy, dx): [Cout, Cin]} -- the 3x3 taps summed by the offsets they read."""
    wq = {}
    for py in range(2):
        for px in range(2):
            for ky in range(3):
                for kx in range(3):
                    key = (py, px, off(py, ky), off(px, kx))
                    wq[key] = wq.get(key, 0) + weight[:, :, ky, kx]
    return wq


def phase_form(raw, bias, weight):
    a = TF.elu(raw + bias.view(1, -1, 1, 1))
    B, _, h, w = a.shape
    out = a.new_zeros(B, weight.shape[0], 2 * h, 2 * w)
    for (py, px, dy, dx), m in phase_weights(weight).items():
        out[:, :, py::2, px::2] += torch.einsum("oc,bchw->bohw", m, shifted(a, dy, dx))
    return out


def _inputs(B, h, w, seed=0):
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(B, 16, h, w, dtype=torch.float64, generator=g)
    bias = 0.1 * torch.randn(16, dtype=torch.float64, generator=g)
    weight = 0.1 * torch.randn(16, 16, 3, 3, dtype=torch.float64, generator=g)
    return raw, bias, weight


def test_offset_table():
    assert [[off(p, k) for k in range(3)] for p in range(2)] == [[-1, 0, 0], [0, 0, 1]]
    assert len(phase_weights(torch.zeros(1, 1, 3, 3))) == 16          # four phases x 2 x 2 offsets


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_identity(shape):
    raw, bias, weight = _inputs(*shape)
    ref = op_sequence(raw, bias, weight)
    got = phase_form(raw, bias, weight)
    assert got.shape == ref.shape
    assert float((got - ref).abs().max()) <= 1e-13 * float(ref.abs().max())


@pytest.mark.parametrize("shape", SHAPES)
def test_weight_gradient_recombination(shape):
    """G[py][px][dy][dx] = sum over (b, Y, X) of gy[2Y+py, 2X+px] (x) a[clamp(Y+dy), clamp(X+dx)], recombined tap by tap."""
    raw, bias, weight = _inputs(*shape, seed=1)
    weight.requires_grad_(True)
    y = op_sequence(raw, bias, weight)
    gy = torch.randn(y.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    ref, = torch.autograd.grad(y, weight, gy)
    a = TF.elu(raw + bias.view(1, -1, 1, 1))
    G = {}
    for py in range(2):
        for px in range(2):
            for dy in (py - 1, py):
                for dx in (px - 1, px):
                    G[py, px, dy, dx] = torch.einsum("bohw,bchw->oc", gy[:, :, py::2, px::2], shifted(a, dy, dx))
    got = torch.zeros_like(ref)
    for ky in range(3):
        for kx in range(3):
            for py in range(2):
                for px in range(2):
                    got[:, :, ky, kx] += G[py, px, off(py, ky), off(px, kx)]
    # float64 sums of up to 2 * 24 * 80 * 4 terms in two different orders: n * eps = 1.7e-12 at the very worst
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
