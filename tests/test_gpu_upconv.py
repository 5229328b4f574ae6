"""GPU tests (MI355X) of the decoder's last stage convolution on the low-resolution map (csrc/upconv_nhwc.hip,
mdx.functional.up_conv3x3) against the float64 op sequence on the CPU:
conv2d(pad(interpolate(elu(raw + bias), 2, "nearest"), 1, "reflect"), weight) and its autograd.grad for a random gy.
y, graw, gweight within 2e-6 x max|reference| (the bound test_thin_conv3x3_weight_gradient_matches_float64 holds MIOpen and the
thin weight gradient to), gbias within 1e-5 x (the disparity head's bias-gradient bound)."""
import functools
import importlib

import pytest
import torch
import torch.nn.functional as TF

importlib.import_module("digging-into-self-supervised-monocular-depth-estimation_amd")

pytestmark = pytest.mark.gpu

# low-resolution (B, h, w): a single row (both clamps on it), two rows, widths that are no multiple of the 16-pixel strip,
# more than one strip and row run
SHAPES = [(1, 1, 4), (2, 2, 4), (1, 3, 8), (2, 5, 12), (3, 7, 20), (1, 33, 36), (2, 24, 80)]


@pytest.fixture(scope="module")
def F():
    from mdx import functional
    return functional


@functools.lru_cache(maxsize=None)
def reference(shape):
    """Inputs and the float64 results of the op sequence on the CPU, computed once per shape."""
    B, h, w = shape
    g = torch.Generator().manual_seed(1000 * B + 10 * h + w)
    raw = torch.randn(B, 16, h, w, generator=g)
    bias = 0.1 * torch.randn(16, generator=g)
    weight = 0.1 * torch.randn(16, 16, 3, 3, generator=g)
    gy = torch.randn(B, 16, 2 * h, 2 * w, generator=g)
    r, b, wt = (t.double().requires_grad_(True) for t in (raw, bias, weight))
    a = TF.elu(r + b.view(1, -1, 1, 1))
    y = TF.conv2d(TF.pad(TF.interpolate(a, scale_factor=2, mode="nearest"), (1, 1, 1, 1), mode="reflect"), wt)
    graw, gbias, gweight = torch.autograd.grad(y, (r, b, wt), gy.double())
    return (raw, bias, weight, gy), (y.detach(), graw, gbias, gweight)


def _gpu_inputs(shape, weight_cl):
    (raw, bias, weight, gy), _ = reference(shape)
    raw = raw.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    weight = weight.cuda()
    if weight_cl:
        weight = weight.contiguous(memory_format=torch.channels_last)
    return raw, bias.cuda().requires_grad_(True), weight.requires_grad_(True), gy.cuda().contiguous(memory_format=torch.channels_last)


def _close(name, got, want, rel):
    err, scale = float((got.detach().double().cpu() - want).abs().max()), float(want.abs().max())
    print("%s: max error %.3g = %.3g x max|reference|" % (name, err, err / scale))
    assert err <= rel * scale, (name, err, scale)


@pytest.mark.parametrize("weight_cl", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_up_conv3x3_matches_float64(F, shape, weight_cl):
    raw, bias, weight, gy = _gpu_inputs(shape, weight_cl)
    _, (y_ref, graw_ref, gbias_ref, gweight_ref) = reference(shape)
    assert F.up_conv_ok(raw, weight)
    y = F.up_conv3x3(raw, bias, weight)
    B, h, w = shape
    assert y.shape == (B, 16, 2 * h, 2 * w) and y.is_contiguous(memory_format=torch.channels_last)
    graw, gbias, gweight = torch.autograd.grad(y, (raw, bias, weight), gy)
    assert gweight.shape == weight.shape and gweight.stride() == weight.stride()
    assert graw.shape == raw.shape and graw.stride() == raw.stride() and gbias.shape == bias.shape
    _close("y", y, y_ref, 2e-6)
    _close("graw", graw, graw_ref, 2e-6)
    _close("gweight", gweight, gweight_ref, 2e-6)
    _close("gbias", gbias, gbias_ref, 1e-5)


@pytest.mark.parametrize("shape", [(2, 5, 12), (2, 24, 80)])
def test_same_bits_at_every_call_and_from_any_workspace(F, shape):
    """Two calls give the same bits; the backward's workspace may hold anything on entry (0xff bytes: NaNs) -- every partial it reads
    it has written."""
    from mdx._lib import api, ptr, stream
    raw, bias, weight, gy = _gpu_inputs(shape, False)
    raw, bias, weight = raw.detach(), bias.detach(), weight.detach()
    B, h, w = shape
    assert torch.equal(F.up_conv3x3(raw, bias, weight), F.up_conv3x3(raw, bias, weight))
    nws = api.mdx_up_conv3x3_workspace_bytes(B, h, w)
    assert nws > 0
    results = []
    for fill in (0x00, 0xff, 0xff):
        ws = torch.full((nws,), fill, dtype=torch.uint8, device="cuda")
        graw, gbias, gw = torch.full_like(raw, 7.0), torch.full_like(bias, 7.0), torch.full_like(weight, 7.0)
        so, sc, sy, sx = weight.stride()
        api.mdx_up_conv3x3_bwd(ptr(gy, cl=True), ptr(raw, cl=True), ptr(bias), ptr(weight, cl="any"), so, sc, sy, sx, ptr(graw, cl=True),
                               ptr(gbias), ptr(gw, cl="any"), so, sc, sy, sx, B, h, w, ptr(ws, torch.uint8), nws, stream())
        results.append((graw, gbias, gw))
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    # and the autograd function gives these bits too
    r, b, wt = raw.clone().requires_grad_(True), bias.clone().requires_grad_(True), weight.clone().requires_grad_(True)
    for a, g in zip(results[0], torch.autograd.grad(F.up_conv3x3(r, b, wt), (r, b, wt), gy)):
        assert torch.equal(a, g)


def test_captured_graph_replays_on_new_values(F):
    shape = (2, 5, 12)
    raw, bias, weight, gy = _gpu_inputs(shape, True)
    static_raw = raw.detach().clone().requires_grad_(True)

    def step():
        y = F.up_conv3x3(static_raw, bias, weight)
        return (y,) + torch.autograd.grad(y, (static_raw, bias, weight), gy)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                              # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    new_raw = torch.randn(raw.shape, generator=torch.Generator().manual_seed(5)).cuda().contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        static_raw.copy_(new_raw)
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in captured]
    eager_raw = new_raw.clone().requires_grad_(True)
    y = F.up_conv3x3(eager_raw, bias, weight)
    want = (y,) + torch.autograd.grad(y, (eager_raw, bias, weight), gy)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_refusals(F):
    from mdx._lib import MdxError
    cl = torch.channels_last
    weight, bias = torch.randn(16, 16, 3, 3, device="cuda"), torch.zeros(16, device="cuda")
    good = torch.randn(1, 16, 3, 8, device="cuda").contiguous(memory_format=cl)
    assert F.up_conv_ok(good, weight)
    bad = [(torch.randn(1, 16, 3, 6, device="cuda").contiguous(memory_format=cl), weight),            # w % 4 != 0
           (torch.randn(1, 32, 3, 8, device="cuda").contiguous(memory_format=cl), weight),            # other channel counts
           (good, torch.randn(16, 32, 3, 3, device="cuda")),
           (good, torch.randn(32, 16, 3, 3, device="cuda")),
           (good.bfloat16(), weight),                                                                 # bf16
           (good, weight.bfloat16()),
           (good.contiguous(), weight)]                                                               # a planar map
    for raw, wt in bad:
        assert not F.up_conv_ok(raw, wt)
        with pytest.raises(MdxError):
            F.up_conv3x3(raw, bias, wt)


def test_decoder_with_and_without_the_fused_stage(monkeypatch):
    """DepthDecoder (channels-last, float32) with fused_upconv True against False: the bounds of
    test_decoder_glue_path_equals_module_path."""
    from mdx import functional
    from model_layer import ResnetEncoder, DepthDecoder
    monkeypatch.delenv("MDX_FUSED_UPCONV", raising=False)
    torch.manual_seed(3)
    enc = ResnetEncoder(18, False).cuda().to(memory_format=torch.channels_last)
    dec = DepthDecoder(enc.num_ch_enc).cuda().to(memory_format=torch.channels_last)
    img = torch.rand(2, 3, 64, 96, device="cuda")
    base = [f.detach() for f in enc(img)]
    seen, real, runs = [], functional.up_conv3x3, {}
    monkeypatch.setattr(functional, "up_conv3x3", lambda *a: (seen.append(1), real(*a))[1])
    for fused in (True, False):
        monkeypatch.setattr(DepthDecoder, "fused_upconv", fused)
        dec.zero_grad()
        feats = [f.clone().requires_grad_(True) for f in base]
        out = dec(feats)
        sum(v.float().mean() for v in out.values()).backward()
        runs[fused] = ({k: v.detach() for k, v in out.items()}, {n: p.grad.clone() for n, p in dec.named_parameters()},
                       [f.grad.clone() for f in feats])
        assert len(seen) == 1                               # taken when the switch is on, and only then
    (out1, grads1, fg1), (out0, grads0, fg0) = runs[True], runs[False]
    for k in out0:
        torch.testing.assert_close(out1[k], out0[k], rtol=2e-5, atol=2e-5)
    for n in grads0:
        scale = float(grads0[n].abs().max()) + 1e-12
        assert float((grads1[n] - grads0[n]).abs().max()) <= 5e-4 * scale, n
    for a, b in zip(fg1, fg0):
        assert float((a - b).abs().max()) <= 5e-4 * (float(b.abs().max()) + 1e-12)
