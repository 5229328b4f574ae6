"""Sparse lidar supervision (csrc/sparse_depth.hip, mdx.functional / mdx.composite sparse_depth_loss): seeded case builders and an
independent float64 yardstick, shared by tests/test_sparse_depth_cpu.py and tests/test_gpu_sparse_depth.py.

The yardstick is plain torch on the CPU and imports nothing of the product: F.interpolate(..., align_corners=False) in float64,
boolean indexing of the valid pixels, autograd.  Besides the terms and their gradients it returns, per scale, the float64 sum over
the valid pixels of the per-pixel coefficient (r / sqrt(r^2 + eps^2)) * (-b / sd) / max(n, 1): a bilinear sample's tap weights add
up to 1, so the sum of a scale's whole disparity gradient must equal it -- a check of the backward's footprint that does not go
through the yardstick's own interpolation backward.

    case  B  disparity sizes             gt size    valid     covers
    A     2  (8,16) (4,8) (2,4) (1,2)    (19,37)    ~30 %     odd, non-integer ratios; both clamps; a one-row map
    B     2  the same                    (8,16)     ~30 %     identity sampling at scale 0
    C     3  (24,80) .. (3,10)           (47,155)   ~5 %      KITTI's ratio; widths that are no multiples of 4
    C1    C with gt and every disparity as views one float into their buffers (bases that are not 16-byte aligned)
    Cd    C with every pixel valid (dense)
    D     A with no valid pixel
    E     A with ONE valid pixel, in the bottom-right corner of the last image
    F     A's sizes, valid pixels only at X >= 28, among them a NaN, +inf, -1, exactly lo, exactly hi (all invalid)
Every case can be cut to its first `nscales` scales and to its first image (B = 1).
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as TF

MIN_DEPTH, MAX_DEPTH, EPS = 0.1, 100.0, 1e-3
LO, HI = float(np.float32(MIN_DEPTH)), float(np.float32(MAX_DEPTH))        # the bounds are float32 numbers
SIZES_A = [(8, 16), (4, 8), (2, 4), (1, 2)]
SIZES_C = [(24, 80), (12, 40), (6, 20), (3, 10)]
NAMES = ["A", "B", "C", "C1", "Cd", "D", "E", "F"]
F_FIRST_VALID_COLUMN = 28         # at gw = 37 no pixel at X >= 28 has a tap on column 0 of any of A's scales


def _offset_view(t):
    """The same numbers as a contiguous view one float into a larger buffer."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype)
    buf[1:] = t.reshape(-1)
    return buf[1:].view(t.shape)


@functools.lru_cache(maxsize=None)
def _full(name):
    g = torch.Generator().manual_seed(1000 + NAMES.index(name))
    B, sizes, gsize, share = {"A": (2, SIZES_A, (19, 37), 0.3), "B": (2, SIZES_A, (8, 16), 0.3), "C": (3, SIZES_C, (47, 155), 0.05),
                              "C1": (3, SIZES_C, (47, 155), 0.05), "Cd": (3, SIZES_C, (47, 155), 1.0), "D": (2, SIZES_A, (19, 37), 0.0),
                              "E": (2, SIZES_A, (19, 37), 0.0), "F": (2, SIZES_A, (19, 37), 0.5)}[name]
    disps = [0.02 + 0.9 * torch.rand(B, 1, h, w, generator=g) for h, w in sizes]
    depth = torch.exp(math.log(0.2) + math.log(60.0 / 0.2) * torch.rand(B, 1, *gsize, generator=g))    # residuals of both signs
    mask = torch.rand(B, 1, *gsize, generator=g) < share
    extra = {}
    if name == "E":
        mask[-1, 0, -1, -1] = True
    if name == "F":
        mask[..., :F_FIRST_VALID_COLUMN] = False
    gt = torch.where(mask, depth, torch.zeros_like(depth))
    if name == "F":
        spots = torch.nonzero(mask[0, 0])[:5]
        assert len(spots) == 5
        for (y, x), v in zip(spots.tolist(), (float("nan"), float("inf"), -1.0, LO, HI)):
            gt[0, 0, y, x] = v
        extra["n"] = int(mask.sum()) - 5
    if name == "C1":
        disps, gt = [_offset_view(d) for d in disps], _offset_view(gt)
        assert gt.is_contiguous() and gt.data_ptr() % 16 != 0
    return disps, gt, extra


def build(name, nscales=4, one_image=False):
    """-> (disparities [float32 CPU], gt float32 CPU, extra)"""
    disps, gt, extra = _full(name)
    disps = disps[:nscales]
    if one_image:
        keep = slice(-1, None) if name == "E" else slice(0, 1)          # E's pixel lies in the last image
        disps, gt = [d[keep] for d in disps], gt[keep]
        if name == "F":
            extra = dict(extra, n=int(((gt > LO) & (gt < HI)).sum()))
    disps, gt = [d.clone() for d in disps], gt.clone()
    if name == "C1":                  # a clone (and the B = 1 slice) is a fresh, aligned allocation: put the offset back
        disps, gt = [_offset_view(d) for d in disps], _offset_view(gt)
        assert all(t.is_contiguous() and t.data_ptr() % 16 == 4 for t in disps + [gt])
    return disps, gt, dict(extra)


def yardstick(disps, gt, weights=None, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, lo=LO, hi=HI, eps=EPS):
    """float64 -> dict(loss [nscales], n, grads: d(sum_k weights[k] * L_k) / d disp_k, coef: the per-scale coefficient sums times
    weights[k])."""
    gt = gt.detach().cpu()
    valid = (gt.float() > torch.tensor(lo, dtype=torch.float32)) & (gt.float() < torch.tensor(hi, dtype=torch.float32))
    n = int(valid.sum())
    g64 = gt.double()[valid]
    a, b = 1.0 / max_depth, 1.0 / min_depth - 1.0 / max_depth
    weights = [1.0] * len(disps) if weights is None else [float(v) for v in weights]
    losses, grads, coefs = [], [], []
    for d, wk in zip(disps, weights):
        x = d.detach().cpu().double().requires_grad_(True)
        u = x if tuple(x.shape[2:]) == tuple(gt.shape[2:]) else TF.interpolate(x, size=tuple(gt.shape[2:]), mode="bilinear",
                                                                               align_corners=False)
        sd = (a + b * u)[valid]
        r = -torch.log(sd) - torch.log(g64)
        root = torch.sqrt(r * r + eps * eps)
        L = (root - eps).sum() / max(n, 1)
        (wk * L).backward()
        losses.append(float(L.detach()))
        grads.append(x.grad.clone())
        coefs.append(float((r / root * (-b / sd)).sum().detach()) * wk / max(n, 1))
    return dict(loss=np.array(losses), n=n, grads=grads, coef=np.array(coefs))


@functools.lru_cache(maxsize=None)
def reference(name, nscales=4, one_image=False):
    """build() and its yardstick with the weights WEIGHTS[:nscales], computed once per session; read-only."""
    disps, gt, extra = build(name, nscales, one_image)
    return disps, gt, extra, yardstick(disps, gt, WEIGHTS[:nscales])


WEIGHTS = [1.0, -0.5, 2.0, 0.25]             # an upstream gradient that is neither 1 nor of one sign
VARIANTS = [(n, False) for n in (1, 2, 3, 4)] + [(4, True)]
VARIANT_IDS = ["%dscales" % n for n in (1, 2, 3, 4)] + ["B1"]
