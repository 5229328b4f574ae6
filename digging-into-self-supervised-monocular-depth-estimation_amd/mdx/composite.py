"""The hot-path ops as plain PyTorch op sequences, for CPU tensors only.

The reference picks its device at start-up (`'cuda' if torch.cuda.is_available() else 'cpu'`, model_train.py:28) and BASELINE
configs[0] is its CPU-runnable case.  model_layer / model_loss hand CPU tensors to the functions below -- this package's own
restatement of the reference's op sequences (warp.py:12-39,193-269; model_loss.py:11-116), checked against the reference-made
goldens by tests/test_torch_composite.py -- so that the same scripts run on a machine without a GPU.

This is a dispatch on the TENSOR'S DEVICE, not a fallback: a CUDA/HIP tensor always goes to libmdx_hip.so and raises if the
library is missing (mdx/_lib.py); nothing here is ever reached with a GPU tensor, and nothing under oracle/ is ever imported.
"""
import warnings

import torch
import torch.nn.functional as TF

_told = False


def _notice():
    global _told
    if not _told:
        _told = True
        warnings.warn("mdx: CPU tensors -- running the plain-PyTorch composite of the hot path (the reference's own CPU path, "
                      "model_train.py:28); the gfx950 kernels are not involved", stacklevel=3)


def interpolate_bilinear(x, H, W):
    _notice()
    return TF.interpolate(x, [H, W], mode="bilinear", align_corners=False)


def disparity2depth(disp, min_depth, max_depth):
    """reference warp.py:29-39 -> (scaled_disp, depth)."""
    _notice()
    lo, hi = 1 / max_depth, 1 / min_depth
    scaled = lo + (hi - lo) * disp
    return scaled, 1 / scaled


def backproject(depth, invK):
    """reference warp.py:193-246: depth [B,1,H,W], inv_K [B,4,4] -> [B,4,H*W]."""
    _notice()
    B, _, H, W = depth.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=depth.dtype), torch.arange(W, dtype=depth.dtype), indexing="ij")
    pix = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(H * W, dtype=depth.dtype)], 0).unsqueeze(0).expand(B, 3, H * W)
    cam = depth.view(B, 1, -1) * torch.matmul(invK[:, :3, :3], pix)
    return torch.cat([cam, torch.ones(B, 1, H * W, dtype=depth.dtype)], 1)


def project(cam, K, T, H, W, eps=1e-7):
    """reference warp.py:250-269: cam [B,4,HW], K, T [B,4,4] -> grid [B,H,W,2] in [-1, 1]."""
    _notice()
    B = cam.shape[0]
    q = torch.matmul(torch.matmul(K, T)[:, :3, :], cam)
    uv = (q[:, :2] / (q[:, 2:3] + eps)).view(B, 2, H, W).permute(0, 2, 3, 1)
    grid = torch.stack([uv[..., 0] / (W - 1), uv[..., 1] / (H - 1)], -1)
    return (grid - 0.5) * 2


def grid_sample_border(img, grid):
    _notice()
    return TF.grid_sample(img, grid, padding_mode="border", align_corners=True)


def ssim(x, y):
    """reference model_loss.py:11-41."""
    _notice()
    x, y = TF.pad(x, (1, 1, 1, 1), mode="reflect"), TF.pad(y, (1, 1, 1, 1), mode="reflect")
    mu_x, mu_y = TF.avg_pool2d(x, 3, 1), TF.avg_pool2d(y, 3, 1)
    sig_x = TF.avg_pool2d(x * x, 3, 1) - mu_x * mu_x
    sig_y = TF.avg_pool2d(y * y, 3, 1) - mu_y * mu_y
    sig_xy = TF.avg_pool2d(x * y, 3, 1) - mu_x * mu_y
    n = (2 * mu_x * mu_y + 0.01 ** 2) * (2 * sig_xy + 0.03 ** 2)
    d = (mu_x ** 2 + mu_y ** 2 + 0.01 ** 2) * (sig_x + sig_y + 0.03 ** 2)
    return torch.clamp((1 - n / d) / 2, 0, 1)


def reprojection_loss(pred, target):
    """reference model_loss.py:92-103."""
    l1 = torch.abs(target - pred).mean(1, True)
    return 0.85 * ssim(pred, target).mean(1, True) + 0.15 * l1


def smooth_loss(disp, color, normalize=True):
    """reference model_loss.py:45-88 (normalize=False) / 107-116 (normalize=True)."""
    _notice()
    if normalize:
        disp = disp / (disp.mean(2, True).mean(3, True) + 1e-7)
    gx = torch.abs(disp[:, :, :, :-1] - disp[:, :, :, 1:])
    gy = torch.abs(disp[:, :, :-1, :] - disp[:, :, 1:, :])
    gx = gx * torch.exp(-torch.abs(color[:, :, :, :-1] - color[:, :, :, 1:]).mean(1, True))
    gy = gy * torch.exp(-torch.abs(color[:, :, :-1, :] - color[:, :, 1:, :]).mean(1, True))
    return gx.mean() + gy.mean()


def sparse_depth_loss(disps, gt, min_depth, max_depth, lo=None, hi=None, eps=1e-3):
    """Sparse lidar supervision (csrc/sparse_depth.hip has the definition; mdx.functional.sparse_depth_loss is the GPU form) in any
    float dtype, mask-free: per scale the Charbonnier penalty sqrt(r^2 + eps^2) - eps of r = log depth - log gt over the valid
    pixels (lo < gt < hi, strict, the bounds taken as float32 numbers as the C-ABI takes them), divided by max(n, 1).
    -> dict(loss = tensor [nscales], valid = n).  Invalid pixels are replaced before the logarithms, so neither their values nor a
    non-finite disparity that only they touch reach the result or a gradient; a scaled disparity that is not a positive finite
    number under a valid pixel makes that scale's term NaN."""
    _notice()
    disps = list(disps)
    lo = float(torch.tensor(min_depth if lo is None else lo, dtype=torch.float32))
    hi = float(torch.tensor(max_depth if hi is None else hi, dtype=torch.float32))
    a, b = 1 / max_depth, 1 / min_depth
    gh, gw = gt.shape[2:]
    valid = (gt > lo) & (gt < hi)
    n = valid.sum()
    denom = torch.clamp(n, min=1)
    losses = []
    for disp in disps:
        g = gt.to(disp.dtype)
        u = disp if tuple(disp.shape[2:]) == (gh, gw) else TF.interpolate(disp, [gh, gw], mode="bilinear", align_corners=False)
        sd = a + (b - a) * u
        usable = (sd > 0) & torch.isfinite(sd)
        r = -torch.log(torch.where(valid & usable, sd, torch.ones_like(sd))) - torch.log(torch.where(valid, g, torch.ones_like(g)))
        r = torch.where(valid & ~usable, torch.full_like(r, float("nan")), r)
        rho = torch.sqrt(r * r + eps * eps) - eps
        losses.append(torch.where(valid, rho, torch.zeros_like(rho)).sum() / denom)
    return dict(loss=torch.stack(losses), valid=n.to(disps[0].dtype))


def _sgm_path(C, dy, dx, p1, p2):
    """One path recursion of stereo_hints over a cost volume C [H,W,D] (int32): rows (dy != 0) or columns (dy == 0) in path order,
    the predecessors of a whole row / column advanced at once."""
    H, W, D = C.shape
    whole = L = C.clone()
    if dy == 0:
        C, L = C.transpose(0, 1), L.transpose(0, 1)            # views: columns as the leading axis, no column offset inside one
        dy, dx, W = dx, 0, H
    n = C.shape[0]
    far = 1 << 20
    lo, hi = max(dx, 0), W + min(dx, 0)                         # the positions of a line whose predecessor (at -dx) is inside
    for i in (range(1, n) if dy > 0 else range(n - 2, -1, -1)):
        prev = L[i - dy, lo - dx:hi - dx]
        m = prev.min(dim=1, keepdim=True).values
        side = TF.pad(prev, (1, 1), value=far)
        best = torch.minimum(torch.minimum(prev, torch.minimum(side[:, :-2], side[:, 2:]) + p1), m + p2)
        L[i, lo:hi] = C[i, lo:hi] + best - m
    return whole


def stereo_hints(target, partner, K, T, max_disp=64, p1=8, p2=64, return_volume=False):
    """Stereo proxy depth in plain torch for CPU tensors (include/mdx.h "stereo proxy depth" has the definition, items 1-10;
    mdx.functional.stereo_hints is the GPU form): census + semi-global matching over the rectified pair target / partner
    [B,3,H,W], left-right checked.  -> dict(depth, disp float32 [B,1,H,W], 0 where invalid; valid uint8 [B,1,H,W]
    [, volume = S uint16-valued int32 [B,H,W,D]]).  Integers as the definition states them, floats in its order."""
    _notice()
    if any(t.is_cuda for t in (target, partner, K, T)):
        from ._lib import MdxError
        raise MdxError("mdx.composite.stereo_hints is the CPU form: GPU tensors go to mdx.functional.stereo_hints")
    D, p1, p2 = int(max_disp), int(p1), int(p2)
    if D not in (64, 128) or not 0 < p1 < p2 <= 190 or target.dim() != 4 or target.shape[1] != 3 or partner.shape != target.shape:
        raise ValueError("stereo_hints: max_disp %r (64 or 128), p1 %r < p2 %r <= 190, images %s / %s ([B,3,H,W])"
                         % (max_disp, p1, p2, tuple(target.shape), tuple(partner.shape)))
    B, _, H, W = target.shape
    target, partner, K, T = target.float(), partner.float(), K.float(), T.float()
    ys = torch.arange(H)
    xs = torch.arange(W)

    def census(img):
        L = (0.299 * img[0] + 0.587 * img[1]) + 0.114 * img[2]
        bits = [L[(ys + dy).clamp(0, H - 1)][:, (xs + dx).clamp(0, W - 1)] < L
                for dy in range(-3, 4) for dx in range(-4, 5) if (dy, dx) != (0, 0)]
        return torch.stack(bits, -1)

    out = dict(depth=torch.zeros(B, 1, H, W), disp=torch.zeros(B, 1, H, W), valid=torch.zeros(B, 1, H, W, dtype=torch.uint8))
    volume = torch.zeros(B, H, W, D, dtype=torch.int32)
    for b in range(B):
        tx = T[b, 0, 3]
        if not bool(torch.isfinite(tx)) or float(tx) == 0:
            continue
        sgn = 1 if float(tx) > 0 else -1
        ct, cs = census(target[b]), census(partner[b])
        C = torch.full((H, W, D), 31, dtype=torch.int32)
        for d in range(min(D, W)):
            a, z = (0, W - d) if sgn > 0 else (d, W)              # the target columns whose match lies inside
            C[:, a:z, d] = (ct[:, a:z] != cs[:, a + sgn * d:z + sgn * d]).sum(-1, dtype=torch.int32)
        S = sum(_sgm_path(C, dy, dx, p1, p2) for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1)))
        volume[b] = S
        key = S.long() * 256 + torch.arange(D)                    # the smallest S, then the smallest d
        d0 = key.min(dim=2).values % 256
        # the partner's view: column xr sees S(y, xr - sgn*d, d)
        cols = xs[:, None] - sgn * torch.arange(D)[None, :]       # [W,D]
        seen = torch.where(((cols >= 0) & (cols < W))[None], key[:, cols.clamp(0, W - 1), torch.arange(D)[None, :]],
                           torch.full((), 1 << 40, dtype=torch.long))
        dR = seen.min(dim=2).values % 256
        xm = xs[None, :] + sgn * d0
        inside = (xm >= 0) & (xm < W)
        valid = (d0 >= 1) & inside & ((torch.gather(dR, 1, xm.clamp(0, W - 1)) - d0).abs() <= 1)
        Sf = S.float()
        a = torch.gather(Sf, 2, (d0 - 1).clamp(0, D - 1)[..., None])[..., 0]
        m = torch.gather(Sf, 2, d0[..., None])[..., 0]
        c = torch.gather(Sf, 2, (d0 + 1).clamp(0, D - 1)[..., None])[..., 0]
        den = (a + c) - 2 * m
        fit = (d0 > 0) & (d0 < D - 1) & (den > 0)
        dsub = torch.where(fit, d0.float() + (a - c) / (2 * torch.where(fit, den, torch.ones_like(den))), d0.float())
        num = K[b, 0, 0] * tx.abs()
        out["disp"][b, 0] = torch.where(valid, dsub, torch.zeros_like(dsub))
        out["depth"][b, 0] = torch.where(valid, num / torch.where(valid, dsub, torch.ones_like(dsub)), torch.zeros_like(dsub))
        out["valid"][b, 0] = valid.to(torch.uint8)
    if return_volume:
        out["volume"] = volume
    return out


def hint_select(target, partner, K, invK, T, hint, disp, min_depth, max_depth, return_losses=False):
    """Depth-hint selection in plain torch for CPU tensors (include/mdx.h "depth-hint selection" has the definition;
    mdx.functional.hint_select is the GPU form), from the ops above: the hint ([B,1,H,W], 0 = none) is kept only where the partner
    warped with it gives a strictly lower reprojection loss against `target` than the partner warped with the depth of `disp`
    ([B,1,h,w]).  -> dict(sel float32 [B,1,H,W], counts int32 [B,2] = (hints, kept)[, l_hint, l_pred])."""
    _notice()
    tensors = (target, partner, K, invK, T, hint, disp)
    if any(t.is_cuda for t in tensors):
        from ._lib import MdxError
        raise MdxError("mdx.composite.hint_select is the CPU form: GPU tensors go to mdx.functional.hint_select")
    with torch.no_grad():
        target, partner, K, invK, T, hint, disp = (t.detach().float() for t in tensors)
        B, _, H, W = target.shape
        if tuple(hint.shape) != (B, 1, H, W) or disp.dim() != 4 or disp.shape[2] > H or disp.shape[3] > W:
            raise ValueError("hint_select: hint %s and disp %s against images of %s" % (tuple(hint.shape), tuple(disp.shape), tuple(target.shape)))
        up = disp if tuple(disp.shape[2:]) == (H, W) else interpolate_bilinear(disp, H, W)
        losses = [reprojection_loss(grid_sample_border(partner, project(backproject(d, invK), K, T, H, W)), target)
                  for d in (hint, disparity2depth(up, min_depth, max_depth)[1])]
        has = hint > 0
        keep = has & (losses[0] < losses[1])
        out = dict(sel=torch.where(keep, hint, torch.zeros_like(hint)),
                   counts=torch.stack([has.sum((1, 2, 3)), keep.sum((1, 2, 3))], 1).to(torch.int32))
        if return_losses:
            out["l_hint"], out["l_pred"] = losses
    return out
