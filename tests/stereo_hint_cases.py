"""Stereo proxy depth (csrc/stereo_hints.hip, mdx.functional / mdx.composite stereo_hints): seeded case builders and an independent
numpy restatement of the definition in include/mdx.h ("stereo proxy depth"), shared by tests/test_stereo_hints_cpu.py and
tests/test_gpu_stereo_hints.py.  Nothing of mdx/ or csrc/ is imported here.

The restatement follows the header item by item: direction from T[b,0,3]; float32 luma, each operation rounded on its own; a 9 x 7
census of 62 clamped neighbours; Hamming cost, 31 where the match leaves the image; eight path recursions written as loops over the
positions of a path with every path of a direction advanced together; S as their sum; d0 and the partner's dR as first minima;
the left-right check; the float32 parabola; depth = (K00 * |T03|) / dsub.

    restate(target, partner, K, T, D, P1, P2) -> dict(S uint16 [B,H,W,D], d0, dR int32 [B,H,W], valid uint8 [B,1,H,W],
                                                      disp, depth float32 [B,1,H,W])
"""
import functools

import numpy as np

P1, P2 = 8, 64
BORDER_COST = 31
PATHS = [(0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1)]          # (row, column) steps


def luma(img):
    """img float32 [3,H,W] -> (0.299 R + 0.587 G) + 0.114 B, float32 at every step."""
    img = np.asarray(img, dtype=np.float32)
    r, g, b = img[0], img[1], img[2]
    return ((np.float32(0.299) * r + np.float32(0.587) * g).astype(np.float32) + np.float32(0.114) * b).astype(np.float32)


def census(L):
    """62 bits: L(neighbour) < L(centre) over the 9 wide x 7 high window, coordinates clamped to the image."""
    H, W = L.shape
    ys, xs = np.arange(H), np.arange(W)
    word = np.zeros((H, W), dtype=np.uint64)
    for dy in range(-3, 4):
        for dx in range(-4, 5):
            if dy == 0 and dx == 0:
                continue
            nb = L[np.clip(ys + dy, 0, H - 1)][:, np.clip(xs + dx, 0, W - 1)]
            word = (word << np.uint64(1)) | (nb < L).astype(np.uint64)
    return word


def _popcount(v):
    v = v.copy()
    n = np.zeros(v.shape, dtype=np.int32)
    for _ in range(64):
        n += (v & np.uint64(1)).astype(np.int32)
        v >>= np.uint64(1)
    return n


def cost_volume(ct, cs, direction, D):
    H, W = ct.shape
    C = np.full((H, W, D), BORDER_COST, dtype=np.int32)
    x = np.arange(W)
    for d in range(D):
        xs = x + direction * d
        ok = (xs >= 0) & (xs < W)
        if ok.any():
            C[:, ok, d] = _popcount(ct[:, ok] ^ cs[:, xs[ok]])
    return C


def _advance(prev, C, p1, p2):
    """One step of the recursion for a set of pixels: prev, C [n,D] -> L [n,D]."""
    big = np.int32(1 << 20)
    m = prev.min(axis=1, keepdims=True)
    down = np.full_like(prev, big)
    down[:, 1:] = prev[:, :-1] + p1                    # L(p-r, d-1) + P1, absent at d = 0
    up = np.full_like(prev, big)
    up[:, :-1] = prev[:, 1:] + p1                      # L(p-r, d+1) + P1, absent at d = D-1
    return C + np.minimum(np.minimum(prev, down), np.minimum(up, m + p2)) - m


def path(C, r, p1, p2):
    """L_r over the whole image for the step r = (dy, dx)."""
    H, W, D = C.shape
    dy, dx = r
    L = np.empty_like(C)
    if dy == 0:
        order = range(W) if dx > 0 else range(W - 1, -1, -1)
        for n, x in enumerate(order):
            L[:, x] = C[:, x] if n == 0 else _advance(L[:, x - dx], C[:, x], p1, p2)
        return L
    order = range(H) if dy > 0 else range(H - 1, -1, -1)
    x = np.arange(W)
    for n, y in enumerate(order):
        if n == 0:
            L[y] = C[y]
            continue
        px = x - dx
        inside = (px >= 0) & (px < W)
        L[y] = C[y]
        L[y, inside] = _advance(L[y - dy, px[inside]], C[y, inside], p1, p2)
    return L


def restate_one(target, partner, fx, tx, D, p1=P1, p2=P2):
    """One sample: target, partner float32 [3,H,W]; fx = K[0,0], tx = T[0,3]."""
    _, H, W = target.shape
    tx = np.float32(tx)
    zero = dict(S=np.zeros((H, W, D), np.uint16), d0=np.zeros((H, W), np.int32), dR=np.zeros((H, W), np.int32),
                valid=np.zeros((H, W), np.uint8), disp=np.zeros((H, W), np.float32), depth=np.zeros((H, W), np.float32))
    if not np.isfinite(tx) or tx == 0:
        return zero
    direction = 1 if tx > 0 else -1
    C = cost_volume(census(luma(target)), census(luma(partner)), direction, D)
    S = np.zeros((H, W, D), dtype=np.int32)
    for r in PATHS:
        Lr = path(C, r, p1, p2)
        assert Lr.max() <= 62 + p2 and Lr.min() >= 0
        S += Lr
    assert S.max() < 65536
    d0 = S.argmin(axis=2).astype(np.int32)                                   # numpy: the first minimum
    x = np.arange(W)
    dR = np.zeros((H, W), dtype=np.int32)
    for xr in range(W):
        best = np.full(H, 1 << 30, dtype=np.int64)
        for d in range(D):
            col = xr - direction * d
            if 0 <= col < W:
                v = S[:, col, d]
                better = v < best                                            # strict: the smallest d on ties
                dR[better, xr] = d
                best = np.where(better, v, best)
    xm = x[None, :] + direction * d0
    inside = (xm >= 0) & (xm < W)
    dRm = np.take_along_axis(dR, np.clip(xm, 0, W - 1), axis=1)
    valid = (d0 >= 1) & inside & (np.abs(dRm - d0) <= 1)
    f32 = np.float32
    ix = np.arange(H)[:, None], x[None, :]
    a = S[ix[0], ix[1], np.clip(d0 - 1, 0, D - 1)].astype(f32)
    m = S[ix[0], ix[1], d0].astype(f32)
    c = S[ix[0], ix[1], np.clip(d0 + 1, 0, D - 1)].astype(f32)
    den = ((a + c).astype(f32) - (f32(2) * m).astype(f32)).astype(f32)
    fit = (d0 > 0) & (d0 < D - 1) & (den > 0)
    safe = np.where(fit, den, f32(1))
    off = ((a - c).astype(f32) / (f32(2) * safe).astype(f32)).astype(f32)
    dsub = np.where(fit, (d0.astype(f32) + off).astype(f32), d0.astype(f32)).astype(f32)
    num = (f32(fx) * np.abs(tx)).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        depth = np.where(valid, (num / np.where(valid, dsub, f32(1))).astype(f32), f32(0)).astype(f32)
    disp = np.where(valid, dsub, f32(0)).astype(f32)
    return dict(S=S.astype(np.uint16), d0=d0, dR=dR, valid=valid.astype(np.uint8), disp=disp, depth=depth)


def restate(target, partner, K, T, D=64, p1=P1, p2=P2):
    """Batched: target, partner [B,3,H,W]; K, T [B,4,4] (numpy or anything np.asarray takes)."""
    target, partner = np.asarray(target, dtype=np.float32), np.asarray(partner, dtype=np.float32)
    K, T = np.asarray(K, dtype=np.float32), np.asarray(T, dtype=np.float32)
    outs = [restate_one(target[b], partner[b], K[b, 0, 0], T[b, 0, 3], D, p1, p2) for b in range(target.shape[0])]
    res = {k: np.stack([o[k] for o in outs]) for k in outs[0]}
    for k in ("valid", "disp", "depth"):
        res[k] = res[k][:, None]
    return res


# ---- case builders ----------------------------------------------------------------------------------------------------------
def make_KT(signs, W, fx_share=0.58, baseline=0.1):
    """K, T float32 [B,4,4]: fx = fx_share * W, T[b,0,3] = signs[b] * baseline (a sign of 0 gives the dead sample)."""
    B = len(signs)
    K = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = fx_share * W, 1.92 * 16, 0.5 * W, 8.0
    T = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    T[:, 0, 3] = np.asarray(signs, dtype=np.float32) * np.float32(baseline)
    return K, T


def _smooth(rng, H, W, passes=2):
    img = rng.random((3, H + 8, W + 8)).astype(np.float32)
    for _ in range(passes):
        img = (img[:, :-1, :-1] + img[:, 1:, :-1] + img[:, :-1, 1:] + img[:, 1:, 1:]) * np.float32(0.25)
    return np.ascontiguousarray(img[:, :H, :W])


def shifted_pair(seed, H, W, signs, disparity=None, noise=0.02, scale=1):
    """Textured targets and partners that show them moved by a per-row-band disparity (larger towards the bottom, as a road is) in
    the direction of each sample's sign, plus noise: not exact anywhere, so the matcher has ties, occlusions and edges to settle."""
    rng = np.random.default_rng(seed)
    B = len(signs)
    t = np.stack([_smooth(rng, H, W) for _ in range(B)])
    p = np.empty_like(t)
    for b, s in enumerate(signs):
        direction = 1 if s >= 0 else -1
        for y in range(H):
            k = scale * (1 + (y * 7) // max(H, 1)) if disparity is None else disparity
            p[b, :, y] = np.roll(t[b, :, y], direction * k, axis=1)
    p = (p + noise * rng.standard_normal(p.shape).astype(np.float32)).astype(np.float32)
    return t, np.ascontiguousarray(p)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (target, partner, K, T, D), read-only.
        n13x37, n37x13  D 64   narrower than D / paths leave through a side edge
        n24x80          D 64
        n20x150         D 128  two disparities per lane
        const           D 64   a constant image: every cost ties
        quant           D 64   colours quantised to five levels
        dead            D 64   a T[0,3] = 0 sample beside a live one
        b3              D 64   three samples, signs + - +"""
    shapes = {"n13x37": (13, 37, 64), "n37x13": (37, 13, 64), "n24x80": (24, 80, 64), "n20x150": (20, 150, 128)}
    if name in shapes:
        H, W, D = shapes[name]
        t, p = shifted_pair(10 + sorted(shapes).index(name), H, W, (1, -1), scale=10 if D == 128 else 1)     # D = 128: winners up to 70
        K, T = make_KT((1, -1), W)
    elif name == "const":
        H, W, D = 16, 40, 64
        t = np.full((2, 3, H, W), 0.5, dtype=np.float32)
        p = t.copy()
        K, T = make_KT((1, -1), W)
    elif name == "quant":
        H, W, D = 18, 70, 64
        rng = np.random.default_rng(20)
        blocks = rng.integers(0, 5, (2, 3, 6, 10)).astype(np.float32) / np.float32(4)           # five levels in flat 3 x 7 blocks
        t = np.ascontiguousarray(np.repeat(np.repeat(blocks, 3, axis=2), 7, axis=3))
        p = np.stack([np.roll(t[0], 3, axis=2), np.roll(t[1], -3, axis=2)])
        K, T = make_KT((1, -1), W)
    elif name == "dead":
        H, W, D = 16, 48, 64
        t, p = shifted_pair(21, H, W, (1, 1))
        K, T = make_KT((0, -1), W)
        p[1] = shifted_pair(21, H, W, (1, -1))[1][1]
    elif name == "b3":
        H, W, D = 14, 45, 64
        t, p = shifted_pair(22, H, W, (1, -1, 1))
        K, T = make_KT((1, -1, 1), W)
    else:
        raise KeyError(name)
    for a in (t, p, K, T):
        a.setflags(write=False)
    return t, p, K, T, D


@functools.lru_cache(maxsize=None)
def reference(name):
    """case(name) and its restatement, computed once per session; read-only."""
    t, p, K, T, D = case(name)
    return restate(t, p, K, T, D)


SHAPE_CASES = ["n13x37", "n37x13", "n24x80", "n20x150", "const", "quant", "dead"]
