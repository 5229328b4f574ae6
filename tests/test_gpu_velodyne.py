"""GPU: mdx.imgproc.velodyne_depth (csrc/velodyne.hip) against the host path it stands for -- model_utility.point2depth ->
resize_nearest -> np.fliplr -> float32 on calibration files written to tmp_path -- BIT FOR BIT on the whole map.

Bit equality across two float64 evaluation orders (numpy's matrix product, the kernel's left-to-right sums) needs inputs away from
rounding boundaries; every test first asserts that on the host, in float64 (`precondition`): every projected u, v at least 1e-9
from a half-integer, every depth at least 1e-12 (relative) from a float32 rounding midpoint.  That is a condition on the inputs,
not a tolerance on the kernel.  Crafted points aim at pixel centres + 0.2."""
import importlib
import os
import random

import numpy as np
import pytest
import torch

import fake_kitti
import goldens_r2

PKG = "digging-into-self-supervised-monocular-depth-estimation_amd"
importlib.import_module(PKG)
import model_utility as mu  # noqa: E402

pytestmark = pytest.mark.gpu

# a camera whose image is a handful of pixels: focal length 6, x forward -> camera Z (T_z = -0.25: exact in binary, so a point
# with x = 0.25 has Z exactly 0), camera 3 shifted sideways
SMALL_V2C = "R: 0 -1 0 0 0 -1 1 0 0\nT: 0 -0.0625 -0.25\n"


def small_c2c(h, w, f=6.0):
    return ("S_rect_02: %d %d\nR_rect_00: 1 0 0 0 1 0 0 0 1\n"
            "P_rect_02: %r 0 %r 0.375 0 %r %r 0.0625 0 0 1 0\nP_rect_03: %r 0 %r -2.5 0 %r %r 0.125 0 0 1 0\n"
            % (w, h, f, w / 2.0, f, h / 2.0, f, w / 2.0, f, h / 2.0))


def write_calib(path, c2c, v2c):
    os.makedirs(str(path), exist_ok=True)
    open(os.path.join(str(path), "calib_cam_to_cam.txt"), "w").write(c2c)
    open(os.path.join(str(path), "calib_velo_to_cam.txt"), "w").write(v2c)
    return str(path)


def aim(P, x, r, c, off=0.2):
    """the float32 point with forward coordinate x that projects to (u, v) = (c + 1 + off, r + 1 + off): pixel (r, c)"""
    u, v = c + 1 + off, r + 1 + off
    A = np.array([P[0] - u * P[2], P[1] - v * P[2]])           # A . (x, y, z, 1) = 0
    y, z = np.linalg.solve(A[:, 1:3], -(A[:, 0] * np.float64(np.float32(x)) + A[:, 3]))
    return [np.float32(x), np.float32(y), np.float32(z)]


def precondition(P, pts, vel_depth):
    """on the host, in float64: the kept points' u, v and depths are away from the rounding boundaries (module docstring)"""
    pts = np.asarray(pts, np.float32).reshape(-1, pts.shape[-1])[:, :3]
    pts = pts[pts[:, 0] >= 0].astype(np.float64)
    if not len(pts):
        return
    with np.errstate(all="ignore"):
        q = (P @ np.hstack([pts, np.ones((len(pts), 1))]).T).T
        uv = q[:, :2] / q[:, 2:3]
    fin = np.isfinite(uv).all(1)
    uv = uv[fin]
    dist = np.abs(np.abs(uv - np.floor(uv) - 0.5))
    assert dist.size == 0 or dist.min() >= 1e-9, "a projected coordinate sits on a rounding boundary: %g" % dist.min()
    d = (pts[:, 0] if vel_depth else q[:, 2])[fin]
    d = d[(d != 0) & (np.abs(d) < 1e38)]
    f = d.astype(np.float32)
    for side in (np.float32(np.inf), np.float32(-np.inf)):
        mid = (f.astype(np.float64) + np.nextafter(f, side).astype(np.float64)) / 2
        rel = np.abs(d - mid) / np.abs(d)
        assert rel.size == 0 or rel.min() >= 1e-12, "a depth sits on a float32 rounding midpoint: %g" % rel.min()


def host_map(calib, pts, tmp_path, cam, vel_depth, gt, flip):
    """the yardstick: point2depth + resize_nearest + fliplr -> float32"""
    pts = np.asarray(pts, np.float32)
    full = np.ones((len(pts), 4), np.float32)
    full[:, :3] = pts[:, :3]
    f = os.path.join(str(tmp_path), "scan_%d.bin" % random.getrandbits(48))
    full.tofile(f)
    with np.errstate(all="ignore"):
        d = mu.resize_nearest(mu.point2depth(calib, f, cam, vel_depth), gt)
    return np.ascontiguousarray(np.fliplr(d) if flip else d, dtype=np.float32)


def device_maps(scans, gt, vel_depth, cols=3, pad=0, fill=np.nan):
    """scans: [(points [n, >= 3], P, (h, w), flip)] -> float32 [B, gh, gw] through velodyne_depth; rows past a scan's own are
    filled with `fill`"""
    from mdx.imgproc import velodyne_depth
    nmax = max([len(s[0]) for s in scans] + [0]) + pad
    block = np.full((len(scans), nmax, cols), fill, np.float32)
    for b, s in enumerate(scans):
        if len(s[0]):
            block[b, :len(s[0]), :3] = np.asarray(s[0], np.float32)[:, :3]
    out = velodyne_depth(torch.from_numpy(block).cuda(), [len(s[0]) for s in scans], np.stack([s[1] for s in scans]),
                         [s[2] for s in scans], gt, [s[3] for s in scans], vel_depth)
    assert out.dtype == torch.float32 and tuple(out.shape) == (len(scans), 1) + tuple(gt)
    return out.cpu().numpy()[:, 0]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def check(tmp_path, calib, pts, cam=2, gt=None, flip=False, cols=3, both=(False, True)):
    """one scan through both paths, for vel_depth off and on; -> the device maps"""
    P, hw = mu.velodyne_projection(calib, cam)
    hw = tuple(int(v) for v in hw[:2])
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    got = {}
    for vd in both:
        precondition(P, pts, vd)
        want = host_map(calib, pts, tmp_path, cam, vd, gt or hw, flip)
        got[vd] = device_maps([(pts, P, hw, flip)], gt or hw, vd, cols)[0]
        assert same_bits(got[vd], want), "vel_depth %s: %d pixels differ" % (vd, (got[vd] != want).sum())
    return got


# ---- the reference itself ---------------------------------------------------------------------------------------------------

def test_reference_fixture_both_cameras(tmp_path):
    """the scan and calibrations recorded with the reference's own results (tests/golden/r2_metrics.npz: 6015 points, 375x1242,
    triple hits on one pixel and the (row, 0) / (row - 1, last) collision)"""
    z = goldens_r2.load("r2_metrics")
    calib = write_calib(tmp_path / "day", str(z["calib_cam_to_cam"]), str(z["calib_velo_to_cam"]))
    pts = z["velo_points"].astype(np.float32)[:, :3]
    for cam in (2, 3):
        got = check(tmp_path, calib, pts, cam)
        for vd in (False, True):
            assert got[vd].shape == tuple(z["p2d_shape"])
            flat = got[vd].reshape(-1)
            nz = np.flatnonzero(flat)
            assert np.array_equal(nz, z["p2d_idx_c%d_v%d" % (cam, vd)]), "pixels hit (cam %d, vel_depth %s)" % (cam, vd)
            assert same_bits(flat[nz], z["p2d_val_c%d_v%d" % (cam, vd)].astype(np.float32)), "depth values"


# ---- the smallest grids where the rules can go wrong ---------------------------------------------------------------------------

H, W = 8, 13          # odd width: the w - 1 collisions are live


@pytest.fixture()
def small(tmp_path):
    calib = write_calib(tmp_path / "small", small_c2c(H, W), SMALL_V2C)
    return calib, mu.velodyne_projection(calib, 2)[0]


def random_scan(P, n, seed, h=H, w=W):
    """n points: most aimed at random pixels of the image and a rim around it (duplicates and g collisions happen by themselves:
    the image has 104 pixels), some behind the car"""
    rng = np.random.RandomState(seed)
    pts = []
    for i in range(n):
        x = 2.0 + 0.37 * i + rng.uniform(0, 0.3)
        p = aim(P, x, rng.randint(-2, h + 2), rng.randint(-2, w + 2))
        if rng.rand() < 0.15:
            p[0] = np.float32(-p[0])
        pts.append(p)
    return np.array(pts, np.float32).reshape(-1, 3)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 200])
def test_small_grid_scan_lengths(tmp_path, small, n):
    calib, P = small
    pts = random_scan(P, n, seed=n)
    got = check(tmp_path, calib, pts)
    if n >= 63:
        assert (got[True] > 0).sum() > 10 and (pts[:, 0] < 0).any()
    else:
        assert n == 1 or not got[True].any()
    check(tmp_path, calib, pts, cam=3)


def test_three_points_on_one_pixel_nearest_first_middle_last(tmp_path, small):
    calib, P = small
    pts = []
    for (r, c), depths in (((1, 3), (5.0, 9.0, 7.0)), ((3, 6), (9.0, 5.0, 7.0)), ((6, 9), (9.0, 7.0, 5.0))):
        pts += [aim(P, d, r, c) for d in depths]
    got = check(tmp_path, calib, pts)
    for r, c in ((1, 3), (3, 6), (6, 9)):
        assert got[True][r, c] == 5.0            # the nearest, wherever it stands in the file
    assert (got[True] > 0).sum() == 3


@pytest.mark.parametrize("order", ["row_first", "row_last"])
def test_first_column_collides_with_the_previous_rows_last_column(tmp_path, small, order):
    """(r, 0) and (r - 1, w - 1) share the reference's linear index: the pixel of the group's FIRST point receives the minimum over
    both pixels' points, the other pixel keeps its last-written value -- in both file orders, so the head changes pixel, and with
    the minimum coming from the pixel that is not the head"""
    calib, P = small
    a, b = aim(P, 20.0, 3, 0), aim(P, 6.0, 2, W - 1)            # the nearer point lies on (2, 12)
    extra = [aim(P, 30.0, 3, 0), aim(P, 11.0, 2, W - 1)]         # written later: what "last wins" leaves on each pixel
    pts = ([a, b] if order == "row_first" else [b, a]) + extra
    got = check(tmp_path, calib, pts)[True]
    if order == "row_first":
        assert got[3, 0] == 6.0 and got[2, W - 1] == 11.0        # head (3, 0): the minimum, which came from the other pixel
    else:
        assert got[2, W - 1] == 6.0 and got[3, 0] == 30.0        # head (2, 12)
    assert (got > 0).sum() == 2


def test_two_hundred_points_on_one_pixel(tmp_path, small):
    calib, P = small
    rng = np.random.RandomState(5)
    depths = rng.permutation(200) * 0.25 + 3.0
    got = check(tmp_path, calib, [aim(P, d, 4, 7) for d in depths])
    assert got[True][4, 7] == 3.0 and (got[True] > 0).sum() == 1


def test_points_behind_the_image_plane_and_degenerate_ones(tmp_path, small):
    calib, P = small
    base = [aim(P, 8.0, 2, 2), aim(P, 12.0, 5, 10)]
    behind = aim(P, 0.125, 4, 4)                                 # 0 <= x < 0.25: camera Z < 0, yet it lands inside the image
    zero_z = [np.float32(0.25), np.float32(1.0), np.float32(0.5)]            # Z exactly 0
    huge = [np.float32(5.0), np.float32(1e30), np.float32(0.0)]
    rear = [np.float32(-8.0), np.float32(0.1), np.float32(0.1)]
    assert (P[2] @ np.array([0.25, 1.0, 0.5, 1.0])) == 0.0 and (P[2] @ np.append(np.float64(behind), 1.0)) < 0
    got = check(tmp_path, calib, base + [behind, zero_z, huge, rear])
    assert got[False][4, 4] == 0.0 and got[True][4, 4] == np.float32(0.125)
    plain = check(tmp_path, calib, base)
    assert same_bits(got[False], plain[False])                   # no effect elsewhere
    assert (got[True] > 0).sum() == 3 and (plain[True] > 0).sum() == 2


def test_four_column_rows_with_garbage_in_the_fourth(tmp_path, small):
    calib, P = small
    pts = random_scan(P, 90, seed=11)
    three = check(tmp_path, calib, pts, cols=3)
    four = check(tmp_path, calib, pts, cols=4)                   # device_maps leaves NaN in column 3
    assert all(same_bits(three[vd], four[vd]) for vd in (False, True))


# ---- batches ----------------------------------------------------------------------------------------------------------------

@pytest.fixture()
def batch3(tmp_path):
    """three scans: different lengths (one empty), cameras 2 and 3, native sizes 8x13, 6x10, 9x16, flips on two of them"""
    out = []
    for k, ((h, w), cam, n, flip) in enumerate((((8, 13), 2, 130, True), ((6, 10), 3, 0, False), ((9, 16), 3, 77, True))):
        calib = write_calib(tmp_path / ("cal%d" % k), small_c2c(h, w), SMALL_V2C)
        P, hw = mu.velodyne_projection(calib, cam)
        assert tuple(hw[:2]) == (h, w)
        out.append((calib, cam, random_scan(P, n, seed=40 + k, h=h, w=w), P, (h, w), flip))
    return out


@pytest.mark.parametrize("gt", [(7, 11), (8, 13)])
def test_ragged_batch(tmp_path, batch3, gt):
    for vd in (False, True):
        for calib, cam, pts, P, hw, flip in batch3:
            precondition(P, pts, vd)
        want = [host_map(calib, pts, tmp_path, cam, vd, gt, flip) for calib, cam, pts, P, hw, flip in batch3]
        got = device_maps([(pts, P, hw, flip) for calib, cam, pts, P, hw, flip in batch3], gt, vd, pad=9)      # padding rows: NaN
        for b in range(3):
            assert same_bits(got[b], want[b]), (vd, b)
        assert not got[1].any() and got[0].any() and got[2].any()
    # a flip is not the identity on these maps: the flag is seen
    unflipped = device_maps([(pts, P, hw, False) for calib, cam, pts, P, hw, flip in batch3], gt, True)
    assert same_bits(unflipped[0][:, ::-1], got[0]) and not same_bits(unflipped[0], got[0])


def test_empty_batches():
    from mdx.imgproc import velodyne_depth
    P = np.zeros((0, 3, 4))
    assert tuple(velodyne_depth(torch.zeros(0, 5, 3).cuda(), [], P, [], (4, 6)).shape) == (0, 1, 4, 6)
    out = velodyne_depth(torch.zeros(2, 0, 4).cuda(), [0, 0], np.ones((2, 3, 4)), [(8, 13), (6, 10)], (4, 6))
    assert tuple(out.shape) == (2, 1, 4, 6) and not out.any()


def test_binding_refuses_what_the_kernels_cannot_read():
    from mdx import _lib
    from mdx.imgproc import velodyne_depth
    P, hw = np.ones((1, 3, 4)), [(8, 13)]
    good = torch.zeros(1, 4, 3).cuda()
    for bad in (good.double(), good.half(), torch.zeros(1, 4, 6).cuda()[:, :, :3], torch.zeros(1, 4, 5).cuda(), torch.zeros(4, 3).cuda()):
        with pytest.raises(_lib.MdxError):
            velodyne_depth(bad, [4], P, hw, (8, 13))
    with pytest.raises(_lib.MdxError):
        velodyne_depth(good, [5], P, hw, (8, 13))              # more points than rows
    with pytest.raises(_lib.MdxError):
        velodyne_depth(good, [4], P, [(8, 1)], (8, 13))        # w < 2


def test_reproducible_across_calls_and_workspace_reuse(small, batch3):
    calib, P = small
    rng = np.random.RandomState(6)
    crowd = np.array([aim(P, d, 4, 7) for d in rng.permutation(200) * 0.25 + 3.0], np.float32)
    scans = [(crowd, P, (H, W), False), (crowd[::-1].copy(), P, (H, W), True)]
    first = device_maps(scans, (H, W), False)
    again = device_maps(scans, (H, W), False)
    other = device_maps([(pts, Pb, hw, flip) for _, _, pts, Pb, hw, flip in batch3], (7, 11), False)      # takes the freed workspace
    third = device_maps(scans, (H, W), False)
    assert same_bits(first, again) and same_bits(first, third) and other.any()
    assert first[0][4, 7] == first[1][4, W - 1 - 7] and (first[0] > 0).sum() == 1


def test_side_stream(monkeypatch, small):
    """issued on a side stream while the default stream is busy: the same map, and the workspace is recorded on that stream"""
    from mdx import _lib
    from mdx.imgproc import velodyne_depth
    calib, P = small
    pts = random_scan(P, 150, seed=21)
    want = device_maps([(pts, P, (H, W), True)], (7, 11), False)[0]
    dev_pts = torch.from_numpy(pts[None]).cuda()
    seen, made = [], []
    record, workspace = torch.Tensor.record_stream, _lib.workspace
    monkeypatch.setattr(torch.Tensor, "record_stream", lambda t, s: (seen.append((t.data_ptr(), s)), record(t, s))[1])
    monkeypatch.setattr(_lib, "workspace", lambda n, d: (made.append(workspace(n, d)), made[-1])[1])
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    a = torch.randn(2048, 2048, device="cuda")
    for _ in range(10):
        a = a @ a * 1e-3                                           # the default stream is busy
    with torch.cuda.stream(side):
        got = velodyne_depth(dev_pts, [len(pts)], P[None], [(H, W)], (7, 11), [True], False)
    side.synchronize()
    assert same_bits(got.cpu().numpy()[0, 0], want)
    assert len(made) == 1 and (made[0].data_ptr(), side) in seen
    torch.cuda.synchronize()


# ---- through the loader and the evaluation --------------------------------------------------------------------------------------

def flip_seed(want):
    """a seed under which KITTIDataset.__getitem__ draws do_flip == want (its second random.random())"""
    for seed in range(100):
        random.seed(seed)
        random.random()
        if (random.random() > 0.5) == want:
            return seed


def fake_tree_precondition(root, names, vel_depth):
    P, _ = mu.velodyne_projection(os.path.join(root, "2011_09_26"), 2)
    for line in names:
        folder, frame, _ = line.split()
        pts = np.fromfile(os.path.join(root, folder, "velodyne_points/data/%010d.bin" % int(frame)), np.float32).reshape(-1, 4)
        precondition(P, pts, vel_depth)


def test_through_the_loader(tmp_path):
    from mdx.imgproc import image_prep
    from model_loader.kitti import KITTIDataset, collate_raw
    root = str(tmp_path)
    names = fake_kitti.make(root)
    fake_tree_precondition(root, names[:2], False)
    maps = {}
    for velo in (False, True):
        ds = KITTIDataset(root, names, True, [0, -1, 1], gpu_prep=True, gpu_velo=velo)
        samples = []
        for i, flip in ((0, True), (1, False)):                   # the flip is on for one sample of the batch
            random.seed(flip_seed(flip))
            samples.append(ds[i])
        batch = collate_raw(samples)
        assert batch["raw_flip"].tolist() == [True, False] and (("velo", 0) in batch) == velo
        out = image_prep(192, 640, [0, -1, 1], 4, "cuda")(batch)
        assert not any(k == ("velo", 0) or (isinstance(k, str) and k.startswith(("velo", "depth_"))) for k in out)
        maps[velo] = out[("depth", 0)].cpu().numpy()
    assert maps[True].shape == (2, 1, 375, 1242) and same_bits(maps[True], maps[False]) and (maps[True] > 0).mean() > 0.005


def test_evaluation_ground_truth(tmp_path):
    import model_test
    from model_velodyne import load_ground_truth
    root = str(tmp_path)
    names = fake_kitti.make(root)[:2]
    fake_tree_precondition(root, names, True)
    host = model_test.load_ground_truth(root, names)
    dev = load_ground_truth(root, names, device="cuda")
    assert all(same_bits(a, b) for a, b in zip(host, load_ground_truth(root, names)))     # device=None: the host function
    assert len(dev) == 2 and all(d.dtype == np.float32 and d.shape == (375, 1242) for d in dev)
    assert all(same_bits(a, b) for a, b in zip(host, dev)) and (dev[0] > 0).sum() > 1000
