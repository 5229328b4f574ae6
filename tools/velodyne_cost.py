#!/usr/bin/env python3
"""Cost of the velodyne ground truth on the device (mdx.imgproc.velodyne_depth, csrc/velodyne.hip) beside what it replaces, for a
batch of 12 scans of 120 000 points (a 360-degree sweep: half of them behind the car) on the 375x1242 grid.

    python tools/velodyne_cost.py [--out profiles/r13_velodyne_cost.json]

  device (HIP events around one call each, warm, median of RUNS calls):
    velodyne_depth()                       the binding: job table, workspace from the allocator, three launches -- on the points the
                                           worker hands over (x >= 0, [n, 3])
    mdx_velodyne_depth alone               the three launches over a job table and workspace built once
    the same on the raw [120000, 4] scans  what the pass costs when nothing was filtered on the host
    torch.zeros + scatter_                 what image_prep does today with the (index, value) pairs the workers send
    torch.zeros of the workspace           the clear the pass does NOT make (16 bytes per native pixel)
  host, one core, per sample:
    KITTIDataset.load_point                calibration parse + projection + duplicates + nonzero (today's worker)
    KITTIDataset.load_scan                 np.fromfile + the x >= 0 filter (the gpu_velo worker)
    bytes handed over per sample, both ways
One JSON line."""
import argparse
import importlib
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

importlib.import_module("digging-into-self-supervised-monocular-depth-estimation_amd")


def write_scans(root, names, points, seed=0):
    """fake_kitti's tree with scans of `points` points over the full circle: range 3..70 m, elevation as a velodyne's"""
    rng = np.random.RandomState(seed)
    folder = names[0].split()[0]
    d = os.path.join(root, folder, "velodyne_points/data")
    for f in sorted(os.listdir(d)):
        az, rg = rng.uniform(-np.pi, np.pi, points), rng.uniform(3, 70, points)
        el = rng.uniform(-0.43, 0.04, points)
        pts = np.stack([rg * np.cos(az), rg * np.sin(az), rg * np.sin(el), rng.uniform(0, 1, points)], 1)
        pts.astype(np.float32).tofile(os.path.join(d, f))


def event_us(fn, runs):
    """median (and min) microseconds of one call between two HIP events, over `runs` calls"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(runs):
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        out.append(1e3 * start.elapsed_time(stop))
    return round(statistics.median(out), 1), round(min(out), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--host-samples", type=int, default=24)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    import fake_kitti
    from model_loader.kitti import KITTIDataset, collate_raw
    torch.set_num_threads(1)
    out = {"what": "tools/velodyne_cost.py", "batch": a.batch, "points_per_scan": a.points, "grid": [375, 1242], "runs": a.runs}
    with tempfile.TemporaryDirectory() as root:
        names = fake_kitti.make(root, n_frames=a.batch + 2)
        write_scans(root, names, a.points)
        off = KITTIDataset(root, names, False, [0], gpu_prep=True)
        on = KITTIDataset(root, names, False, [0], gpu_prep=True, gpu_velo=True)
        folder = names[0].split()[0]

        def per_sample(fn):
            fn(0)
            t0 = time.perf_counter()
            for i in range(a.host_samples):
                fn(1 + i % len(names))
            return round(1e3 * (time.perf_counter() - t0) / a.host_samples, 3)

        def old(i):
            depth = off.load_point(folder, i, "l", False)
            flat = depth.reshape(-1)
            idx = torch.nonzero(flat).reshape(-1)
            return idx.to(torch.int32), flat[idx]
        out["host_ms_per_sample_load_point"] = per_sample(old)
        out["host_ms_per_sample_load_scan"] = per_sample(lambda i: on.load_scan(folder, i, "l"))
        so, sn = [off[i] for i in range(a.batch)], [on[i] for i in range(a.batch)]
        out["bytes_per_sample_pairs"] = int(np.mean([8 * s[("depth_idx", 0)].numel() for s in so]))
        out["bytes_per_sample_points"] = int(np.mean([4 * s[("velo", 0)].numel() for s in sn]))
        out["points_kept_per_scan"] = int(np.mean([s[("velo", 0)].shape[0] for s in sn]))
        out["pixels_hit_per_scan"] = int(np.mean([s[("depth_idx", 0)].numel() for s in so]))
        if torch.cuda.is_available():
            from mdx import _lib, imgproc
            bo, bn = collate_raw(so), collate_raw(sn)
            pts = bn[("velo", 0)].cuda()
            counts, P, hw = bn["velo_n"].tolist(), bn["velo_P"].numpy(), bn["velo_hw"].tolist()
            idx, val = bo[("depth_idx", 0)].cuda().long(), bo[("depth_val", 0)].cuda()
            raw = torch.from_numpy(np.stack([np.fromfile(os.path.join(root, folder, "velodyne_points/data/%010d.bin" % int(line.split()[1])),
                                                         np.float32).reshape(-1, 4) for line in names[:a.batch]])).cuda()
            gh, gw = 375, 1242

            def scatter():
                buf = torch.zeros(idx.shape[0], gh * gw + 1, device="cuda")
                buf.scatter_(1, idx, val)
                return buf[:, :gh * gw].reshape(-1, 1, gh, gw).contiguous()
            want = scatter()
            got = imgproc.velodyne_depth(pts, counts, P, hw, (gh, gw))
            out["device_equals_host_bitwise"] = bool(torch.equal(got.view(torch.int32), want.view(torch.int32)))
            out["raw_equals_filtered_bitwise"] = bool(torch.equal(
                imgproc.velodyne_depth(raw, [a.points] * a.batch, P, hw, (gh, gw)).view(torch.int32), got.view(torch.int32)))
            nbytes = _lib.api.mdx_velodyne_workspace_bytes(a.batch, max(counts), gh, gw)
            ws, dst = _lib.workspace(nbytes, "cuda"), torch.empty(a.batch, 1, gh, gw, device="cuda")
            jobs = np.zeros(a.batch, imgproc.VELODYNE_JOB)
            k = np.arange(a.batch, dtype=np.uint64)
            jobs["points"] = pts.data_ptr() + k * np.uint64(12 * pts.shape[1])
            jobs["out"] = dst.data_ptr() + k * np.uint64(4 * gh * gw)
            jobs["P"], jobs["n"], jobs["stride"] = P.reshape(-1, 12), counts, 3
            jobs["h"], jobs["w"], jobs["gh"], jobs["gw"] = gh, gw, gh, gw
            calls = [("velodyne_depth", lambda: imgproc.velodyne_depth(pts, counts, P, hw, (gh, gw))),
                     ("mdx_velodyne_depth_alone", lambda: _lib.api.mdx_velodyne_depth(jobs.ctypes.data, a.batch, ws.data_ptr(),
                                                                                     ws.numel(), _lib.stream())),
                     ("velodyne_depth_raw_scans", lambda: imgproc.velodyne_depth(raw, [a.points] * a.batch, P, hw, (gh, gw))),
                     ("zeros_scatter", scatter),
                     ("zeros_of_the_workspace", lambda: torch.zeros(nbytes, dtype=torch.uint8, device="cuda"))]
            for _, fn in calls:
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            for name, fn in calls:
                out["device_us_%s_median" % name], out["device_us_%s_min" % name] = event_us(fn, a.runs)
            assert torch.equal(dst.view(torch.int32), want.view(torch.int32))
            out["workspace_bytes"] = int(nbytes)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
