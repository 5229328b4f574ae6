"""Evaluation ground truth with the projection on the GPU: model_test.load_ground_truth's maps through
mdx.imgproc.velodyne_depth (csrc/velodyne.hip), bit for bit.  model_test.py itself is untouched: hand the result to
model_test.inference(..., ground_truth=load_ground_truth(datapath, lines, device)).
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from model_utility import velodyne_projection  # noqa: E402


def load_ground_truth(datapath, lines, device=None, chunk=16):
    """velodyne depth of camera 2 (vel_depth) at the image's native size, one float32 map per test line.
    device=None: model_test.load_ground_truth, the host function.  With a device: the scans are projected there, `chunk` scans
    per call, grouped by native size; a day's calibration is parsed once."""
    if device is None:
        from model_test import load_ground_truth as host
        return host(datapath, lines)
    from mdx.imgproc import velodyne_depth
    calibs, scans = {}, []
    for line in lines:
        folder, frame_id, _ = line.split()
        calib = os.path.join(datapath, folder.split("/")[0])
        if calib not in calibs:
            P, hw = velodyne_projection(calib, 2)
            calibs[calib] = (P, tuple(int(v) for v in hw[:2]))
        scans.append((os.path.join(datapath, folder, "velodyne_points/data", "{:010d}.bin".format(int(frame_id))), calib))
    out = [None] * len(scans)
    with torch.cuda.device(device):
        for first in range(0, len(scans), chunk):
            part = range(first, min(first + chunk, len(scans)))
            pts = {}
            for i in part:
                p = np.fromfile(scans[i][0], dtype=np.float32).reshape(-1, 4)
                pts[i] = p[p[:, 0] >= 0, :3]
            for hw in sorted({calibs[scans[i][1]][1] for i in part}):            # one output size per call
                sel = [i for i in part if calibs[scans[i][1]][1] == hw]
                block = np.zeros((len(sel), max(len(pts[i]) for i in sel), 3), np.float32)
                for j, i in enumerate(sel):
                    block[j, :len(pts[i])] = pts[i]
                maps = velodyne_depth(torch.from_numpy(block).to(device), [len(pts[i]) for i in sel],
                                      [calibs[scans[i][1]][0] for i in sel], [hw] * len(sel), hw, vel_depth=True).cpu().numpy()
                for j, i in enumerate(sel):
                    out[i] = maps[j, 0]
    return out
