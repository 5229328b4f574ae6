#!/usr/bin/env python3
"""Cost of the decoder's last stage convolution on the low-resolution map (csrc/upconv_nhwc.hip, mdx.functional.up_conv3x3) against the
launches it replaces, at the stage-0 shapes of configs[1] (12x16x96x320) and configs[3] (8x16x160x512), float32 channels-last.

    python tools/upconv_cost.py [--out profiles/r18_upconv_cost.txt]

    new     F.up_conv3x3 forward + its backward: 1 + 3 launches
    parent  F.thin_conv3x3(F.decoder_glue(raw, bias=bias), weight) forward + backward: the glue's forward, MIOpen's forward, MIOpen's
            data gradient, the glue's backward + its column sums, the thin weight gradient + its finishing pass
Either form is captured into a hipGraph holding REPS forward + backward calls and timed as replays (HIP events around ROUNDS replays,
the two forms alternating in one process): us per forward + backward.  The two forms are compared before anything is timed."""
import argparse
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from stereo_hints_cost import _time, _write  # noqa: E402

SHAPES = [("configs[1] stage 0", 12, 96, 320), ("configs[3] stage 0", 8, 160, 512)]


def floors(B, h, w):
    """(MB moved, GFLOP) of forward, data gradient, weight gradient: the maps each must read and write once."""
    lo, hi = B * h * w * 16 * 4 / 1e6, B * h * w * 4 * 16 * 4 / 1e6
    flop = 2.0 * B * h * w * 4 * 4 * 16 * 16 / 1e9
    return [("forward", lo + hi, flop), ("data gradient", hi + 2 * lo, flop), ("weight gradient", hi + lo, flop)]


def main(reps, rounds, out):
    import torch
    importlib.import_module("digging-into-self-supervised-monocular-depth-estimation_amd")
    from mdx import functional as F
    cl = torch.channels_last
    lines = ["tools/upconv_cost.py: stage 0's second convolution, forward + backward, float32 channels-last; a hipGraph of %d calls, "
             "%d replays per form, the two forms alternating in one process, us per forward + backward (HIP events)" % (reps, rounds)]
    for name, B, h, w in SHAPES:
        g = torch.Generator().manual_seed(0)
        raw = torch.randn(B, 16, h, w, generator=g).cuda().contiguous(memory_format=cl).requires_grad_(True)
        bias = (0.1 * torch.randn(16, generator=g)).cuda().requires_grad_(True)
        weight = (0.1 * torch.randn(16, 16, 3, 3, generator=g)).cuda().contiguous(memory_format=cl).requires_grad_(True)
        gy = torch.randn(B, 16, 2 * h, 2 * w, generator=g).cuda().contiguous(memory_format=cl)

        def new():
            y = F.up_conv3x3(raw, bias, weight)
            return (y,) + torch.autograd.grad(y, (raw, bias, weight), gy)

        def parent():
            y = F.thin_conv3x3(F.decoder_glue(raw, None, elu=True, upsample=True, bias=bias), weight)
            return (y,) + torch.autograd.grad(y, (raw, bias, weight), gy)

        assert F.up_conv_ok(raw, weight)
        worst = []
        for a, b in zip(new(), parent()):
            worst.append(float((a - b).abs().max()) / float(b.abs().max()))
        assert max(worst) < 1e-5, worst
        graphs = {}
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for fn in (new, parent):
                for _ in range(3):
                    fn()
        torch.cuda.current_stream().wait_stream(side)
        for key, fn in (("new", new), ("parent", parent)):
            graphs[key] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[key]):
                for _ in range(reps):
                    fn()
            graphs[key].replay()
        torch.cuda.synchronize()
        rows = {"new": [], "parent": []}
        for _ in range(rounds):
            for key in rows:
                rows[key].append(1e3 * _time(graphs[key].replay, 1) / reps)
        lines.append("%s, %d x 16 x %d x %d -> %d x %d; new against parent, largest difference over the array's maximum (y, graw, gbias, "
                     "gweight): %s" % (name, B, h, w, 2 * h, 2 * w, "  ".join("%.1e" % v for v in worst)))
        lines.append("  new     %s   min %.1f us;  4 launches" % ("  ".join("%.1f" % x for x in rows["new"]), min(rows["new"])))
        lines.append("  parent  %s   min %.1f us;  7 launches" % ("  ".join("%.1f" % x for x in rows["parent"]), min(rows["parent"])))
        total = 0.0
        for part, mb, gf in floors(B, h, w):
            t_b, t_f = mb / 5.5, 1e3 * gf / 157.3                      # us at 5.5 TB/s (what the streaming kernels here reach), at the f32 MFMA peak
            total += max(t_b, t_f)
            lines.append("    floor, %-15s %6.1f MB %5.2f GFLOP: %5.1f us of bytes at 5.5 TB/s, %5.1f us at the f32 MFMA peak" % (part, mb, gf, t_b, t_f))
        lines.append("  new / parent %.3f; the new form is at %.2f x the sum of its floors (%.1f us)" % (min(rows["new"]) / min(rows["parent"]), min(rows["new"]) / total, total))
    _write(lines, out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    main(a.reps, a.rounds, a.out)
