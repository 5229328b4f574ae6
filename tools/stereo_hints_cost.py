#!/usr/bin/env python3
"""Cost of the stereo matcher (csrc/stereo_hints.hip, mdx.functional.stereo_hints) at configs[4]: batch 12, 192x640, mono + stereo.

    python tools/stereo_hints_cost.py --what kernels [--out profiles/r16_stereo_hints_cost.txt]
        one process, HIP events around REPS calls of mdx_stereo_hints over buffers made once, ROUNDS rounds, D = 64 and D = 128
        alternating, on rendered pairs of the synthetic scenes (model_tool.synthetic, geometry=True): ms per call, the bytes the
        form moves (S written once and read + written seven times by the path passes, read twice by the winners) and what that
        traffic would take at 8 TB/s.  The outputs are compared with mdx.composite.stereo_hints on the first image before anything
        is timed.
    rocprofv3 --kernel-trace --output-format csv -d OUT -- python3 tools/stereo_hints_cost.py --what trace
        a few calls per D and nothing else, for a kernel trace;
    python tools/stereo_hints_cost.py --what launches --trace OUT [--out ...]
        the per-launch times of that trace: every launch of a call in order, mean over the traced calls, and each path pass's
        traffic over 8 TB/s as a share of its time.
    python tools/stereo_hints_cost.py --what step [--out ...]
        the training loop's step at configs[4] (frame_ids 0 -1 1 s) -- the captured step and, with the option on, the eager launches
        that add the step's term and count to the epoch's sums (trainer.stereo_hints_add) -- with --stereo_hints 0 and 0.05 on the
        same synthetic batch: host clock around N replays ending in a synchronise, the two trainers alternating.
"""
import argparse
import csv
import glob
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, H, W = 12, 192, 640
PEAK = 8e12            # bytes per second, HBM3E


def path_bytes(D):
    """The path passes' traffic: S (2 bytes per element) written once and read + written seven times."""
    return B * H * W * D * 2 * 15


def _pairs(dev):
    """Twelve rendered stereo pairs (two scenes' worth of the synthetic geometry set would cost seconds each at this size: four
    scenes, each used three times with another noise) -> target, partner [B,3,H,W], K, T [B,4,4] on the device."""
    import torch
    from model_tool.synthetic import make_K, scene
    K = make_K(H, W)[0]
    T = torch.eye(4, dtype=torch.float64)
    T[0, 3] = 0.1
    ts, ps = [], []
    for seed in range(4):
        world = scene(torch.Generator().manual_seed(seed))
        t, _ = world.render(K, torch.eye(4, dtype=torch.float64), H, W)
        p, _ = world.render(K, T, H, W)
        for k in range(3):
            g = torch.Generator().manual_seed(10 * seed + k)
            ts.append((t + 0.01 * torch.randn(t.shape, generator=g)).clamp(0, 1))
            ps.append((p + 0.01 * torch.randn(p.shape, generator=g)).clamp(0, 1))
    Ks, Ts = K[None].repeat(B, 1, 1), T.float()[None].repeat(B, 1, 1)
    Ts[1::2, 0, 3] = -0.1                      # every other sample looks the other way: partner and target change places
    target, partner = torch.stack(ts), torch.stack(ps)
    target[1::2], partner[1::2] = torch.stack(ps)[1::2], torch.stack(ts)[1::2]
    return target.to(dev), partner.to(dev), Ks.to(dev), Ts.to(dev)


def _call(D):
    import torch
    from mdx._lib import api, ptr, stream, workspace
    dev = "cuda"
    if not hasattr(_call, "data"):
        _call.data = _pairs(dev)
    target, partner, K, T = _call.data
    nws = api.mdx_stereo_hints_workspace_bytes(B, H, W, D)
    ws = workspace(nws, dev)
    disp = torch.empty(B, 1, H, W, device=dev)
    depth, valid = torch.empty_like(disp), torch.empty(B, 1, H, W, device=dev, dtype=torch.uint8)

    def run():
        api.mdx_stereo_hints(ptr(target), ptr(partner), ptr(K), ptr(T), B, H, W, D, 8, 64, ptr(disp), ptr(depth),
                             ptr(valid, torch.uint8), ptr(ws, torch.uint8), nws, stream())
    return run, (disp, depth, valid), nws


def _time(fn, reps):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def _write(lines, out):
    text = "\n".join(lines)
    print(text, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(text + "\n")


def kernels(reps, rounds, out):
    import torch
    importlib.import_module("digging-into-self-supervised-monocular-depth-estimation_amd")
    from mdx import composite
    calls = {D: _call(D) for D in (64, 128)}
    lines = ["tools/stereo_hints_cost.py --what kernels: mdx_stereo_hints on %d rendered pairs of %d x %d, P1 8, P2 64; %d rounds x %d "
             "calls, D = 64 and 128 alternating in one process, ms per call (HIP events)" % (B, H, W, rounds, reps)]
    target, partner, K, T = _call.data
    for D, (run, (disp, depth, valid), nws) in calls.items():
        run()
        torch.cuda.synchronize()
        want = composite.stereo_hints(target[:1].cpu(), partner[:1].cpu(), K[:1].cpu(), T[:1].cpu(), D)
        assert torch.equal(valid[:1].cpu(), want["valid"]) and torch.equal(disp[:1].cpu(), want["disp"]) \
            and torch.equal(depth[:1].cpu(), want["depth"]), "D = %d: the kernels and the composite differ on the first pair" % D
        lines.append(" D = %d: workspace %.1f MB; valid share %.3f over the batch; first pair equal to the composite bit for bit"
                     % (D, nws / 1e6, float(valid.float().mean())))
    for run, _, _ in calls.values():
        for _ in range(3):
            run()
    torch.cuda.synchronize()
    rows = {D: [] for D in calls}
    for _ in range(rounds):
        for D, (run, _, _) in calls.items():
            rows[D].append(_time(run, reps))
    for D, v in rows.items():
        best, nb = min(v), path_bytes(D)
        lines.append("  D = %-4d %s   min %.3f ms; 12 launches; the path passes move %.2f GB = %.3f ms at 8 TB/s (%.0f %% of the call)"
                     % (D, "  ".join("%.3f" % x for x in v), best, nb / 1e9, 1e3 * nb / PEAK, 100 * 1e3 * nb / PEAK / best))
    _write(lines, out)


def trace(reps):
    import torch
    importlib.import_module("digging-into-self-supervised-monocular-depth-estimation_amd")
    for D in (64, 128):
        run = _call(D)[0]
        for _ in range(reps):
            run()
        torch.cuda.synchronize()


def launches(src, out):
    f = max(glob.glob(os.path.join(src, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    rows = [r for r in csv.DictReader(open(f)) if "stereo_hints" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert rows and len(rows) % 12 == 0, len(rows)
    calls = [rows[i:i + 12] for i in range(0, len(rows), 12)]
    lines = ["tools/stereo_hints_cost.py --what launches: rocprofv3 --kernel-trace of --what trace, us per launch in launch order, mean "
             "over the traced calls (min); a path pass's share = its S traffic at 8 TB/s over its time"]
    names = ["luma", "census", "path (0,+1) writes S", "path (0,-1)", "path (+1,0)", "path (-1,0)", "path (+1,+1)", "path (+1,-1)",
             "path (-1,+1)", "path (-1,-1)", "winners", "outputs"]
    for D, tag in ((64, "<1>"), (128, "<2>")):
        mine = [c for c in calls if tag in c[2]["Kernel_Name"]]
        if not mine:
            continue
        lines.append(" D = %d, %d calls" % (D, len(mine)))
        total = 0.0
        for k, name in enumerate(names):
            us = [(int(c[k]["End_Timestamp"]) - int(c[k]["Start_Timestamp"])) / 1e3 for c in mine]
            mean = sum(us) / len(us)
            total += mean
            share = ""
            if name.startswith("path"):
                nb = B * H * W * D * 2 * (1 if k == 2 else 2)
                share = "   %.0f MB = %.1f us at 8 TB/s: %.0f %%" % (nb / 1e6, 1e6 * nb / PEAK, 100 * 1e6 * nb / PEAK / mean)
            lines.append("  %-22s %9.1f (%9.1f)%s" % (name, mean, min(us), share))
        lines.append("  %-22s %9.1f" % ("sum of the launches", total))
    _write(lines, out)


def step(steps, out):
    import torch
    bench = importlib.import_module("bench")
    importlib.import_module("digging-into-self-supervised-monocular-depth-estimation_amd")
    from model_train import trainer
    runs = {}
    for weight in (0.0, 0.05):
        torch.manual_seed(0)
        opt = bench.make_opt(B, frame_ids=(0, -1, 1, "s"))
        opt.graph, opt.stereo_hints = True, weight
        tr = trainer(opt)
        tr.setting.set_train()
        runs[weight] = (tr, bench.one_batch(tr.setting, tr.device))
    for tr, inputs in runs.values():
        for _ in range(5):
            tr.train_step(dict(inputs))
        assert tr._graphed is not None
    torch.cuda.synchronize()
    times = {w: [] for w in runs}
    for _ in range(3):                                 # alternating: both see the same neighbours on the machine
        for w, (tr, inputs) in runs.items():
            t0 = time.perf_counter()
            for _ in range(steps):
                outputs = tr.train_step(dict(inputs))
                if w > 0:                              # as trainer.train does behind every step: the epoch's sums, eager launches
                    tr.stereo_hints_add(outputs)
            torch.cuda.synchronize()
            times[w].append(1e3 * (time.perf_counter() - t0) / steps)
    share = float(outputs["hint_valid"]) / (B * H * W)
    lines = ["tools/stereo_hints_cost.py --what step: captured step + the epoch sums' eager launches, batch %d at %dx%d, frame_ids 0 -1 1 s, "
             "synthetic batch (hint on %.3f of the pixels), ms per step over 3 x %d replays, the two trainers alternating in one process"
             % (B, H, W, share, steps)]
    for w, v in times.items():
        lines.append("  --stereo_hints %-5g %s   min %.3f ms" % (w, "  ".join("%.3f" % x for x in v), min(v)))
    a, b = min(times[0.0]), min(times[0.05])
    lines.append("  with the term / without (min over rounds): %.4f  (+%.1f us per step)" % (b / a, 1e3 * (b - a)))
    _write(lines, out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["kernels", "trace", "launches", "step"], required=True)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--trace", type=str, default="")
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    if a.what == "kernels":
        kernels(a.reps, a.rounds, a.out)
    elif a.what == "trace":
        trace(min(a.reps, 5))
    elif a.what == "launches":
        launches(a.trace, a.out)
    else:
        step(a.steps, a.out)
