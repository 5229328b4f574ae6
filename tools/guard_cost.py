#!/usr/bin/env python3
"""Cost of the optimiser's step guard (mdx/optim.py: max_grad_norm, skip_nonfinite) on the trainer at configs[1] (ResNet-18,
192x640, batch 12, fp32: 27.8 M parameters).

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/guard_cost.py --what trace
        one trainer, eager steps: N unguarded, N guarded (clip + skip), then N x torch.nn.utils.clip_grad_norm_(foreach=True) --
        the workaround without the guard -- on the gradients the last backward left
    python tools/guard_cost.py --what summarise OUT
        per-launch times of adam_step_kernel, grad_sumsq_kernel, guard_finish_kernel, adam_step_guarded_kernel, and the kernel
        time of one clip_grad_norm_ (every kernel after the last guarded Adam launch, / N)
    python tools/guard_cost.py --what step
        the captured training step (model_train.graphed_step), guard off against on: host clock around N replays
"""
import argparse
import collections
import csv
import glob
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MDX = ("adam_step_kernel", "grad_sumsq_kernel", "guard_finish_kernel", "adam_step_guarded_kernel")


def _trainer(graph, guard):
    import torch
    bench = importlib.import_module("bench")
    importlib.import_module("digging-into-self-supervised-monocular-depth-estimation_amd")
    from model_train import trainer
    torch.manual_seed(0)
    opt = bench.make_opt(12)
    opt.graph = graph
    if guard:
        opt.clip_grad_norm, opt.skip_nonfinite = 1.0, 1
    tr = trainer(opt)
    tr.setting.set_train()
    return tr, bench.one_batch(tr.setting, tr.device)


def trace(steps):
    import torch
    tr, inputs = _trainer(False, False)
    opt = tr.setting.optim["optimizer"]
    for _ in range(3 + steps):
        tr._eager_step(dict(inputs))
    opt.max_grad_norm, opt.skip_nonfinite = 1.0, True
    for _ in range(steps):
        tr._eager_step(dict(inputs))
    torch.cuda.synchronize()
    print("guard: %s" % opt.guard_stats(), flush=True)
    params = [p for g in opt.param_groups for p in g["params"] if p.grad is not None]
    print("gradients: %d tensors, %.1f MB" % (len(params), sum(p.numel() for p in params) * 4 / 1e6), flush=True)
    for _ in range(steps):
        torch.nn.utils.clip_grad_norm_(params, 1.0, foreach=True)
    torch.cuda.synchronize()


def summarise(src, steps):
    dur = collections.defaultdict(list)
    rows = []
    for f in glob.glob(os.path.join(src, "**", "*_kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    last = max(i for i, r in enumerate(rows) if "adam_step_guarded_kernel" in r[2])
    for s, e, name in rows[:last + 1]:
        for k in MDX:
            if "mdx::" + k + "(" in name or name.replace("void ", "").split("(")[0] == "mdx::" + k:
                dur[k].append((e - s) / 1e3)
    clip = collections.defaultdict(list)
    for s, e, name in rows[last + 1:]:
        clip[name.replace("void ", "")[:100]].append((e - s) / 1e3)
    print("per launch, us (mean / min / launches):")
    mean = {}
    for k in MDX:
        v = dur[k]
        mean[k] = sum(v) / len(v)
        print("  %-28s %8.2f %8.2f %6d" % (k, mean[k], min(v), len(v)))
    added = mean["grad_sumsq_kernel"] + mean["guard_finish_kernel"] + mean["adam_step_guarded_kernel"] - mean["adam_step_kernel"]
    total = sum(sum(v) for v in clip.values()) / steps
    print("clip_grad_norm_(foreach=True), kernel time per call over %d calls: %.2f us in %d launches" %
          (steps, total, sum(len(v) for v in clip.values()) // steps))
    for name, v in sorted(clip.items(), key=lambda kv: -sum(kv[1])):
        print("  %8.2f us/call %4d launches/call  %s" % (sum(v) / steps, len(v) // steps, name))
    print("added GPU time of the guard (sum of squares + finish + guarded Adam - plain Adam): %.2f us = %.2f of torch's clip"
          % (added, added / total))


def step(steps):
    import torch
    for guard in (False, True):
        tr, inputs = _trainer(True, guard)
        for _ in range(5):
            tr.train_step(dict(inputs))
        torch.cuda.synchronize()
        best = []
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.train_step(dict(inputs))
            torch.cuda.synchronize()
            best.append(1e3 * (time.perf_counter() - t0) / steps)
        assert tr._graphed is not None
        opt = tr.setting.optim["optimizer"]
        print("captured step, guard %s: ms per step over 3 x %d replays: %s%s" % (
            "on (clip 1.0 + skip)" if guard else "off", steps, "  ".join("%.3f" % b for b in best),
            "   %s" % opt.guard_stats() if guard else ""), flush=True)
        del tr
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["trace", "summarise", "step"], required=True)
    ap.add_argument("dir", nargs="?")
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    if a.what == "trace":
        trace(a.steps)
    elif a.what == "summarise":
        summarise(a.dir, a.steps)
    else:
        step(a.steps)
