#!/usr/bin/env python3
"""Cost of the sparse lidar term (csrc/sparse_depth.hip, mdx.functional.sparse_depth_loss) at configs[1]: batch 12, disparities
192x640 ... 24x80 (7.8 MB), ground truth 375x1242 (22.4 MB).

    python tools/sparse_depth_cost.py --what kernels [--out profiles/r14_sparse_depth_cost.txt]
        one process, HIP events around REPS forward + backward pairs, ROUNDS rounds alternating, once with a seeded ~4.5 % valid
        mask and once dense:
          mdx_sparse_depth_fwd + mdx_sparse_depth_bwd      the two C-ABI calls over buffers made once: 2 + nscales launches
          sparse_depth_loss(...) + backward                the autograd node as the step runs it (allocations, the weighted sum)
          the torch composite + backward                   mdx.composite.sparse_depth_loss on the same device tensors: interpolate,
                                                           where, log, sqrt, sum per scale and autograd's backward of them
        Time per pair, launches per pair (counted by torch's profiler in a pass of its own) and GB/s over the bytes the pair must
        move (gt twice, the disparities twice, the gradients once); a loop re-reads them, so they stay inside the Infinity Cache
        and the rate is no fraction of the HBM peak.  The pair's results are compared with the composite's before anything is timed.
    python tools/sparse_depth_cost.py --what step
        the training loop's step -- the captured step (model_train.graphed_step) and, with the option on, the eager launches that
        add the step's term and count to the epoch's sums (trainer.depth_supervision_add) -- with --depth_supervision 0 and 0.05 on
        the same synthetic batch: host clock around N replays ending in a synchronise
"""
import argparse
import ctypes as C
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, GT, SIZES = 12, (375, 1242), [(192, 640), (96, 320), (48, 160), (24, 80)]
MIN_DEPTH, MAX_DEPTH, EPS = 0.1, 100.0, 1e-3


def _time(fn, reps):
    """Mean microseconds per call over `reps` calls between two HIP events."""
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return 1e3 * start.elapsed_time(stop) / reps


def _launches(fn):
    """Device kernels one call of fn launches, by torch's profiler; None where the profiler gives no device events."""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or None
    except Exception as exc:  # noqa: BLE001
        print("launch count not measured: %r" % (exc,), flush=True)
        return None


def kernels(reps, rounds, out):
    import torch
    importlib.import_module("digging-into-self-supervised-monocular-depth-estimation_amd")
    from mdx import composite
    from mdx import functional as F
    from mdx._lib import api, ptr, ptr_array, stream, workspace
    dev = "cuda"
    gen = torch.Generator().manual_seed(0)
    disps = [(0.02 + 0.9 * torch.rand(B, 1, h, w, generator=gen)).to(dev) for h, w in SIZES]
    depth = 1.0 + 79.0 * torch.rand(B, 1, *GT, generator=gen)
    mask = torch.rand(B, 1, *GT, generator=gen) < 0.045
    weights = torch.tensor([1.0, 0.5, 0.25, 0.125], device=dev)
    n = len(SIZES)
    hs, ws_ = (C.c_int32 * n)(*[h for h, _ in SIZES]), (C.c_int32 * n)(*[w for _, w in SIZES])
    nbytes = 2 * 4 * B * GT[0] * GT[1] + 3 * 4 * sum(d.numel() for d in disps)
    lines = ["tools/sparse_depth_cost.py --what kernels: %d images, disparities %s, ground truth %d x %d; the pair moves %.1f MB (gt "
             "twice, disparities twice, gradients once); %d rounds x %d pairs (the composite: %d), alternating in one process, us per "
             "forward + backward pair (HIP events)" % (B, " ".join("%dx%d" % s for s in SIZES), GT[0], GT[1], nbytes / 1e6, rounds, reps,
                                                        max(reps // 10, 5))]
    for label, gt in (("~4.5 % valid", torch.where(mask, depth, torch.zeros_like(depth)).to(dev)), ("dense", depth.to(dev))):
        xs = [d.clone().requires_grad_(True) for d in disps]
        out_t = torch.empty(n + 1, device=dev)
        dd = [torch.empty_like(d) for d in disps]
        nws = api.mdx_sparse_depth_workspace_bytes(n, B, GT[0], GT[1])
        wsp = workspace(nws, dev)
        gout = torch.cat([weights, torch.zeros(1, device=dev)])
        dp, ddp = ptr_array(disps), ptr_array(dd)

        def abi_pair():
            st = stream()
            api.mdx_sparse_depth_fwd(n, B, hs, ws_, dp, ptr(gt), GT[0], GT[1], MIN_DEPTH, MAX_DEPTH, MIN_DEPTH, MAX_DEPTH, EPS,
                                     ptr(out_t), ptr(wsp, torch.uint8), nws, st)
            api.mdx_sparse_depth_bwd(n, B, hs, ws_, dp, ptr(gt), GT[0], GT[1], MIN_DEPTH, MAX_DEPTH, MIN_DEPTH, MAX_DEPTH, EPS,
                                     ptr(out_t), ptr(gout), ddp, ptr(wsp, torch.uint8), nws, st)

        def node_pair():
            res = F.sparse_depth_loss(xs, gt, MIN_DEPTH, MAX_DEPTH, eps=EPS)
            return res, torch.autograd.grad((res["loss"] * weights).sum(), xs)

        def composite_pair():
            res = composite.sparse_depth_loss(xs, gt, MIN_DEPTH, MAX_DEPTH, eps=EPS)
            return res, torch.autograd.grad((res["loss"] * weights).sum(), xs)

        # the same numbers first
        abi_pair()
        (res_k, g_k), (res_c, g_c) = node_pair(), composite_pair()
        torch.cuda.synchronize()
        valid = int(res_k["valid"])
        assert valid == int(res_c["valid"]) == int(out_t[n])
        worst = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(g_k, g_c))
        worst_abi = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(dd, g_c))
        loss_err = float(((res_k["loss"] - res_c["loss"]).abs() / res_c["loss"].abs()).max())
        assert worst < 1e-3 and worst_abi < 1e-3 and loss_err < 1e-4, (worst, worst_abi, loss_err)
        calls = [("mdx_sparse_depth_fwd + mdx_sparse_depth_bwd", abi_pair), ("sparse_depth_loss + backward", node_pair),
                 ("torch composite + backward", composite_pair)]
        counts = {k: _launches(fn) for k, fn in calls}
        for _, fn in calls:
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        rows = {k: [] for k, _ in calls}
        for _ in range(rounds):
            for k, fn in calls:
                rows[k].append(_time(fn, reps if "composite" not in k else max(reps // 10, 5)))
        lines.append(" %s: %d valid pixels (%.2f %%); kernels against the float32 composite: terms within %.1e, gradients within %.1e "
                     "of the largest entry" % (label, valid, 100.0 * valid / (B * GT[0] * GT[1]), loss_err, worst))
        for k, v in rows.items():
            best = min(v)
            lines.append("  %-44s %s   min %.1f us = %.0f GB/s over %.1f MB; launches per pair: %s" % (
                k, "  ".join("%.1f" % x for x in v), best, nbytes / best / 1e3, nbytes / 1e6,
                counts[k] if counts[k] is not None else "not measured"))
        lines.append("  C-ABI pair / composite (min over rounds): %.4f" % (min(rows[calls[0][0]]) / min(rows[calls[2][0]])))
    text = "\n".join(lines)
    print(text, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(text + "\n")


def step(steps, out):
    import torch
    bench = importlib.import_module("bench")
    importlib.import_module("digging-into-self-supervised-monocular-depth-estimation_amd")
    from model_train import trainer
    runs = {}
    for weight in (0.0, 0.05):
        torch.manual_seed(0)
        opt = bench.make_opt(B)
        opt.graph, opt.depth_supervision = True, weight
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
                    tr.depth_supervision_add(outputs)
            torch.cuda.synchronize()
            times[w].append(1e3 * (time.perf_counter() - t0) / steps)
    valid = float(outputs["depth_valid"]) / B
    lines = ["tools/sparse_depth_cost.py --what step: captured step + the epoch sums' eager launches, batch %d at 192x640, synthetic batch (%.0f valid pixels per image), "
             "ms per step over 3 x %d replays, the two trainers alternating in one process" % (B, valid, steps)]
    for w, v in times.items():
        lines.append("  --depth_supervision %-5g %s   min %.3f ms" % (w, "  ".join("%.3f" % x for x in v), min(v)))
    a, b = min(times[0.0]), min(times[0.05])
    lines.append("  with the term / without (min over rounds): %.4f  (+%.1f us per step)" % (b / a, 1e3 * (b - a)))
    text = "\n".join(lines)
    print(text, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["kernels", "step"], required=True)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    if a.what == "kernels":
        kernels(a.reps, a.rounds, a.out)
    else:
        step(a.steps, a.out)
