#!/usr/bin/env python3
"""Cost of the weight digests (mdx/optim.py: WeightDigest, csrc/digest.hip) on the trainer at configs[1] (ResNet-18, 192x640, batch 12,
fp32): its own tensor list -- the trained float32 master parameters of the four networks.

    python tools/digest_cost.py --what kernels [--out profiles/r09_digest_cost.txt]
        one process, HIP events around REPS calls, ROUNDS rounds alternating: mdx_adam_grad_sumsq, mdx_digest_words, mdx_adam_grad_sumsq
        again over the SAME tensors with the SAME block map -- both are read-only passes over the same bytes, one float multiply-add
        in double per word against three 32-bit integer multiplies.  The second grad_sumsq column is the tool's own run-to-run
        spread.  Time per pass and GB/s at 4 B / element.
    python tools/digest_cost.py --what step [--every 100]
        the captured training step (model_train.graphed_step) with --check_weights 0 and --check_weights EVERY, checked as
        trainer.train checks: host clock around N replays, the checks between them
"""
import argparse
import ctypes as C
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _trainer(graph, check):
    import torch
    bench = importlib.import_module("bench")
    importlib.import_module("digging-into-self-supervised-monocular-depth-estimation_amd")
    from model_train import trainer
    torch.manual_seed(0)
    opt = bench.make_opt(12)
    opt.graph, opt.check_weights = graph, check
    tr = trainer(opt)
    tr.setting.set_train()
    return tr, bench.one_batch(tr.setting, tr.device)


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


def kernels(reps, rounds, out):
    import torch
    tr, _ = _trainer(False, 1)
    from mdx._lib import api, stream
    from mdx.optim import _Table, _device_table
    digest = tr.setting.optim["digest"]
    ts = digest.tensors
    n = sum(t.numel() for t in ts)
    # grad_sumsq over the weights themselves: its table is read for numel only, the "gradients" are the same pointers the digest reads
    table = _device_table(_Table, api.mdx_adam_table_entry_bytes(), ts, ts, ts, ts)
    launches = digest._launches
    partials = torch.empty(sum(nb for _, _, _, nb in launches), dtype=torch.float64, device=ts[0].device)
    garrs = [(C.c_void_p * count)(*[t.data_ptr() for t in ts[first:first + count]]) for first, count, _, _ in launches]

    def sumsq():
        slot = 0
        for garr, (first, count, blockmap, nblocks) in zip(garrs, launches):
            api.mdx_adam_grad_sumsq(table.data_ptr(), first, count, garr, blockmap.data_ptr(), nblocks, partials.data_ptr() + 8 * slot, stream())
            slot += nblocks

    calls = [("grad_sumsq (csrc/adam.hip)", sumsq), ("digest_words (csrc/digest.hip)", digest.compute), ("grad_sumsq, again", sumsq)]
    for _, fn in calls:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    rows = {k: [] for k, _ in calls}
    for _ in range(rounds):
        for k, fn in calls:
            rows[k].append(_time(fn, reps))
    lines = ["tools/digest_cost.py --what kernels: %d tensors, %.2f M elements (%.1f MB), %d launch(es) per pass (the digest: + one clearing "
             "launch each); %d rounds x %d calls, alternating in one process, us per call (HIP events)"
             % (len(ts), n / 1e6, 4 * n / 1e6, len(launches), rounds, reps)]
    for k, v in rows.items():
        best = min(v)
        lines.append("  %-32s %s   min %.2f us = %.0f GB/s at 4 B / element" % (k, "  ".join("%.2f" % x for x in v), best, 4 * n / best / 1e3))
    a, b, d = (min(rows[k]) for k in ("grad_sumsq (csrc/adam.hip)", "grad_sumsq, again", "digest_words (csrc/digest.hip)"))
    lines.append("  digest / grad_sumsq (min over rounds): %.3f and %.3f; grad_sumsq against itself: %.3f" % (d / a, d / b, max(a, b) / min(a, b)))
    text = "\n".join(lines)
    print(text, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(text + "\n")


def step(steps, every, out):
    import torch
    lines = []
    for check in (0, every):
        tr, inputs = _trainer(True, check)
        for _ in range(5):
            tr.train_step(dict(inputs))
        torch.cuda.synchronize()
        best = []
        for _ in range(3):
            tr._weight_checks, t0 = 0, time.perf_counter()
            for k in range(steps):
                tr.train_step(dict(inputs))
                if check and (k + 1) % check == 0:
                    tr.check_weights()
            torch.cuda.synchronize()
            best.append(1e3 * (time.perf_counter() - t0) / steps)
        assert tr._graphed is not None
        lines.append("captured step, --check_weights %d: ms per step over 3 x %d replays: %s   (%d checks per %d replays)" % (
            check, steps, "  ".join("%.3f" % b for b in best), tr._weight_checks, steps))
        print(lines[-1], flush=True)
        del tr
        torch.cuda.empty_cache()
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["kernels", "step"], required=True)
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--every", type=int, default=100)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    if a.what == "kernels":
        kernels(a.reps, a.rounds, a.out)
    else:
        step(a.steps, a.every, a.out)
