#!/usr/bin/env python3
"""Cost of the per-tensor statistics (mdx/optim.py: GradStats, csrc/tensor_stats.hip) on the trainer at configs[1] (ResNet-18, 192x640,
batch 12, fp32): its own tensor list -- the trained float32 master parameters of the four networks and the gradients one step left.

    python tools/gradstats_cost.py --what kernels [--out profiles/r10_gradstats_cost.txt]
        one process, HIP events around REPS calls, ROUNDS rounds alternating:
          torch._foreach_norm(grads) then torch._foreach_norm(params)   ATen's way to the two norms alone: no maxima, no counts, no
                                                                        history, and float32 sums
          GradStats.compute()                                           the pass: its host half and two launches
          mdx_tensor_stats_partials + mdx_tensor_stats_finish           the two launches alone, over prebuilt pointer arrays: the
                                                                        kernels' own cost, as far as a loop of calls shows it
          mdx_adam_grad_sumsq over the gradients, then over the weights the family's own streaming rate for the same 8 bytes per
                                                                        element, over the SAME block map
        The bar: the pass is not slower than the two _foreach_norm calls.  The ratio against grad_sumsq is recorded without one.
        Time per pass and GB/s at 8 B / element; the loop re-reads 2 x 107 MB, which stay inside the Infinity Cache, so the rate is
        no fraction of the HBM peak.
    python tools/gradstats_cost.py --what step [--every 100]
        the captured training step (model_train.graphed_step) with --grad_stats 0 and --grad_stats EVERY, the passes issued as
        trainer.train issues them: host clock around N replays, the passes between them
"""
import argparse
import ctypes as C
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _trainer(graph, every):
    import torch
    bench = importlib.import_module("bench")
    importlib.import_module("digging-into-self-supervised-monocular-depth-estimation_amd")
    from model_train import trainer
    torch.manual_seed(0)
    opt = bench.make_opt(12)
    opt.graph, opt.grad_stats = graph, every
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
    tr, inputs = _trainer(False, 1)
    from mdx._lib import api, stream
    from mdx.optim import GradStats, _Table, _device_table, _launches
    tr.train_step(dict(inputs))                             # one eager step: .grad holds its gradients
    pairs = [(p.detach(), p.grad) for p in tr.setting.parameters if p.grad is not None]      # the same tensors in every column
    ws, gs = [w for w, _ in pairs], [g for _, g in pairs]
    n = sum(w.numel() for w in ws)
    stats = GradStats(ws)
    stats.compute(gs)
    assert stats._last_native
    table = _device_table(_Table, api.mdx_adam_table_entry_bytes(), ws, ws, ws, ws)      # grad_sumsq reads the table for numel only
    launches = _launches(ws, 0)
    partials = torch.empty(2 * sum(nb for _, _, _, nb in launches), dtype=torch.float64, device=ws[0].device)
    garrs = [[(C.c_void_p * count)(*[t.data_ptr() for t in ts[first:first + count]]) for first, count, _, _ in launches] for ts in (gs, ws)]

    def sumsq():
        slot = 0
        for arrs in garrs:
            for garr, (first, count, blockmap, nblocks) in zip(arrs, launches):
                api.mdx_adam_grad_sumsq(table.data_ptr(), first, count, garr, blockmap.data_ptr(), nblocks, partials.data_ptr() + 8 * slot, stream())
                slot += nblocks

    def foreach():
        torch._foreach_norm(gs)
        torch._foreach_norm(ws)

    def two_launches():
        """compute() without its host half (the dtype, device and stride checks of 156 gradients, 156 data_ptr() calls): the two
        launches over the pointer arrays as the last compute() filled them -- what grad_sumsq's column does with its prebuilt ones."""
        s, table, partials = stream(), stats._table.data_ptr(), stats._partials.data_ptr()
        for first, count, blockmap, nblocks, slot, garr in stats._launches:
            api.mdx_tensor_stats_partials(table, first, count, garr, blockmap.data_ptr(), nblocks, partials + 40 * slot, s)
        for first, count, _, _, _, _ in stats._launches:
            api.mdx_tensor_stats_finish(first, count, stats._offsets.data_ptr(), partials, stats._records.data_ptr(), stats._history.data_ptr(), s)

    calls = [("2 x _foreach_norm (ATen)", foreach), ("GradStats.compute()", lambda: stats.compute(gs)), ("its two launches alone", two_launches),
             ("2 x grad_sumsq (csrc/adam.hip)", sumsq), ("2 x _foreach_norm, again", foreach)]
    for _, fn in calls:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    rows = {k: [] for k, _ in calls}
    for _ in range(rounds):
        for k, fn in calls:
            rows[k].append(_time(fn, reps))
    lines = ["tools/gradstats_cost.py --what kernels: %d tensors, %.2f M elements (%.1f MB of gradients + as much of weights), %d launch(es) "
             "per half; %d rounds x %d calls, alternating in one process, us per call (HIP events)"
             % (len(ws), n / 1e6, 4 * n / 1e6, len(launches), rounds, reps)]
    for k, v in rows.items():
        best = min(v)
        lines.append("  %-32s %s   min %.2f us = %.0f GB/s at 8 B / element" % (k, "  ".join("%.2f" % x for x in v), best, 8 * n / best / 1e3))
    f1, f2, p, k, s = (min(rows[k]) for k in ("2 x _foreach_norm (ATen)", "2 x _foreach_norm, again", "GradStats.compute()",
                                              "its two launches alone", "2 x grad_sumsq (csrc/adam.hip)"))
    lines.append("  pass / _foreach_norm (min over rounds): %.3f and %.3f (the bar: <= 1); _foreach_norm against itself: %.3f; "
                 "pass / grad_sumsq: %.3f; the two launches alone / grad_sumsq: %.3f" % (p / f1, p / f2, max(f1, f2) / min(f1, f2), p / s, k / s))
    text = "\n".join(lines)
    print(text, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(text + "\n")


def step(steps, every, out):
    import torch
    lines = []
    for stats in (0, every):
        tr, inputs = _trainer(True, stats)
        for _ in range(5):
            tr.train_step(dict(inputs))
        torch.cuda.synchronize()
        best = []
        for _ in range(3):
            before, t0 = tr._grad_stat_passes, time.perf_counter()
            for k in range(steps):
                tr.train_step(dict(inputs))
                if stats and (k + 1) % stats == 0:
                    tr.grad_stats(k + 1)
            torch.cuda.synchronize()
            best.append(1e3 * (time.perf_counter() - t0) / steps)
        assert tr._graphed is not None
        lines.append("captured step, --grad_stats %d: ms per step over 3 x %d replays: %s   (%d passes per %d replays)" % (
            stats, steps, "  ".join("%.3f" % b for b in best), tr._grad_stat_passes - before, steps))
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
