#!/usr/bin/env python3
"""Cost of the loss-path statistics (mdx/loss_stats.py: LossStats, csrc/loss_stats.hip) at configs[1] (192x640, batch 12, four
scales, S = 2 with the auto-mask): four uint8 index maps [12,192,640] (5.9 MB) and the four disparities (7.8 MB).

    python tools/lossstats_cost.py --what kernels [--out profiles/r11_lossstats_cost.txt]
        one process, HIP events around REPS calls, ROUNDS rounds alternating:
          a torch formulation                              per scale and image torch.bincount of the index map, and per scale
                                                           isfinite, amin / amax over the finite elements and float64 sums of the
                                                           disparity: the same numbers by ATen's kernels, without a history
          LossStats.compute()                              the pass: its host half and two launches
          mdx_loss_stats_partials + mdx_loss_stats_finish  the two launches alone, over the pointer arrays as compute() left them
          mdx_loss_stats_partials / mdx_loss_stats_finish  each launch on its own
        Time per pass and GB/s over the 13.7 MB the pass reads; a loop re-reads them, so they stay inside the Infinity Cache and the
        rate is no fraction of the HBM peak.
    python tools/lossstats_cost.py --what step [--every 1]
        the captured training step (model_train.graphed_step) with --loss_stats 0 and --loss_stats EVERY, the passes issued as
        trainer.train issues them: host clock around N replays, the passes between them
"""
import argparse
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
    opt.graph, opt.loss_stats = graph, every
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
    outputs = tr.train_step(dict(inputs))                   # one eager step: its maps are the workload
    scales = tr.opt.scales
    idx = [outputs[("automask", s)] for s in scales]
    disp = [outputs[("disp", s)].detach() for s in scales]
    stats = tr.setting.optim["loss_stats"]
    stats.compute(idx, disp)
    assert stats._last_native
    n, B = len(scales), stats.B
    nbytes = sum(i.numel() for i in idx) + 4 * sum(d.numel() for d in disp)
    shape = (n, B, stats.H, stats.W, stats.S, int(stats.automask), stats._h, stats._w)

    def partials():
        api.mdx_loss_stats_partials(*shape, stats._idx, stats._disp, stats._blockmap.data_ptr(), stats.nblocks,
                                    stats._partials.data_ptr(), stream())

    def finish():
        api.mdx_loss_stats_finish(*shape, stats.static_share, stats._partials.data_ptr(), stats._records.data_ptr(),
                                  stats._history.data_ptr(), stream())

    def two_launches():
        partials()
        finish()

    def torch_way():
        res = []
        for i, d in zip(idx, disp):
            flat = i.view(B, -1)
            res.append([torch.bincount(flat[b], minlength=8) for b in range(B)])
            x = d.view(B, -1)
            finite = torch.isfinite(x)
            kept = x.double()
            zero = torch.zeros((), dtype=torch.float64, device=x.device)
            res.append((torch.where(finite, kept, zero).sum(1), torch.where(finite, kept * kept, zero).sum(1),
                        torch.where(finite, x, torch.full_like(x, float("inf"))).amin(1),
                        torch.where(finite, x, torch.full_like(x, float("-inf"))).amax(1), (~finite).sum(1)))
        return res

    calls = [("torch: bincount, isfinite, amin/amax", torch_way), ("LossStats.compute()", lambda: stats.compute(idx, disp)),
             ("its two launches alone", two_launches), ("mdx_loss_stats_partials alone", partials), ("mdx_loss_stats_finish alone", finish),
             ("torch, again", torch_way)]
    for _, fn in calls:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    rows = {k: [] for k, _ in calls}
    for _ in range(rounds):
        for k, fn in calls:
            rows[k].append(_time(fn, reps if "torch" not in k else max(reps // 10, 5)))
    lines = ["tools/lossstats_cost.py --what kernels: %d scales x %d images, %d x %d, S = %d, automask %d; %.2f MB of index maps + %.2f MB "
             "of disparities, %d blocks in pass 1; %d rounds x %d calls (the torch rows: %d), alternating in one process, us per call "
             "(HIP events)" % (n, B, stats.H, stats.W, stats.S, stats.automask, sum(i.numel() for i in idx) / 1e6,
                               4 * sum(d.numel() for d in disp) / 1e6, stats.nblocks, rounds, reps, max(reps // 10, 5))]
    for k, v in rows.items():
        best = min(v)
        lines.append("  %-40s %s   min %.2f us = %.0f GB/s over %.1f MB" % (k, "  ".join("%.2f" % x for x in v), best, nbytes / best / 1e3,
                                                                           nbytes / 1e6))
    t, p, k2 = (min(rows[k]) for k in ("torch: bincount, isfinite, amin/amax", "LossStats.compute()", "its two launches alone"))
    lines.append("  pass / torch formulation (min over rounds): %.4f; host half of compute(): %.2f us" % (p / t, p - k2))
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
        outputs = None
        for _ in range(5):
            outputs = tr.train_step(dict(inputs))
        torch.cuda.synchronize()
        best = []
        for _ in range(3):
            before, t0 = tr._loss_stat_total, time.perf_counter()
            for k in range(steps):
                outputs = tr.train_step(dict(inputs))
                if stats and (k + 1) % stats == 0:
                    tr.loss_stats(outputs, k + 1)
            torch.cuda.synchronize()
            best.append(1e3 * (time.perf_counter() - t0) / steps)
        assert tr._graphed is not None
        lines.append("captured step, --loss_stats %d: ms per step over 3 x %d replays: %s   (%d passes per %d replays)" % (
            stats, steps, "  ".join("%.3f" % b for b in best), tr._loss_stat_total - before, steps))
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
    ap.add_argument("--every", type=int, default=1)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    if a.what == "kernels":
        kernels(a.reps, a.rounds, a.out)
    else:
        step(a.steps, a.every, a.out)
