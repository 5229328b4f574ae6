#!/usr/bin/env python3
"""Cost of the weight average (mdx/optim.py: WeightEMA, csrc/ema.hip) on the trainer at configs[1] (ResNet-18, 192x640, batch 12,
fp32): its own tensor list -- every trained parameter and batch-norm statistic of the four networks.

    python tools/ema_cost.py --what kernels [--out profiles/r08_ema_cost.txt]
        one process, HIP events around REPS calls, ROUNDS rounds alternating: the update (ema_update_kernel launches + the tick)
        against torch._foreach_lerp_ over the same tensors with the same weight -- what a user would otherwise write, and what a
        capture would freeze the decay schedule of --, then the swap.  The update's achieved bytes per second against the
        12 B / element it has to move (read live, read shadow, write shadow); the swap's against 16 B / element.
    python tools/ema_cost.py --what step
        the captured training step (model_train.graphed_step), --ema_decay 0 against 0.999: host clock around N replays
"""
import argparse
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _trainer(graph, decay):
    import torch
    bench = importlib.import_module("bench")
    importlib.import_module("digging-into-self-supervised-monocular-depth-estimation_amd")
    from model_train import trainer
    torch.manual_seed(0)
    opt = bench.make_opt(12)
    opt.graph, opt.ema_decay = graph, decay
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
    tr, _ = _trainer(False, 0.999)
    ema = tr.setting.optim["ema"]
    live, shadow = [t.detach() for t in ema.live], ema.shadow
    n = sum(t.numel() for t in live)
    ema.load_state_dict(dict(ema.state_dict(), updates=10 ** 6))            # past the warm-up: w = 1 - 0.999
    w = ema._weight(10 ** 6)
    with torch.no_grad():
        for t in live:                                                       # live != shadow, as after a step
            t.add_(1e-3)
    other = [e.clone() for e in shadow]                                      # _foreach_lerp_'s own shadows: same sizes and strides
    calls = {"update (csrc/ema.hip)": ema.update, "torch._foreach_lerp_": lambda: torch._foreach_lerp_(other, live, w), "swap": ema.swap}
    for fn in calls.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    rows = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            rows[k].append(_time(fn, reps))
    if (5 + rounds * reps) % 2:                     # an odd number of swaps so far: put the weights back
        ema.swap()
    lines = ["tools/ema_cost.py --what kernels: %d tensors, %.2f M elements (%.1f MB), %d launches per update + the tick; %d rounds x %d calls, "
             "alternating in one process, us per call (HIP events)" % (len(live), n / 1e6, 4 * n / 1e6, len(ema._launches), rounds, reps)]
    for k, v in rows.items():
        per = {"swap": 16}.get(k, 12)
        best = min(v)
        lines.append("  %-24s %s   min %.2f us = %.2f TB/s at %d B / element" % (k, "  ".join("%.2f" % x for x in v), best, per * n / best / 1e6, per))
    ratio = min(rows["update (csrc/ema.hip)"]) / min(rows["torch._foreach_lerp_"])
    lines.append("  update / _foreach_lerp_ (min over rounds): %.3f" % ratio)
    text = "\n".join(lines)
    print(text, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(text + "\n")


def step(steps, out):
    import torch
    lines = []
    for decay in (0.0, 0.999):
        tr, inputs = _trainer(True, decay)
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
        ema = tr.setting.optim.get("ema")
        lines.append("captured step, --ema_decay %g: ms per step over 3 x %d replays: %s%s" % (
            decay, steps, "  ".join("%.3f" % b for b in best), "   %s" % ema.stats() if ema is not None else ""))
        print(lines[-1], flush=True)
        del tr
        torch.cuda.empty_cache()
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["kernels", "step"], required=True)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    if a.what == "kernels":
        kernels(a.reps, a.rounds, a.out)
    else:
        step(a.steps, a.out)
