#!/usr/bin/env python3
"""Time of a VALIDATION step (torch.no_grad(), networks in eval mode; model_train.py:75-79 of the reference) on bench.py's own batch,
three ways in one process: eager with the batch norms as torch ops (BatchNorm2d.fused_eval = False), eager with the fused eval
kernel (csrc/norm_infer.hip), and captured into a hipGraph (model_train.graphed_valid_step).  Host clock around N steps that end
in a device synchronise.

    python tools/valid_step_probe.py              # configs[1] (ResNet-18, 192x640, batch 12): fp32, then bf16
    python tools/valid_step_probe.py --config 3   # configs[3] (ResNet-50, 320x1024, batch 8), bf16
"""
import argparse
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

bench = importlib.import_module("bench")
importlib.import_module("digging-into-self-supervised-monocular-depth-estimation_amd")
from model_layer.depth_encoder import BatchNorm2d  # noqa: E402
from model_train import trainer  # noqa: E402


def timed(fn, steps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def probe(name, opt, steps):
    opt.graph, opt.graph_valid = True, True
    tr = trainer(opt)
    tr.setting.set_train()
    inputs = bench.one_batch(tr.setting, tr.device)
    for _ in range(3):                   # a few training steps first: the disparities of a net that has moved off its init
        tr._eager_step(dict(inputs))
    tr.setting.set_valid()
    res = {}
    with torch.no_grad():
        BatchNorm2d.fused_eval = False
        res["eager, torch-op batch norm"] = timed(lambda: tr.batch_process(dict(inputs)), steps)
        BatchNorm2d.fused_eval = True
        res["eager, fused eval batch norm"] = timed(lambda: tr.batch_process(dict(inputs)), steps)
        res["captured"] = timed(lambda: tr.valid_step(dict(inputs)), steps)
    assert tr._graphed_valid is not None and tr._graphed_valid.replays > 0
    print("%s: validation step ms  %s" % (name, "  ".join("%s %.2f" % kv for kv in res.items())), flush=True)
    del tr
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=1, choices=[1, 3])
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    if a.config == 1:
        probe("configs[1] fp32 ResNet-18 192x640 batch 12", bench.make_opt(12), a.steps)
        probe("configs[1] bf16 ResNet-18 192x640 batch 12", bench.make_opt(12, amp="bf16"), a.steps)
    else:
        probe("configs[3] bf16 ResNet-50 320x1024 batch 8", bench.make_opt(8, 320, 1024, num_layers=50, amp="bf16"), a.steps)


if __name__ == "__main__":
    main()
