"""Eigen-split evaluation of a checkpoint's weight average: model_test.py's protocol and command line, reading
`ema_encoder<N>.pt` / `ema_decoder<N>.pt` (model_tool/logger.py: save writes them under the live files' keys, so
model_test.load_weights reads them as they are) when --ema_decay > 0 and both exist, the live files otherwise.

    python model_ema_eval.py --save NAME --epoch N --ema_decay 0.999
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def checkpoint_files(save, epoch, ema_decay=0.0):
    """(encoder file, decoder file, averaged?) of epoch `epoch` under the directory `save`."""
    live = tuple(os.path.join(save, "%s%d.pt" % (k, epoch)) for k in ("encoder", "decoder"))
    ema = tuple(os.path.join(save, "ema_%s%d.pt" % (k, epoch)) for k in ("encoder", "decoder"))
    if float(ema_decay or 0.0) > 0 and all(os.path.isfile(f) for f in ema):
        return ema + (True,)
    return live + (False,)


if __name__ == "__main__":
    from model_option import options
    from model_test import METRICS, inference
    o = options()
    enc, dec, averaged = checkpoint_files(os.path.join("./model_save", o.save), o.epoch, getattr(o, "ema_decay", 0.0))
    print("evaluating the %s: %s, %s" % ("weight EMA" if averaged else "live weights", enc, dec))
    res = inference(o, weights=(enc, dec) if os.path.isfile(enc) else None)
    print(("{:>9}" * 7).format(*METRICS))
    print(("{:9.3f}" * 7).format(*[res[k] for k in METRICS]))
