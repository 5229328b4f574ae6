"""CPU: the weight average (mdx.optim.WeightEMA, csrc/ema.hip).  (1) Its entry points are declared by include/mdx.h with the documented
prototypes, exported by the built library, and refuse bad arguments with status codes before any HIP call (no kernel is launched, no
GPU needed).  (2) On CPU tensors the average runs through torch's own functions with a host counter: the float64 formula, the swap,
the state round trip, the resume from a checkpoint without an average.  (3) The trainer's options."""
import ctypes as C
import importlib
import os
import re

import pytest
import torch

PKG = "digging-into-self-supervised-monocular-depth-estimation_amd"
importlib.import_module(PKG)
from mdx import _lib  # noqa: E402
from mdx.optim import Adam, WeightEMA, _EmaTable  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, D, Z = C.c_void_p, C.c_int, C.c_double, C.c_size_t
PROTOS = {
    "mdx_ema_table_entry_bytes": (Z, []),
    "mdx_ema_record_bytes": (Z, []),
    # table, first, count, blockmap, nblocks, decay, warmup, record, guard_record, stream
    "mdx_ema_update": (I, [P, I, I, P, I, D, I, P, P, P]),
    # record, guard_record, stream
    "mdx_ema_tick": (I, [P, P, P]),
    # table, first, count, blockmap, nblocks, stream
    "mdx_ema_swap": (I, [P, I, I, P, I, P]),
}
FAKE = C.c_void_p(4096)          # a non-null, aligned address that is never dereferenced on these paths
ODD = C.c_void_p(4096 + 4)       # 4-byte but not 8-byte aligned
NULL, SHAPE, MISALIGNED = -2, -1, -6


@pytest.mark.parametrize("name", sorted(PROTOS))
def test_header_declares_the_prototype(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdx.h")).read(), flags=re.S)
    assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, text), name
    assert _lib.signatures()[name] == PROTOS[name]


@pytest.mark.parametrize("name", sorted(PROTOS))
def test_built_library_exports_the_entry(name):
    raw = C.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, name)
    fn = getattr(_lib.lib(), name)
    assert fn.restype is PROTOS[name][0] and list(fn.argtypes) == PROTOS[name][1]


def test_sizes_agree_with_the_python_structs():
    lib = _lib.lib()
    assert lib.mdx_version() == 510 == _lib.DEFINES["VERSION"]
    assert lib.mdx_ema_table_entry_bytes() == 24 == C.sizeof(_EmaTable)          # {float *live, *shadow; int64 numel}
    assert [f[0] for f in _EmaTable._fields_] == ["p", "e", "n"]
    assert lib.mdx_ema_record_bytes() == 16 == torch.zeros(2, dtype=torch.int64).numel() * 8     # {int64 updates, held}
    assert lib.mdx_adam_table_entry_bytes() == 40 and lib.mdx_adam_guard_record_bytes() == 32    # the neighbours stay


def _struct_fields(source, name):
    """[(type, field), ...] of `struct name { ... };` in csrc/<source>, in declaration order ("float a, b;" gives two)."""
    text = open(os.path.join(ROOT, PKG, "csrc", source)).read()
    body = re.search(r"\bstruct\s+%s\s*\{(.*?)\};" % name, text, flags=re.S).group(1)
    body = re.sub(r"//[^\n]*|/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        parts = decl.split(",")
        kind, first = parts[0].rsplit(None, 1)
        out += [(" ".join(kind.split()), n.strip()) for n in [first] + parts[1:]]
    return out


def test_the_guard_record_is_read_as_adam_writes_it():
    """adam.hip writes the guard's record and ema.hip reads `skipped` from it through ONE declaration (csrc/mdx_multi_tensor.hpp),
    which Python restates as a ctypes structure: the two agree field by field and offset by offset, so a reordering over there
    fails here, not on the GPU."""
    from mdx.optim import GuardRecord
    theirs = _struct_fields("mdx_multi_tensor.hpp", "GuardRecord")
    assert theirs == [("float", "total_norm"), ("float", "coef"), ("int", "skipped"), ("int", "reserved"),
                      ("long long", "steps"), ("long long", "skipped_steps")]
    ctype = {"float": C.c_float, "int": C.c_int, "long long": C.c_int64}
    assert C.sizeof(C.c_longlong) == 8
    assert [(ctype[kind], name) for kind, name in theirs] == [(t, n) for n, t in GuardRecord._fields_]      # names, order, types
    offset = 0
    for kind, name in theirs:                               # every field naturally aligned: the C layout has no padding
        assert getattr(GuardRecord, name).offset == offset and offset % C.sizeof(ctype[kind]) == 0, name
        offset += C.sizeof(ctype[kind])
    assert offset == C.sizeof(GuardRecord) == _lib.lib().mdx_adam_guard_record_bytes() == 32
    assert GuardRecord.skipped.offset == 8                  # include/mdx.h: skipped at byte 8
    for source in ("ema.hip", "adam.hip"):                  # no record struct of their own
        text = open(os.path.join(ROOT, PKG, "csrc", source)).read()
        assert not re.search(r"\bstruct\s+\w*GuardRecord\b", text) and '#include "mdx_multi_tensor.hpp"' in text, source


def _update(table=FAKE, first=0, count=2, blockmap=FAKE, nblocks=3, decay=0.999, warmup=1, record=FAKE, guard=None):
    return _lib.lib().mdx_ema_update(table, first, count, blockmap, nblocks, decay, warmup, record, guard, None)


def _swap(table=FAKE, first=0, count=2, blockmap=FAKE, nblocks=3):
    return _lib.lib().mdx_ema_swap(table, first, count, blockmap, nblocks, None)


@pytest.mark.parametrize("call, missing", [(_update, k) for k in ("table", "blockmap", "record")] + [(_swap, k) for k in ("table", "blockmap")],
                         ids=lambda v: v if isinstance(v, str) else v.__name__)
def test_null_pointers_are_refused(call, missing):
    assert call(**{missing: None}) == NULL


def test_tick_refuses_a_null_or_misaligned_record():
    lib = _lib.lib()
    assert lib.mdx_ema_tick(None, None, None) == NULL
    assert lib.mdx_ema_tick(ODD, None, None) == MISALIGNED
    assert lib.mdx_ema_tick(FAKE, ODD, None) == MISALIGNED


@pytest.mark.parametrize("call", [_update, _swap], ids=["update", "swap"])
@pytest.mark.parametrize("bad", [dict(first=-1), dict(count=0), dict(count=-2), dict(count=385), dict(nblocks=0), dict(nblocks=-1)],
                         ids=lambda d: "%s=%d" % next(iter(d.items())))
def test_bad_counts_are_refused(call, bad):
    assert _lib.lib().mdx_adam_max_tensors() == 384
    assert call(**bad) == SHAPE


@pytest.mark.parametrize("decay", [float("nan"), 1.0, 1.5, -1e-9, float("inf"), float("-inf")], ids=str)
def test_a_decay_outside_the_half_open_unit_interval_is_refused(decay):
    assert _update(decay=decay) == SHAPE


def test_a_misaligned_record_is_refused():
    assert _update(record=ODD) == MISALIGNED
    assert _update(guard=ODD) == MISALIGNED


# ---- the average through torch's own functions (CPU tensors) ---------------------------------------------------------------
class Net(torch.nn.Module):
    def __init__(self, seed):
        super().__init__()
        torch.manual_seed(seed)
        self.conv = torch.nn.Conv2d(3, 4, 3)
        self.bn = torch.nn.BatchNorm2d(4)                   # running_mean / running_var: averaged; num_batches_tracked: not
        self.frozen = torch.nn.Parameter(torch.randn(5), requires_grad=False)
        with torch.no_grad():
            self.bn.running_mean.normal_()
            self.bn.running_var.uniform_(0.5, 2.0)


def _move(nets, gen):
    with torch.no_grad():
        for net in nets:
            for t in list(net.parameters()) + [b for b in net.buffers() if b.dtype == torch.float32]:
                t.add_(0.1 * torch.randn(t.shape, generator=gen))


def test_what_is_covered():
    nets = [Net(0), Net(1)]
    ema = WeightEMA(nets, 0.9)
    assert ema.names == ["%d.%s" % (i, n) for i in (0, 1) for n in ("conv.weight", "conv.bias", "bn.weight", "bn.bias",
                                                                     "bn.running_mean", "bn.running_var")]
    assert all(e.dtype == torch.float32 and torch.equal(e, t) and e.data_ptr() != t.data_ptr() for e, t in zip(ema.shadow, ema.live))
    assert ema.stats() == dict(updates=0, held=0)
    for bad in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            WeightEMA(nets, bad)


@pytest.mark.parametrize("warmup", [True, False], ids=["warm-up", "constant"])
def test_cpu_path_follows_the_float64_formula(warmup):
    """20 updates against the float64 chain with w rounded to float32.  The bound per update is the rule's worst case of four
    float32 roundings, 2**-21 of the larger magnitude (tests/test_gpu_ema.py), added up over the updates so far."""
    import numpy as np
    nets = [Net(0), Net(1)]
    ema = WeightEMA(nets, 0.9, warmup=warmup)
    ref = [e.double().clone() for e in ema.shadow]
    big = [e.abs().double() for e in ema.shadow]
    gen = torch.Generator().manual_seed(3)
    for t in range(20):
        _move(nets, gen)
        ema.update()
        d = min(0.9, (1.0 + t) / (10.0 + t)) if warmup else 0.9
        w = float(np.float32(1.0 - d))
        for i, (r, live) in enumerate(zip(ref, ema.live)):
            p = live.detach().double()
            r.copy_(r + w * (p - r) if w < 0.5 else p - (p - r) * (1.0 - w))
            big[i] = torch.maximum(big[i], torch.maximum(p.abs(), r.abs()))
            assert bool(((ema.shadow[i].double() - r).abs() <= (t + 1) * 2.0 ** -21 * big[i]).all()), (t, ema.names[i])
    assert ema.stats() == dict(updates=20, held=0)
    if warmup:                                              # the first update's weight is 0.9: the shadow all but follows
        late = WeightEMA([Net(0)], 0.999)
        assert late._weight(0) == float(np.float32(0.9)) and late._weight(10 ** 6) == float(np.float32(1.0 - 0.999))


def test_the_host_guard_skip_withholds_the_update():
    net = Net(0)
    opt = Adam([p for p in net.parameters() if p.requires_grad], 1e-2, skip_nonfinite=True, fused=False)
    ema = WeightEMA([net], 0.5, warmup=False)
    gen = torch.Generator().manual_seed(1)
    for k, bad in enumerate((False, True, False)):
        for p in opt.param_groups[0]["params"]:
            p.grad = torch.randn(p.shape, generator=gen)
        if bad:
            net.conv.bias.grad[1] = float("nan")
        before = [e.clone() for e in ema.shadow]
        opt.step()
        ema.update(opt)
        changed = any(not torch.equal(a, b) for a, b in zip(before, ema.shadow))
        assert changed == (not bad), k
    assert ema.stats() == dict(updates=2, held=1)


def test_swap_and_applied_restore_on_exception():
    net = Net(0)
    ema = WeightEMA([net], 0.9)
    _move([net], torch.Generator().manual_seed(5))
    live = [t.detach().clone() for t in ema.live]
    shadow = [e.clone() for e in ema.shadow]
    assert not any(torch.equal(a, b) for a, b in zip(live, shadow))
    tracked = net.bn.num_batches_tracked.clone()
    with pytest.raises(RuntimeError, match="inside"):
        with ema.applied():
            for t, e, a, b in zip(ema.live, ema.shadow, live, shadow):
                assert torch.equal(t.view(torch.int32), b.view(torch.int32)) and torch.equal(e.view(torch.int32), a.view(torch.int32))
            assert torch.equal(net.state_dict()["conv.weight"], shadow[0])
            raise RuntimeError("inside")
    for t, e, a, b in zip(ema.live, ema.shadow, live, shadow):
        assert torch.equal(t.view(torch.int32), a.view(torch.int32)) and torch.equal(e.view(torch.int32), b.view(torch.int32))
    assert torch.equal(net.bn.num_batches_tracked, tracked) and net.conv.weight.requires_grad


def test_state_dict_round_trip_and_snapshot():
    nets = [Net(0), Net(1)]
    ema = WeightEMA(nets, 0.9)
    gen = torch.Generator().manual_seed(7)
    for _ in range(3):
        _move(nets, gen)
        ema.update()
    state = ema.state_dict()
    assert set(state) == {"shadow", "updates", "held"} and state["updates"] == 3 and state["held"] == 0
    assert sorted(state["shadow"]) == sorted(ema.names)
    snap = ema.snapshot()
    _move(nets, gen)
    ema.update()
    other = WeightEMA(nets, 0.9)
    other.load_state_dict(state)
    assert other.stats() == dict(updates=3, held=0)
    other.update()                                          # update t = 3 from the loaded shadows: the same bits
    assert all(torch.equal(a, b) for a, b in zip(other.shadow, ema.shadow)) and other.stats()["updates"] == 4
    ema.restore(snap)
    assert ema.stats() == dict(updates=3, held=0) and all(torch.equal(e, state["shadow"][n]) for n, e in zip(ema.names, ema.shadow))
    state["shadow"].pop(ema.names[0])
    with pytest.raises(KeyError):
        other.load_state_dict(state)


def _setting_and_control(tmp_path, monkeypatch, decay):
    from model_tool.logger import control

    class O(object):
        save, epoch = "ema", 2

    class S(object):
        pass
    monkeypatch.chdir(tmp_path)
    s = S()
    torch.manual_seed(0)
    s.raw_model = s.model = {"encoder": Net(0), "decoder": Net(1)}
    params = [p for m in s.model.values() for p in m.parameters() if p.requires_grad]
    s.optim = {"optimizer": torch.optim.Adam(params, 1e-3)}
    s.optim["scheduler"] = torch.optim.lr_scheduler.StepLR(s.optim["optimizer"], 15)
    if decay:
        s.optim["ema"] = WeightEMA(s.raw_model.values(), decay)
    return s, control(O(), "cpu")


def test_checkpoints_hold_the_average_and_resume_restores_it(tmp_path, monkeypatch, capsys):
    s, ctl = _setting_and_control(tmp_path, monkeypatch, 0.9)
    ema = s.optim["ema"]
    gen = torch.Generator().manual_seed(2)
    for _ in range(4):
        _move(s.model.values(), gen)
        ema.update()
    log = {k: [0.0, 0.0] for k in ctl.metric_name}
    live = {k: {n: v.clone() for n, v in m.state_dict().items()} for k, m in s.model.items()}
    ctl.save(1, log, log, s)
    d = tmp_path / "model_save" / "ema"
    for k, m in s.model.items():
        saved, avg = torch.load(d / (k + "2.pt")), torch.load(d / ("ema_" + k + "2.pt"))
        assert list(saved) == list(avg) == list(live[k])
        assert all(torch.equal(saved[n], live[k][n]) and torch.equal(m.state_dict()[n], live[k][n]) for n in saved)    # live: as before
        i = list(s.model).index(k)
        for n in avg:
            name = "%d.%s" % (i, n)
            want = ema.shadow[ema.names.index(name)] if name in ema.names else live[k][n]
            assert torch.equal(avg[n], want), (k, n)
    assert torch.load(d / "state2.pt")["ema"]["updates"] == 4
    # a fresh run resumes: weights and the average as saved
    s2, ctl2 = _setting_and_control(tmp_path, monkeypatch, 0.9)
    assert ctl2.resume(s2, 2) == 2
    assert s2.optim["ema"].stats() == dict(updates=4, held=0)
    assert all(torch.equal(a, b) for a, b in zip(s2.optim["ema"].shadow, ema.shadow))
    assert "holds no weight EMA" not in capsys.readouterr().out


def test_resume_from_a_checkpoint_without_an_average(tmp_path, monkeypatch, capsys):
    s, ctl = _setting_and_control(tmp_path, monkeypatch, 0.0)
    _move(s.model.values(), torch.Generator().manual_seed(2))
    log = {k: [0.0, 0.0] for k in ctl.metric_name}
    ctl.save(1, log, log, s)
    d = tmp_path / "model_save" / "ema"
    assert sorted(f.name for f in d.iterdir() if f.is_file()) == ["decoder2.pt", "encoder2.pt", "state2.pt"]      # decay 0: nothing more
    assert "ema" not in torch.load(d / "state2.pt")
    s2, ctl2 = _setting_and_control(tmp_path, monkeypatch, 0.9)
    s2.optim["ema"].update()                                # something to forget
    assert ctl2.resume(s2, 2) == 2
    ema = s2.optim["ema"]
    assert ema.stats() == dict(updates=0, held=0)
    assert all(torch.equal(e, t) for e, t in zip(ema.shadow, ema.live))
    assert all(torch.equal(a, b) for a, b in zip(s2.model["encoder"].state_dict().values(), s.model["encoder"].state_dict().values()))
    assert "holds no weight EMA; the average starts from the loaded weights with 0 updates" in capsys.readouterr().out


def test_loader_builds_the_average_only_when_asked():
    from model_tool.loader import setting

    class S(object):
        set_optim = setting.set_optim

    class O(object):
        learning_rate, scheduler_step = 1e-4, 15

    def build(**kw):
        s, o = S(), O()
        for k, v in kw.items():
            setattr(o, k, v)
        s.raw_model = {"encoder": Net(0), "decoder": Net(1)}
        s.opt, s.device, s.optim = o, "cpu", {}
        s.parameters = [p for m in s.raw_model.values() for p in m.parameters() if p.requires_grad]
        s.set_optim()
        return s.optim
    assert "ema" not in build() and "ema" not in build(ema_decay=0.0)
    ema = build(ema_decay=0.99, ema_warmup=0)["ema"]
    assert isinstance(ema, WeightEMA) and ema.decay == 0.99 and ema.warmup is False and len(ema.live) == 12
    assert build(ema_decay=0.5)["ema"].warmup is True


def test_shadow_storage_of_the_callers():
    nets = [Net(0), Net(1)]
    ema = WeightEMA(nets, 0.9)
    name = ema.names[0]
    arena = torch.full((ema.live[0].numel() + 2,), 7.0)
    mine = arena[1:-1].view_as(ema.live[0])
    other = WeightEMA(nets, 0.9, shadows={name: mine})
    assert other.shadow[0] is mine and torch.equal(mine, other.live[0]) and float(arena[0]) == float(arena[-1]) == 7.0
    assert all(e.data_ptr() != t.data_ptr() for e, t in zip(other.shadow, other.live))
    with pytest.raises(KeyError):
        WeightEMA(nets, 0.9, shadows={"no.such.tensor": mine})
    with pytest.raises(ValueError):
        WeightEMA(nets, 0.9, shadows={name: mine.double()})
    with pytest.raises(ValueError):
        WeightEMA(nets, 0.9, shadows={name: ema.live[0]})


def test_the_evaluation_script_picks_the_averaged_files(tmp_path):
    from model_ema_eval import checkpoint_files
    d = str(tmp_path)
    live = (os.path.join(d, "encoder3.pt"), os.path.join(d, "decoder3.pt"))
    ema = (os.path.join(d, "ema_encoder3.pt"), os.path.join(d, "ema_decoder3.pt"))
    assert checkpoint_files(d, 3, 0.999) == live + (False,)          # no averaged files: the live ones
    open(ema[0], "wb").close()
    assert checkpoint_files(d, 3, 0.999) == live + (False,)          # only one of the two: still the live ones
    open(ema[1], "wb").close()
    assert checkpoint_files(d, 3, 0.999) == ema + (True,)
    assert checkpoint_files(d, 3, 0.0) == live + (False,) and checkpoint_files(d, 3) == live + (False,)    # off: as before


def test_the_options_parse():
    import model_option
    opt = model_option.options(["--ema_decay", "0.999", "--ema_warmup", "0", "--ema_valid", "0"])
    assert opt.ema_decay == 0.999 and opt.ema_warmup == 0 and opt.ema_valid == 0
    opt = model_option.options([])
    assert opt.ema_decay == 0.0 and opt.ema_warmup == 1 and opt.ema_valid == 1
