"""CPU: the per-tensor gradient and weight statistics (mdx.optim.GradStats, csrc/tensor_stats.hip).  (1) The six entry points are
declared by include/mdx.h, exported by the built library, and the two structs as gcc lays them out are the ctypes structures
mdx/optim.py fills.  (2) Bad arguments are refused with status codes before any HIP call (no kernel is launched, no GPU needed).
(3) On CPU tensors the records come from torch's own functions and are held to the reference of tests/gradstats_cases.py, field by
field.  (4) The history over six passes.  (5) The trainer's option, its epoch lines and grad_stats.jsonl."""
import ctypes as C
import importlib
import json
import os
import re
import subprocess

import pytest
import torch

PKG = "digging-into-self-supervised-monocular-depth-estimation_amd"
importlib.import_module(PKG)
import gradstats_cases as cases  # noqa: E402
from mdx import _lib  # noqa: E402
from mdx.optim import GradStats, TensorStats, TensorStatsHistory, _StatsTable  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, Z = C.c_void_p, C.c_int, C.c_size_t
PROTOS = {
    "mdx_tensor_stats_table_entry_bytes": (Z, []),
    "mdx_tensor_stats_partial_bytes": (Z, []),
    "mdx_tensor_stats_record_bytes": (Z, []),
    "mdx_tensor_stats_history_bytes": (Z, []),
    # table, first, count, grads, blockmap, nblocks, partials, stream
    "mdx_tensor_stats_partials": (I, [P, I, I, P, P, I, P, P]),
    # first, count, offsets, partials, records, history, stream
    "mdx_tensor_stats_finish": (I, [I, I, P, P, P, P, P]),
}
FAKE = C.c_void_p(4096)          # a non-null, aligned address that is never dereferenced on these paths
ODD = C.c_void_p(4096 + 4)       # 4-byte but not 8-byte aligned
NULL, SHAPE, MISALIGNED = -2, -1, -6
SIZES = (1, 17, 4095, 4096, 4097, 12289)


# ---- (1) the ABI ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PROTOS))
def test_header_declares_and_library_exports_the_entry(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdx.h")).read(), flags=re.S)
    assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, text), name
    assert _lib.signatures()[name] == PROTOS[name]
    assert hasattr(C.CDLL(_lib.LIB_PATH), name)
    fn = getattr(_lib.lib(), name)
    assert fn.restype is PROTOS[name][0] and list(fn.argtypes) == PROTOS[name][1]


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof, and offsetof / sizeof of every field, of the two structs as the host C compiler lays them out == the ctypes
    structures (the technique of tests/test_abi.py)."""
    want, code = [], []
    for name, t in (("mdx_tensor_stats", TensorStats), ("mdx_tensor_stats_history", TensorStatsHistory)):
        want.append("%s %d" % (name, C.sizeof(t)))
        code.append('printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        for f, _ in t._fields_:
            want.append("%s.%s %d %d" % (name, f, getattr(t, f).offset, getattr(t, f).size))
            code.append('printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (name, f, name, f, name, f))
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "mdx.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(code))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    assert subprocess.check_output([exe], text=True).splitlines() == want
    assert [f for f, _ in TensorStats._fields_] == ["grad_sumsq", "weight_sumsq", "grad_absmax", "weight_absmax", "grad_nonfinite",
                                                    "weight_nonfinite", "grad_zeros", "grad_present"]
    assert [f for f, _ in TensorStatsHistory._fields_] == ["passes", "bad_passes", "first_bad_pass", "last_bad_pass",
                                                           "first_bad_weight_pass", "max_grad_sumsq", "max_grad_pass"]


def test_sizes_agree_with_the_python_structs():
    lib = _lib.lib()
    assert lib.mdx_version() == 510 == _lib.DEFINES["VERSION"]
    assert lib.mdx_tensor_stats_table_entry_bytes() == 16 == C.sizeof(_StatsTable)
    assert lib.mdx_tensor_stats_record_bytes() == 40 == C.sizeof(TensorStats) == lib.mdx_tensor_stats_partial_bytes()
    assert lib.mdx_tensor_stats_history_bytes() == 56 == C.sizeof(TensorStatsHistory)
    assert lib.mdx_adam_chunk() == 4096 and lib.mdx_adam_max_tensors() == 384           # the block-map recipe it shares
    assert (lib.mdx_digest_table_entry_bytes(), lib.mdx_ema_table_entry_bytes(), lib.mdx_adam_table_entry_bytes()) == (16, 24, 40)


# ---- (2) refusals ----------------------------------------------------------------------------------------------------------------
def _partials(table=FAKE, first=0, count=2, grads=FAKE, blockmap=FAKE, nblocks=3, partials=FAKE):
    return _lib.lib().mdx_tensor_stats_partials(table, first, count, grads, blockmap, nblocks, partials, None)


def _finish(first=0, count=2, offsets=FAKE, partials=FAKE, records=FAKE, history=FAKE):
    return _lib.lib().mdx_tensor_stats_finish(first, count, offsets, partials, records, history, None)


@pytest.mark.parametrize("missing", ["table", "grads", "blockmap", "partials"])
def test_partials_refuses_null_pointers(missing):
    assert _partials(**{missing: None}) == NULL


@pytest.mark.parametrize("missing", ["offsets", "partials", "records"])
def test_finish_refuses_null_pointers(missing):
    assert _finish(**{missing: None}) == NULL


BAD = [dict(first=-1), dict(count=0), dict(count=-2), dict(count=385)]


@pytest.mark.parametrize("bad", BAD + [dict(nblocks=0), dict(nblocks=-1)], ids=lambda d: "%s=%d" % next(iter(d.items())))
def test_partials_refuses_bad_counts(bad):
    assert _partials(**bad) == SHAPE


@pytest.mark.parametrize("bad", BAD, ids=lambda d: "%s=%d" % next(iter(d.items())))
def test_finish_refuses_bad_counts(bad):
    assert _finish(**bad) == SHAPE


def test_misaligned_buffers_are_refused():
    assert _partials(partials=ODD) == MISALIGNED
    for which in ("partials", "records", "history"):
        assert _finish(**{which: ODD}) == MISALIGNED, which
    # the order of the refusals: a NULL before a shape, a shape before an alignment
    assert _partials(partials=ODD, count=0) == SHAPE and _partials(partials=ODD, table=None) == NULL
    assert _finish(records=ODD, count=0) == SHAPE and _finish(records=ODD, offsets=None) == NULL


# ---- (3) the torch path on CPU tensors ---------------------------------------------------------------------------------------
def _cpu_set(seed=0):
    """Weights and gradients of SIZES and one channels-last 4-D tensor, the special values in both; the gradient of n = 17 is None."""
    gen = torch.Generator().manual_seed(seed)
    shapes = [(n,) for n in SIZES] + [(6, 5, 3, 3)]
    ws, gs = [], []
    for s in shapes:
        w, g = torch.randn(*s, generator=gen), torch.randn(*s, generator=gen)
        if len(s) == 4:
            w, g = w.contiguous(memory_format=torch.channels_last), g.contiguous(memory_format=torch.channels_last)
        ws.append(cases.put_specials(w).requires_grad_(True))
        gs.append(cases.put_specials(g.mul_(3.0)))
    gs[1] = None
    return ws, gs


def test_cpu_tensors_follow_the_reference():
    ws, gs = _cpu_set()
    stats = GradStats(ws)
    assert stats._native is False and stats.names == [str(i) for i in range(len(ws))]
    out = stats.compute(gs)
    assert out is stats._records and not out.is_cuda and stats._last_native is False
    worst = cases.check(stats, ws, gs)
    print("largest relative error of a sum of squares: %.3g" % worst)
    host = stats.host()
    assert host["1"]["grad_present"] == 0 and host["1"]["grad_norm"] == 0.0 and host["1"]["grad_zeros"] == 0
    assert host["0"]["weight_nonfinite"] == 1 and host["0"]["weight_absmax"] == 0.0        # n = 1: the one element is a NaN
    assert host["4"]["grad_nonfinite"] >= 5 and host["4"]["grad_zeros"] >= 2
    assert not ws[-1].is_contiguous() and host[str(len(ws) - 1)]["numel"] == 6 * 5 * 3 * 3
    # the default gradients are the parameters' .grad
    for w, g in zip(ws, gs):
        w.grad = g
    first = out.clone()
    assert stats.compute() is out and torch.equal(out, first)
    assert stats.history()["1"]["passes"] == 2


def test_finite_classification_is_by_the_exponent_bits():
    """The largest finite float, the smallest denormal and 1e30 (whose float32 square overflows) are finite; both infinities and
    NaNs of either sign are not; only +0 and -0 are zeros."""
    w = torch.ones(8, requires_grad=True)
    g = torch.tensor([3.4028234663852886e38, 1e30, 0.0, -0.0, 1.0, 1.0, 1.0, 1.0])
    bits = g.view(torch.int32)
    bits[4], bits[5], bits[6], bits[7] = cases.DENORMAL, cases.NAN_A, cases.NAN_B, cases.NEG_INF
    stats = GradStats([w], ["t"])
    stats.compute([g])
    cases.check(stats, [w], [g])
    r = stats.host()["t"]
    assert (r["grad_nonfinite"], r["grad_zeros"], r["grad_absmax"]) == (3, 2, 3.4028234663852886e38)
    assert r["grad_norm"] > 3.4e38 and r["grad_norm"] < float("inf")


def test_what_is_refused():
    with pytest.raises(ValueError):
        GradStats([])
    with pytest.raises(ValueError):
        GradStats([torch.zeros(3), torch.zeros(3)], names=["a", "a"])
    stats = GradStats([torch.zeros(3)])
    with pytest.raises(ValueError):
        stats.compute([None, None])


# ---- (4) the history ------------------------------------------------------------------------------------------------------------
def test_history_over_six_passes_on_the_cpu():
    stats, norms3 = cases.run_history_sequence("cpu")
    assert stats._native is False
    cases.check_history(stats, norms3)


# ---- (5) the option and the trainer on the CPU (the set-up of tests/test_digest_abi.py) ---------------------------------------------
ARGS = ["--dataset", "synthetic", "--height", "64", "--width", "96", "--batch", "2", "--epoch", "2", "--max_steps", "2",
        "--num_workers", "0", "--synthetic_length", "8", "--weight_init", "0"]


def test_the_option_parses():
    import model_option
    assert model_option.options([]).grad_stats == 0
    assert model_option.options(["--grad_stats", "25"]).grad_stats == 25


def _run(save, *more):
    import model_option
    from model_train import trainer
    torch.manual_seed(0)
    tr = trainer(model_option.options(ARGS + ["--save", save] + list(more)))
    assert tr.device == "cpu"
    tr.train()
    return tr


def test_without_the_option_nothing_is_built_said_or_written(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    tr = _run("plain", "--epoch", "1")
    assert "grad_stats" not in tr.setting.optim and tr._grad_stat_passes == 0 and tr._grad_stat_steps == {}
    assert "grad stats" not in capsys.readouterr().out
    assert not os.path.exists(tmp_path / "model_save" / "plain" / "grad_stats.jsonl")


def test_the_trainer_reports_once_per_epoch_and_writes_the_file(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    tr = _run("stats", "--grad_stats", "1")
    stats = tr.setting.optim["grad_stats"]
    names = ["%s.%s" % (key, n) for key, net in tr.setting.raw_model.items() for n, p in net.named_parameters() if p.requires_grad]
    assert stats.names == names and len(names) > 100 and [p.data_ptr() for p in stats.params] == [p.data_ptr() for p in tr.setting.parameters]
    # four passes; after a report the trainer keeps the steps of the passes the history points at and of the last one only
    assert tr._grad_stat_passes == 4 and tr._grad_stat_torch == 0 and tr._grad_stat_steps[4] == 4
    assert set(tr._grad_stat_steps) == {h["max_grad_pass"] for h in stats.history().values()} - {0} | {4}
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("grad stats:")]
    assert len(lines) == 2, lines                           # one per epoch: no tensor went bad, so no second or third line
    for line, passes in zip(lines, (2, 4)):
        m = re.match(r"grad stats: %d passes, last gradient norm (\S+), largest (\S+) (\S+), smallest (\S+) (\S+)$" % passes, line)
        assert m and m.group(2) in names and m.group(4) in names and float(m.group(1)) >= float(m.group(3)) >= float(m.group(5)) >= 0
    rows = [json.loads(l) for l in open(tmp_path / "model_save" / "stats" / "grad_stats.jsonl")]
    assert [r["epoch"] for r in rows] == [1, 2] and [r["passes"] for r in rows] == [2, 4] and [r["last_step"] for r in rows] == [2, 4]
    for r in rows:
        assert list(r["records"]) == names and list(r["history"]) == names
    last = rows[-1]
    assert all(h["passes"] == 4 and h["bad_passes"] == 0 and h["first_bad_step"] is None for h in last["history"].values())
    assert all(h["max_grad_step"] == (h["max_grad_pass"] or None) for h in last["history"].values()) and last["torch_passes"] == 0
    now = stats.host()
    assert all(last["records"][n] == now[n] for n in names)
    # the records are those of the gradients the last step left in .grad
    cases.check(stats, [p for p in stats.params], [p.grad for p in stats.params])
    assert last["total_norm"] == stats.total_norm() > 0
