"""GPU: the loss-path statistics (mdx.loss_stats.LossStats; csrc/loss_stats.hip: mdx_loss_stats_partials, mdx_loss_stats_finish).
Every record against the reference of tests/lossstats_cases.py -- counts, minima and maxima exactly, the two sums within
n * 2^-52 * sum(|term|) -- over shapes that meet every path of the kernels: one vector, image bases that are not 16-byte aligned, whole
chunks, a chunk and a tail, more than one block per image; S in {1, 2, 4} with and without the auto-mask; legal and illegal indices;
+-Inf, NaNs and denormals; pointers one element off; absent maps; buffers that start as 0xFF bytes; determinism; the history on the
device; capture and replay; no allocation; guard words; the trainer with --loss_stats in the eager and the captured form."""
import importlib
import math
import sys

import pytest
import torch

importlib.import_module("digging-into-self-supervised-monocular-depth-estimation_amd")
import lossstats_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

OUT_SENTINEL = 0x5A5A5A5A5A5A5A5A
COMBOS = [(1, True), (2, True), (4, True), (1, False), (2, False), (4, False)]


def _shapes():
    """(B, H, W, [(h, w)]): one 16-byte vector; 60 pixels, the bases of images 1 and 2 not 16-byte aligned; the golden size; exactly
    one chunk; one chunk and a 4-element tail; 2.5 chunks per image -- the edges from the library's own chunk sizes."""
    from mdx import _lib
    ci, cd = _lib.lib().mdx_loss_stats_index_chunk(), _lib.lib().mdx_loss_stats_disp_chunk()
    assert ci % 64 == 0 and cd % 64 == 0 and ci == cd
    return [(1, 4, 4, [(4, 4)]),
            (3, 6, 10, [(6, 10), (3, 5)]),
            (2, 24, 40, [(24, 40), (12, 20), (6, 10), (3, 5)]),
            (1, 64, ci // 64, [(64, cd // 64)]),
            (1, 4, ci // 4 + 1, [(4, cd // 4 + 1), (2, cd // 4)]),
            (2, 64, 5 * ci // 128, [(64, 5 * cd // 128), (32, 5 * cd // 256), (16, 5 * cd // 512), (8, 5 * cd // 1024)])]


SHAPE_IDS = ["one-vector", "unaligned-images", "golden", "one-chunk", "chunk-and-tail", "2.5-chunks"]


def _guarded(stats):
    """Put the records, the history and the partials each between two sentinel entries.  The records and the partials start as
    0xFF bytes -- nothing relies on a clear -- the history as zeros, its valid initial state."""
    bufs = []
    for attr, fill in (("_records", -1), ("_history", 0), ("_partials", -1)):
        old = getattr(stats, attr)
        buf = torch.full((old.shape[0] + 2, old.shape[1]), OUT_SENTINEL, dtype=torch.int64, device="cuda")
        buf[1:-1].fill_(fill)
        setattr(stats, attr, buf[1:-1])
        assert getattr(stats, attr).data_ptr() % 8 == 0 and getattr(stats, attr).is_contiguous()
        bufs.append(buf)
    return bufs


def _outputs_intact(bufs):
    return all(bool((b[0] == OUT_SENTINEL).all()) and bool((b[-1] == OUT_SENTINEL).all()) for b in bufs)


def _maps(B, H, W, hw, S, automask, seed, illegal=True):
    gen = torch.Generator().manual_seed(seed)
    idx = [cases.index_map(B, H, W, S, automask, gen, illegal) for _ in hw]
    disp = [cases.disparity(B, h, w, gen) for h, w in hw]
    return idx, disp


def _off_by_one(t, fill):
    """The tensor's values one element into a larger buffer: a uint8 map 1 byte, a float map 4 bytes off a 16-byte boundary."""
    buf = torch.full((t.numel() + 32,), fill, dtype=t.dtype, device="cuda")
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == t.element_size() and view.is_contiguous()
    return view, buf


def _new(B, H, W, hw, S, automask, **kw):
    from mdx.loss_stats import LossStats
    stats = LossStats(B, H, W, S, hw, automask, device="cuda", **kw)
    assert stats._native and stats._records.is_cuda
    return stats


# ---- 1. every shape, every S, with and without the auto-mask ----------------------------------------------------------------------
@pytest.mark.parametrize("S, automask", COMBOS)
@pytest.mark.parametrize("shape", range(6), ids=SHAPE_IDS)
def test_records_follow_the_reference(shape, S, automask):
    B, H, W, hw = _shapes()[shape]
    idx, disp = _maps(B, H, W, hw, S, automask, 10 * shape + S)
    stats = _new(B, H, W, hw, S, automask)
    outs = _guarded(stats)
    gi, gd = [i.cuda() for i in idx], [d.cuda() for d in disp]
    out = stats.compute(gi, gd)
    assert out is stats._records and out.is_cuda and stats._last_native
    want = cases.check(stats, idx, disp)
    assert all(r["bad_index"] >= 1 and r["disp_nonfinite"] >= 1 for r in want[0])
    assert _outputs_intact(outs)
    # read-only: the maps keep their bits (compared as words: the NaNs too)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(gi, idx))
    assert all(torch.equal(a.cpu().view(torch.int32), b.view(torch.int32)) for a, b in zip(gd, disp))
    # the same maps one element into a larger buffer: the scalar path, the same records
    aligned = out.clone()
    moved = [_off_by_one(t, 255) for t in gi] + [_off_by_one(t, float("nan")) for t in gd]
    again = stats.compute([m[0] for m in moved[:len(hw)]], [m[0] for m in moved[len(hw):]])
    assert stats._last_native and torch.equal(again, aligned) and _outputs_intact(outs)
    # and through torch's own functions on the host: one record, two implementations
    cpu = type(stats)(B, H, W, S, hw, automask, device="cpu")
    cpu.compute(idx, disp)
    for a, b in zip(sum(cases.records(stats), []), sum(cases.records(cpu), [])):
        assert (a.disp_min, a.disp_max, list(a.winner), a.bad_index, a.disp_nonfinite, a.index_present, a.disp_present) == \
               (b.disp_min, b.disp_max, list(b.winner), b.bad_index, b.disp_nonfinite, b.index_present, b.disp_present)
    assert [h["passes"] for h in stats.history()] == [2] * len(hw)


# ---- 2. the images the two failures look like --------------------------------------------------------------------------------------
def test_all_masked_none_masked_constant_and_no_finite_element():
    B, H, W, hw = 3, 6, 10, [(6, 10), (3, 5)]
    S = 2
    gen = torch.Generator().manual_seed(2)
    idx = cases.index_map(B, H, W, S, True, gen, illegal=False)
    idx[0] = torch.randint(0, S, (H, W), generator=gen).to(torch.uint8)              # every pixel masked
    idx[1] = torch.randint(S, 2 * S, (H, W), generator=gen).to(torch.uint8)          # none masked
    disp = [cases.disparity(B, h, w, gen, specials=False) for h, w in hw]
    disp[0][0] = 0.4375                                                               # a constant image: range 0
    disp[0][1] = float("nan")                                                         # no finite element
    disp[0][1, 0, 2, 3], disp[0][1, 0, 5, 9] = float("inf"), float("-inf")
    disp[1].view(torch.int32)[2] = cases.DENORMAL                                     # an image of denormals
    disp[1].view(torch.int32)[2, 0, 1, 1] = cases.NEG_DENORMAL
    stats = _new(B, H, W, hw, S, True, static_share=1.0)
    outs = _guarded(stats)
    stats.compute([idx.cuda(), idx.cuda()], [d.cuda() for d in disp])
    want = cases.check(stats, [idx, idx], disp)
    host = stats.host()
    assert [r["masked_share"] for r in host[0]][:2] == [1.0, 0.0]
    assert (host[0][0]["disp_min"], host[0][0]["disp_max"], host[0][0]["disp_std"]) == (0.4375, 0.4375, 0.0)
    assert (host[0][1]["disp_min"], host[0][1]["disp_max"], host[0][1]["disp_nonfinite"]) == (0.0, 0.0, 60)
    assert host[1][2]["disp_min"] < 0.0 < host[1][2]["disp_max"] == 1.401298464324817e-45 and want[1][2]["disp_sumsq"] > 0.0
    h = stats.history()
    assert (h[0]["static_images"], h[0]["first_static_pass"], h[0]["max_masked_share"], h[0]["max_masked_pass"]) == (1, 1, 1.0, 1)
    assert (h[0]["min_disp_range"], h[0]["min_disp_range_pass"], h[0]["bad_passes"], h[1]["bad_passes"]) == (0.0, 1, 1, 0)
    assert h[1]["min_disp_range"] == 2 * 1.401298464324817e-45 and _outputs_intact(outs)


# ---- 3. an absent map --------------------------------------------------------------------------------------------------------------
def test_a_none_entry_for_either_half():
    B, H, W, hw = _shapes()[5]
    idx, disp = _maps(B, H, W, hw, 2, True, 3)
    stats = _new(B, H, W, hw, 2, True)
    outs = _guarded(stats)
    gi, gd = [i.cuda() for i in idx], [d.cuda() for d in disp]
    for drop_i, drop_d in (((0,), (1,)), ((1, 2), (0, 3)), ((0, 1, 2, 3), ()), ((), (0, 1, 2, 3)), ((0, 1, 2, 3), (0, 1, 2, 3))):
        li = [None if s in drop_i else t for s, t in enumerate(gi)]
        ld = [None if s in drop_d else t for s, t in enumerate(gd)]
        stats.compute(li, ld)
        assert stats._last_native
        cases.check(stats, [None if t is None else t.cpu() for t in li], [None if t is None else t.cpu() for t in ld])
    h = stats.history()
    assert [x["passes"] for x in h] == [5] * 4 and [x["images"] for x in h] == [2 * B, 2 * B, 2 * B, 3 * B] and _outputs_intact(outs)


# ---- 4. determinism ------------------------------------------------------------------------------------------------------------------
def test_the_same_inputs_give_the_same_bytes():
    B, H, W, hw = _shapes()[5]
    idx, disp = _maps(B, H, W, hw, 4, True, 4)
    gi, gd = [i.cuda() for i in idx], [d.cuda() for d in disp]
    stats = _new(B, H, W, hw, 4, True)
    outs = _guarded(stats)
    first = stats.compute(gi, gd).clone()
    partials = stats._partials.clone()
    assert torch.equal(stats.compute(gi, gd), first) and torch.equal(stats.compute(gi, gd), first)
    assert torch.equal(stats._partials, partials) and not bool((partials == -1).all(dim=1).any())      # every slot was written
    other = _new(B, H, W, hw, 4, True)
    assert other._partials.data_ptr() != stats._partials.data_ptr()
    assert torch.equal(other.compute(gi, gd), first) and torch.equal(other._partials, partials)
    assert bool((first != 0).any()) and _outputs_intact(outs)


# ---- 5. the history on the device ------------------------------------------------------------------------------------------------
def test_history_over_six_passes_is_kept_on_the_device():
    stats, want = cases.run_history_sequence("cuda")
    assert stats._native and stats._last_native and stats._history.is_cuda
    cases.check_history(stats, want)
    cpu, _ = cases.run_history_sequence("cpu")
    assert torch.equal(stats._history.cpu(), cpu._history)                # the CPU sequence, bit for bit
    cases.check_reset(stats)


# ---- 6. capture ------------------------------------------------------------------------------------------------------------------
def test_captured_compute_replays_on_the_maps_of_the_moment():
    from mdx._lib import MdxError
    B, H, W, hw = _shapes()[5]
    stats = _new(B, H, W, hw, 2, True)
    outs = _guarded(stats)
    first = _maps(B, H, W, hw, 2, True, 60)
    gi, gd = [i.cuda() for i in first[0]], [d.cuda() for d in first[1]]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):                  # one stream, no parallel branches
        result = stats.compute(gi, gd)
    torch.cuda.synchronize()
    assert result is stats._records and all(h["passes"] == 0 for h in stats.history())      # a capture runs nothing
    seen = []
    for k in range(3):
        idx, disp = first if k == 0 else _maps(B, H, W, hw, 2, True, 60 + k, illegal=(k != 1))
        for dst, src in zip(gi + gd, idx + disp):               # in place: the graph holds the pointers
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        want = cases.check(stats, idx, disp)
        seen.append(stats._records.clone())
        assert (want[0][0]["bad_index"] > 0) == (k != 1)
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    hist = stats.history()
    assert all(h["passes"] == 3 and h["images"] == 3 * B and h["bad_passes"] == 3 for h in hist) and _outputs_intact(outs)
    # building and reading refuse a capture; the pass itself does not
    g2 = torch.cuda.CUDAGraph()
    count = []
    with torch.cuda.graph(g2, stream=side):
        for call in (stats.host, stats.history, stats.reset_history, lambda: _new(B, H, W, hw, 2, True),
                     lambda: stats.compute([i.long() for i in gi], gd)):
            with pytest.raises(MdxError, match="captured"):
                call()
            count.append(1)
        stats.compute(gi, gd)
    assert len(count) == 5


# ---- 7. no allocation ------------------------------------------------------------------------------------------------------------
def test_nothing_is_allocated_after_construction():
    B, H, W, hw = _shapes()[5]
    idx, disp = _maps(B, H, W, hw, 2, True, 7)
    gi, gd = [i.cuda() for i in idx], [d.cuda() for d in disp]
    stats = _new(B, H, W, hw, 2, True)
    stats.compute(gi, gd)
    torch.cuda.synchronize()
    mem, count = torch.cuda.memory_allocated(), torch.cuda.memory_stats()["allocation.all.allocated"]
    for k in range(3):
        stats.compute(gi if k != 1 else [None] * 4, gd)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == mem and torch.cuda.memory_stats()["allocation.all.allocated"] == count
    assert all(h["passes"] == 4 for h in stats.history())


def test_what_the_native_path_hands_to_torch():
    B, H, W, hw = 2, 24, 40, [(24, 40), (12, 20)]
    idx, disp = _maps(B, H, W, hw, 2, True, 8)
    stats = _new(B, H, W, hw, 2, True)
    gi, gd = [i.cuda() for i in idx], [d.cuda() for d in disp]
    stats.compute(gi, gd)
    native = stats._records.clone()
    # the int64 indices torch.min returns; a disparity that is a view with other strides: torch's functions, the same records
    wide = torch.stack([gd[1], gd[1]], dim=-1)[..., 0]
    assert not wide.is_contiguous()
    stats.compute([gi[0].long(), gi[1]], [gd[0], wide])
    assert stats._last_native is False and stats._records.is_cuda
    cases.check(stats, idx, disp)
    now = cases.records(stats)
    stats._records.copy_(native)
    for a, b in zip(sum(now, []), sum(cases.records(stats), [])):
        assert (a.disp_min, a.disp_max, list(a.winner), a.bad_index, a.disp_nonfinite) == \
               (b.disp_min, b.disp_max, list(b.winner), b.bad_index, b.disp_nonfinite)
    assert [h["passes"] for h in stats.history()] == [2, 2]
    with pytest.raises(ValueError):
        stats.compute([gi[0][:1], gi[1]], gd)


# ---- the trainer (the set-up of tests/test_gpu_gradstats.py: batch 2, 64x96, synthetic) ------------------------------------------------
def _trainer(graph, stats):
    bench = importlib.import_module("bench")
    from model_train import trainer
    torch.manual_seed(0)
    opt = bench.make_opt(2, height=64, width=96)
    opt.graph, opt.synthetic_length, opt.max_steps, opt.miopen_find = graph, 16, 0, False
    opt.noise = "device"
    opt.loss_stats, opt.loss_stats_static = stats, 0.9
    tr = trainer(opt)
    tr.setting.set_train()
    assert ("loss_stats" in tr.setting.optim) == (stats > 0)
    return tr, list(tr.setting.train_dataloader)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "captured"])
def test_the_trainers_report_is_the_reference_of_the_steps_own_outputs(graph):
    tr, batches = _trainer(graph, 1)
    stats, scales = tr.setting.optim["loss_stats"], tr.opt.scales
    assert stats._native and (stats.B, stats.H, stats.W, stats.S, stats.automask) == (2, 64, 96, 2, True)
    per_scale = [[] for _ in scales]
    for k, b in enumerate(batches[:3], start=1):
        outputs = tr.train_step(dict(b))
        tr.loss_stats(outputs, 10 * k)
        assert stats._last_native and bool(torch.isfinite(outputs["loss"]))
        idx = [outputs[("automask", s)].cpu() for s in scales]
        disp = [outputs[("disp", s)].detach().float().cpu() for s in scales]
        assert all(i.dtype == torch.uint8 for i in idx)
        want = cases.check(stats, idx, disp)
        for s, recs in enumerate(want):
            per_scale[s].append(recs)
            assert all(r["bad_index"] == 0 and r["disp_nonfinite"] == 0 and sum(r["winner"]) == 64 * 96 for r in recs)
    assert (tr._graphed is not None) == graph and tr._loss_stat_steps == {1: 10, 2: 20, 3: 30} and tr._loss_stat_torch == 0
    want = [cases.reference_history(p, 2, 64, 96, 2, True, 0.9) for p in per_scale]
    cases.check_history(stats, want)
    lines, record = tr.loss_stats_report()
    assert len(lines) == len(scales) and all(l.startswith("loss stats scale %d: 3 passes, masked " % s) for l, s in zip(lines, scales))
    assert record["passes"] == 3 and record["last_step"] == 30 and list(record["scales"]) == [str(s) for s in scales]
    for s, w in zip(scales, want):
        h = record["scales"][str(s)]["history"]
        assert list(h["shares"]) == ["identity -1", "identity 1", "frame -1", "frame 1"]
        assert h["min_disp_range_step"] == 10 * w["min_disp_range_pass"] and h["first_bad_step"] is None
        assert h["max_masked_step"] == (10 * w["max_masked_pass"] or None)
    assert tr.loss_stats_report()[0] == lines                   # asked again: the same answer
    tr.loss_stats_new_epoch()
    assert tr._loss_stat_steps == {} and all(h["passes"] == 0 for h in stats.history()) and tr._loss_stat_total == 3


def _losses(graph, stats, n=6):
    tr, batches = _trainer(graph, stats)
    torch.manual_seed(1)
    losses = []
    for k, b in enumerate(batches[:n], start=1):
        outputs = tr.train_step(dict(b))
        losses.append(float(outputs["loss"].detach()))
        tr.loss_stats(outputs, k)
    assert tr._loss_stat_total == (n if stats else 0)
    return losses


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "captured"])
def test_the_pass_changes_no_bit_of_the_losses(graph, monkeypatch):
    """Read-only: six steps with --loss_stats 1 and six without compute the same losses, bit for bit -- with MIOpen's deterministic
    solvers, without which two plain runs differ in the last digit (tests/test_gpu_digest.py)."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    plain, watched = _losses(graph, 0), _losses(graph, 1)
    print("graph=%s: plain %s, with the statistics %s" % (graph, ["%.9g" % x for x in plain], ["%.9g" % x for x in watched]))
    assert all(math.isfinite(x) for x in watched) and watched == plain and len(set(plain)) == len(plain)


class _Recorder(object):
    """mdx._lib.api with a note of every entry point asked for; everything is forwarded to the real one."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)

        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call


def test_without_the_option_nothing_is_built_or_launched(monkeypatch):
    import mdx._lib
    import mdx.functional
    import mdx.loss_stats
    built = []
    init = mdx.loss_stats.LossStats.__init__
    monkeypatch.setattr(mdx.loss_stats.LossStats, "__init__", lambda self, *a, **k: (built.append(1), init(self, *a, **k))[1])
    rec = _Recorder(mdx._lib.api)
    for module in (mdx._lib, mdx.loss_stats, mdx.functional):
        monkeypatch.setattr(module, "api", rec)
    tr, batches = _trainer(True, 0)
    for k, b in enumerate(batches[:3], start=1):
        tr.loss_stats(tr.train_step(dict(b)), k)
    torch.cuda.synchronize()
    assert built == [] and len(rec.calls) > 3 and not [c for c in rec.calls if c.startswith("mdx_loss_stats")]
    assert tr._loss_stat_total == 0 and tr._loss_stat_steps == {}
    # the recorder does see the entry points when the option is on
    tr, batches = _trainer(False, 1)
    tr.loss_stats(tr.train_step(dict(batches[0])), 1)
    launches = ("mdx_loss_stats_plan", "mdx_loss_stats_partials", "mdx_loss_stats_finish")
    assert built == [1] and [c for c in rec.calls if c in launches] == [launches[0]] * 2 + list(launches[1:])
    assert "mdx.loss_stats" in sys.modules
