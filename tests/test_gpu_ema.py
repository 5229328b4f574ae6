"""GPU: the weight average (mdx.optim.WeightEMA; csrc/ema.hip: update, tick, swap).  One update and a sequence against float64;
the swap, bit for bit and inside its bounds; a step the optimiser's guard skipped; the captured update; the trainer with --ema_decay --
plain, bf16, the split data-parallel form --, its validation on the averaged weights and its restart.

The bound of ONE update: the lerp rule has at most four float32 roundings (p - e, 1 - w -- exact for w >= 0.5 --, the product, the
sum), each at most 2**-24 of a value no larger than 2 max(|e|, |p|): 4 x 2**-24 x 2 = 2**-21 x max(|e|, |p|) per element.  After k
updates: k times that, over the running maximum magnitude."""
import importlib
import os

import numpy as np
import pytest
import torch

importlib.import_module("digging-into-self-supervised-monocular-depth-estimation_amd")

pytestmark = pytest.mark.gpu

# the tensor set of tests/test_gpu_guard.py (1, 17, 3x5, 4099: a chunk boundary and a scalar tail; the 4-D ones channels-last) ...
SHAPES = [(64, 6, 7, 7), (64,), (1,), (3, 5), (128, 64, 3, 3), (17,), (4099,), (256, 128, 1, 1), (12, 256, 1, 1), (2, 3, 4, 5)]
MIS = len(SHAPES)                        # ... one tensor whose live AND shadow storage start 4 bytes into larger buffers ...
SHAPES = SHAPES + [(5003,)]
TINY = len(SHAPES)                       # ... and 400 tensors of 1-5 elements: more than one launch's 384 table entries
SHAPES = SHAPES + [(1 + k % 5,) for k in range(400)]
SENTINEL = -123456.0
T_SAME = TINY + 7                        # with (64,) and (17,): tensors whose live values are set equal to the shadow
BOUND = 2.0 ** -21


def _misaligned(n):
    buf = torch.full((n + 8,), SENTINEL, device="cuda")
    view = buf[1:1 + n]
    assert view.data_ptr() % 16 == 4
    return buf, view


def _values(seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=gen) * scale for s in SHAPES]


class Bag(torch.nn.Module):
    def __init__(self, values):
        super().__init__()
        self.buffers_of_misaligned = []
        ps = []
        for i, v in enumerate(values):
            v = v.cuda()
            if v.dim() == 4:
                v = v.contiguous(memory_format=torch.channels_last)
            if i == MIS:
                buf, view = _misaligned(v.numel())
                view.copy_(v)
                self.buffers_of_misaligned.append(buf)
                v = view
            ps.append(torch.nn.Parameter(v))
        self.w = torch.nn.ParameterList(ps)

    def set(self, values):
        with torch.no_grad():
            for p, v in zip(self.w, values):
                p.copy_(v.cuda())


def _ema(values, decay, warmup):
    from mdx.optim import WeightEMA
    bag = Bag(values)
    buf, view = _misaligned(SHAPES[MIS][0])
    ema = WeightEMA([bag], decay, warmup=warmup, shadows={"0.w.%d" % MIS: view})
    ema.shadow_buffer = buf
    assert ema._native and len(ema._launches) == 2 and len(ema.live) == len(SHAPES)
    assert ema.shadow[MIS].data_ptr() % 16 == 4 and ema.live[MIS].data_ptr() % 16 == 4
    assert ema.shadow[0].stride() == ema.live[0].stride() and not ema.live[0].is_contiguous()
    return bag, ema


def _w(t, decay, warmup):
    d = min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay
    return float(np.float32(1.0 - d))


def _lerp64(e, p, w):
    e, p = e.double(), p.double()
    return e + w * (p - e) if w < 0.5 else p - (p - e) * (1.0 - w)


def _bits(ts):
    return [t.detach().clone().view(torch.int32) for t in ts]


def _same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _set_t(ema, t):
    st = ema.state_dict()
    st["updates"] = t
    ema.load_state_dict(st)


# ---- 1: one update against float64 ------------------------------------------------------------------------------------------
CASES = [("d=%g" % d, d, False, 0) for d in (0.9, 0.5, 0.4999, 0.999, 0.9999)] + [("t=%d" % t, 0.9999, True, t) for t in (0, 1, 8, 5000)]


@pytest.mark.parametrize("name, decay, warmup, t", CASES, ids=[c[0] for c in CASES])
def test_one_update_against_float64(name, decay, warmup, t):
    start, target = _values(1), _values(2)
    for k in (1, 5, T_SAME):                               # tensors whose live values equal the shadow: it keeps its bits
        target[k] = start[k].clone()
    bag, ema = _ema(start, decay, warmup)
    _set_t(ema, t)
    bag.set(target)
    e0, p = [e.clone() for e in ema.shadow], [x.detach().clone() for x in ema.live]
    ema.update()
    w = _w(t, decay, warmup)
    assert (w < 0.5) == (name not in ("d=0.5", "d=0.4999", "t=0", "t=1", "t=8"))       # both forms of the rule are met
    worst = 0.0
    for i, (got, e, x) in enumerate(zip(ema.shadow, e0, p)):
        ref = _lerp64(e, x, w)
        lim = BOUND * torch.maximum(e.abs(), x.abs()).double()
        err = (got.double() - ref).abs()
        assert bool((err <= lim).all()), (name, i, SHAPES[i], float((err - lim).max()))
        worst = max(worst, float((err / lim.clamp_min(1e-300)).max()))
        if i in (1, 5, T_SAME):
            assert torch.equal(got.view(torch.int32), e.view(torch.int32)), i
        else:
            assert not torch.equal(got, e)
    print("%s: w = %.9g, worst error %.3f of the bound" % (name, w, worst))
    assert ema.stats() == dict(updates=t + 1, held=0)
    assert _same_bits(_bits(ema.live), _bits(p))           # the live tensors are only read


# ---- 2: a sequence ------------------------------------------------------------------------------------------------------------
def _sequence(n=40, decay=0.999, check=True):
    bag, ema = _ema(_values(3), decay, True)
    ref = [e.double().clone() for e in ema.shadow]
    big = [e.abs().double() for e in ema.shadow]
    worst = 0.0
    for k in range(n):
        bag.set(_values(100 + k, 1.0 + 0.1 * k))
        ema.update()
        w = _w(k, decay, True)
        for i, x in enumerate(ema.live if check else []):
            ref[i] = _lerp64(ref[i], x.detach(), w)
            big[i] = torch.maximum(big[i], torch.maximum(x.detach().abs().double(), ref[i].abs()))
            err = (ema.shadow[i].double() - ref[i]).abs()
            lim = (k + 1) * BOUND * big[i]
            assert bool((err <= lim).all()), (k, i, SHAPES[i], float(err.max()), float(lim.min()))
            worst = max(worst, float((err / lim).max()))
    return ema, worst


def test_sequence_against_the_float64_chain():
    a, worst = _sequence()
    print("40 updates: worst error %.3f of k x 2^-21 x M" % worst)
    assert a.stats() == dict(updates=40, held=0)
    b, _ = _sequence(check=False)
    assert _same_bits(_bits(a.shadow), _bits(b.shadow))    # no atomics: the same bits every time
    assert float(a.shadow_buffer[0]) == SENTINEL and bool((a.shadow_buffer[1 + 5003:] == SENTINEL).all())


# ---- 3: the swap -------------------------------------------------------------------------------------------------------------
def test_swap_exchanges_bits_inside_its_bounds():
    bag, ema = _ema(_values(4), 0.9, True)
    bag.set(_values(5))
    with torch.no_grad():                                   # payloads a float operation would not carry: NaNs, a negative zero
        ema.live[6].view(torch.int32)[4098] = 0x7FC12345
        ema.shadow[6].view(torch.int32)[0] = -0x003FEDCC
        ema.live[MIS][5002] = -0.0
    p0, e0 = _bits(ema.live), _bits(ema.shadow)
    assert not any(torch.equal(a, b) for a, b in zip(p0[:TINY], e0[:TINY]))
    ema.swap()
    assert _same_bits(_bits(ema.live), e0) and _same_bits(_bits(ema.shadow), p0)
    assert torch.equal(bag.state_dict()["w.0"].view(torch.int32), e0[0])       # what a checkpoint under the swap holds
    ema.swap()
    assert _same_bits(_bits(ema.live), p0) and _same_bits(_bits(ema.shadow), e0)
    for buf in (bag.buffers_of_misaligned[0], ema.shadow_buffer):
        assert float(buf[0]) == SENTINEL and bool((buf[1 + 5003:] == SENTINEL).all()) and buf.numel() == 5003 + 8
    assert ema.stats() == dict(updates=0, held=0)
    with ema.applied():
        assert _same_bits(_bits(ema.live), e0)
    assert _same_bits(_bits(ema.live), p0)


# ---- 4: the guard ------------------------------------------------------------------------------------------------------------
def test_a_skipped_step_does_not_move_the_average():
    """The NaN is a gradient VALUE only (as tests/test_gpu_guard.py injects it)."""
    from mdx.optim import Adam
    bag, ema = _ema(_values(6), 0.9, True)
    params = list(bag.w)
    opt = Adam(params, 1e-2, skip_nonfinite=True)

    def step(seed, poison):
        for p, g in zip(params, _values(seed)):
            p.grad = torch.empty_like(p).copy_(g.cuda())
        if poison:
            params[6].grad[4098] = float("nan")
        opt.step()
        ema.update(opt)

    def expect(e_before, t):
        for i, (got, e, x) in enumerate(zip(ema.shadow, e_before, ema.live)):
            ref = _lerp64(e, x.detach(), _w(t, 0.9, True))
            assert bool(((got.double() - ref).abs() <= BOUND * torch.maximum(e.abs(), x.detach().abs()).double()).all()), (t, i)

    e0 = [e.clone() for e in ema.shadow]
    step(20, False)
    expect(e0, 0)
    assert ema.stats() == dict(updates=1, held=0)
    e1, live1 = _bits(ema.shadow), _bits(ema.live)
    keep = [e.clone() for e in ema.shadow]
    step(21, True)
    assert opt.guard_stats()["skipped"] is True
    assert _same_bits(_bits(ema.shadow), e1) and _same_bits(_bits(ema.live), live1)
    assert ema.stats() == dict(updates=1, held=1)
    step(22, False)                                         # the next finite step: update t = 1
    expect(keep, 1)
    assert not _same_bits(_bits(ema.shadow[:TINY]), e1[:TINY])
    assert ema.stats() == dict(updates=2, held=1)
    # without a record pointer the update always applies, also right behind a skipped step
    step(23, True)
    assert ema.stats() == dict(updates=2, held=2)
    keep = [e.clone() for e in ema.shadow]
    bag.set(_values(24))
    ema.update()
    expect(keep, 2)
    assert ema.stats() == dict(updates=3, held=2)


# ---- 5: capture --------------------------------------------------------------------------------------------------------------
def test_captured_update_and_swap_pair_equal_the_eager_sequence():
    seq = [_values(30 + k) for k in range(5)]
    a_bag, a = _ema(_values(7), 0.99, True)
    for v in seq:
        a_bag.set(v)
        a.update()
        a.swap()
        a.swap()
    b_bag, b = _ema(_values(7), 0.99, True)
    snap = b.snapshot()
    b.update()                                              # the eager warm-up, undone
    b.swap()
    b.swap()
    b.restore(snap)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        b.update()
        b.swap()
        b.swap()
    assert b.stats() == dict(updates=0, held=0)             # a capture runs nothing
    for v in seq:
        b_bag.set(v)
        graph.replay()
    assert _same_bits(_bits(b.shadow), _bits(a.shadow)) and _same_bits(_bits(b.live), _bits(a.live))
    assert a.stats() == b.stats() == dict(updates=5, held=0)


# ---- 6-8: the trainer (the options of tests/test_gpu_driver.py: _trainer_losses -- batch 2, 64x96, synthetic, 6 steps) ---------
def _same_trajectory(a, b):
    assert all(np.isfinite(a)) and all(np.isfinite(b)), (a, b)
    np.testing.assert_allclose(a[:3], b[:3], rtol=2e-4, atol=1e-6)     # float32 rounding / atomics-order differences ...
    np.testing.assert_allclose(a, b, rtol=1e-2, atol=1e-5)             # ... which Adam amplifies step by step


def _trainer_losses(graph, decay, amp="none", n=6, lr_change_at=4):
    """-> losses, trainer.  With an average: after every step the shadows are held against the float64 chain over the live values
    of that step."""
    bench = importlib.import_module("bench")
    from model_train import trainer
    torch.manual_seed(0)
    opt = bench.make_opt(2, height=64, width=96, amp=amp)
    opt.use_automasking, opt.graph, opt.synthetic_length, opt.max_steps, opt.miopen_find = False, graph, 16, 0, False
    opt.ema_decay = decay
    tr = trainer(opt)
    tr.setting.set_train()
    batches = list(tr.setting.train_dataloader)[:n]
    ema = tr.setting.optim.get("ema")
    assert (ema is not None) == (decay > 0)
    if ema is not None:
        assert ema._native and len(ema.live) > 100
        assert any(n.endswith("running_var") for n in ema.names) and not any("num_batches_tracked" in n or ".fc." in n for n in ema.names)
        assert all(torch.equal(e, t) for e, t in zip(ema.shadow, ema.live))
        ref = [e.double().clone() for e in ema.shadow]
        big = [e.abs().double() for e in ema.shadow]
    torch.manual_seed(1)
    losses, worst = [], 0.0
    for k, b in enumerate(batches):
        if k == lr_change_at:
            for g in tr.setting.optim["optimizer"].param_groups:       # what StepLR does at an epoch boundary
                if torch.is_tensor(g["lr"]):
                    g["lr"].fill_(1e-6)
                else:
                    g["lr"] = 1e-6
        losses.append(float(tr.train_step(dict(b))["loss"].detach()))
        if ema is not None:
            w = _w(k, decay, True)
            for i, x in enumerate(ema.live):
                ref[i] = _lerp64(ref[i], x.detach(), w)
                big[i] = torch.maximum(big[i], torch.maximum(x.detach().abs().double(), ref[i].abs()))
                err = (ema.shadow[i].double() - ref[i]).abs()
                lim = (k + 1) * BOUND * big[i]
                assert bool((err <= lim).all()), (k, ema.names[i], float(err.max()))
                worst = max(worst, float((err / lim.clamp_min(1e-300)).max()))
    if ema is not None:
        print("graph=%s amp=%s: shadows within %.3f of k x 2^-21 x M over %d steps" % (graph, amp, worst, n))
        assert ema.stats() == dict(updates=n, held=0)       # the warm-up's updates are undone
        assert not all(torch.equal(e, t) for e, t in zip(ema.shadow, ema.live))
    assert (tr._graphed is not None) == graph
    return losses, tr


_PLAIN = {}


def _plain(graph, amp="none"):
    """The run without an average, once per form."""
    if (graph, amp) not in _PLAIN:
        _PLAIN[(graph, amp)] = _trainer_losses(graph, 0.0, amp=amp)[0]
    return _PLAIN[(graph, amp)]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "captured"])
def test_trainer_with_the_average_follows_the_plain_trajectory(graph):
    losses, tr = _trainer_losses(graph, 0.99)
    _same_trajectory(losses, _plain(graph))


def test_trainer_bf16_shadow_weights():
    losses, tr = _trainer_losses(True, 0.99, amp="bf16")
    assert all(t.dtype == torch.float32 for t in tr.setting.optim["ema"].live)      # the float32 masters, never the bf16 copies
    np.testing.assert_allclose(losses, _plain(True, "bf16"), rtol=5e-2, atol=1e-4)   # tests/test_gpu_driver.py's bf16 rule


@pytest.fixture
def rccl_group_of_one():
    import torch.distributed as dist
    import bench
    assert not dist.is_initialized()
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % bench.free_port(), rank=0, world_size=1,
                            device_id=torch.device(torch.cuda.current_device()))
    yield dist
    dist.destroy_process_group()


def test_trainer_split_form_updates_inside_graph_b(rccl_group_of_one, monkeypatch):
    monkeypatch.setenv("MDX_DP_SPLIT", "1")
    plain, tr_p = _trainer_losses(True, 0.0)
    losses, tr = _trainer_losses(True, 0.99)
    g = tr._graphed
    assert g is not None and g.split and g.graph_apply is not None
    _same_trajectory(losses, plain)
    for t in (tr_p, tr):
        t.setting.sync.detach()


# ---- 9, 10: validation on the average, restart -----------------------------------------------------------------------------------
def _epoch_opt(epochs, decay, save, resume=0):
    bench = importlib.import_module("bench")
    opt = bench.make_opt(2, height=64, width=96)
    opt.use_automasking, opt.graph, opt.synthetic_length, opt.max_steps, opt.miopen_find = False, True, 8, 2, False
    opt.epoch, opt.save, opt.resume, opt.ema_decay = epochs, save, resume, decay
    return opt


def _record_valid_means(tr):
    """The epoch means of the validation, as control.epoch_means hands them to the log (the second call of every epoch)."""
    seen, real = [], tr.control.epoch_means

    def epoch_means(log):
        out = real(log)
        seen.append(out)
        return out
    tr.control.epoch_means = epoch_means
    return seen


def test_validation_runs_on_the_average_and_puts_the_weights_back(tmp_path, monkeypatch, capsys):
    from model_train import trainer
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    tr = trainer(_epoch_opt(1, 0.99, "ema_valid"))
    ema = tr.setting.optim["ema"]
    tensors = [t for net in tr.setting.raw_model.values() for t in list(net.parameters()) + list(net.buffers())]
    seen, states, real_swap = _record_valid_means(tr), [], ema.swap

    def swap():
        if len(states) % 2 == 0:
            states.append([t.detach().clone() for t in tensors])           # before swapping in
            real_swap()
        else:
            real_swap()
            states.append([t.detach().clone() for t in tensors])           # after swapping out
    ema.swap = swap
    tr.train()
    torch.cuda.synchronize()
    assert len(states) == 4                                 # around the validation loop, around the averaged checkpoints
    for before, after in (states[0:2], states[2:4]):
        assert all(torch.equal(a, b) for a, b in zip(before, after))
    # (between the two pairs the live checkpoint was written: state_dict() brings num_batches_tracked up to date, nothing else)
    assert all(torch.equal(a, b) for a, b in zip(states[1], states[2]) if a.is_floating_point())
    assert "weight EMA: 2 updates, 0 held" in capsys.readouterr().out
    assert tr._graphed_valid is not None and tr._graphed_valid.replays == 2
    want = seen[1]["loss"]
    d = os.path.join("model_save", "ema_valid")
    assert sorted(os.listdir(d)) == sorted(["loss", "state1.pt"] + [p + k + "1.pt" for k in tr.setting.raw_model for p in ("", "ema_")])
    # a second trainer, no average: the written ema_<key> files as its networks, the same validation loop
    torch.manual_seed(0)
    other = trainer(_epoch_opt(1, 0.0, "unused"))
    assert "ema" not in other.setting.optim
    for key, net in other.setting.raw_model.items():
        net.load_state_dict(torch.load(os.path.join(d, "ema_%s1.pt" % key), map_location=other.device))
    other.setting.set_valid()
    log = {k: [] for k in other.control.metric_name}
    for step, inputs in enumerate(other.batches(other.setting.valid_dataloader)):
        with torch.no_grad():
            log = other.control.metric(inputs, other.valid_step(inputs), log)
        if step + 1 >= 2:
            break
    got = other.control.epoch_means(log)["loss"]
    print("validation loss on the average %.9g, from the ema_ files %.9g" % (want, got))
    assert np.isfinite(want) and abs(got - want) <= 1e-6 * abs(want)


def test_restart_carries_the_average_on(tmp_path, monkeypatch):
    """Two epochs, then a third from the checkpoint, against three epochs straight.  Every epoch's shuffle is seeded alike in both
    runs, so they see the same batches.

    (1) What resume hands the third epoch is held bit for bit: shadows and counters as the two-epoch run left them.
    (2) The resumed epoch is held to the float64 chain: from the handed shadows, updates t = 4 and t = 5 over that trainer's own
    live weights after each step, at the sequence test's bound k x 2**-21 x M.  Deterministic; a wrong t, warm-up updates of the
    new capture left in, or an average restarted from the loaded weights miss it by orders of magnitude.
    (3) Straight against restarted.  The two six-step runs are not bit-equal: the step's reductions use float atomics, and Adam's
    first steps have the size of the learning rate whatever the gradient's, so a last-bit difference in a near-zero gradient moves
    that element the other way by a whole step.  _same_trajectory's rule (1e-2 relative, 1e-5 absolute) is a rule for aggregates
    -- the loss is a mean over the batch's pixels -- so it is applied to each tensor as a whole, not to single elements:
      * trained parameters whose scale the initialisation sets: rms(x - y) <= 1e-2 rms(x) + 1e-5;
      * batch-norm statistics, themselves means over a map: max |x - y| <= 1e-2 max |x| + 1e-5 (an element may be zero by
        cancellation, so the scale is the tensor's);
      * parameters initialised to zero (the batch-norm biases) have no scale but the distance they travelled, at most six steps of
        1e-4, and 1e-2 of that is a fraction of ONE step's sign: the rule cannot hold for them and is not asked; their figure, and
        the element-wise figure of the others, are printed.
    Figures measured on an MI355X: LABNOTES, "The weight average"."""
    from model_train import trainer
    monkeypatch.chdir(tmp_path)
    handed, chain = {}, {}

    def run(epochs, save, resume):
        torch.manual_seed(0)
        tr = trainer(_epoch_opt(epochs, 0.99, save, resume))
        ema = tr.setting.optim["ema"]
        initial = [t.detach().clone() for t in ema.live]
        epoch, real, real_resume, real_step = [resume], tr.setting.set_train, tr.control.resume, tr.train_step

        def set_train():
            torch.manual_seed(1000 + epoch[0])              # the loader's shuffle of this epoch
            epoch[0] += 1
            real()

        def resume_and_look(*a, **kw):
            out = real_resume(*a, **kw)
            handed.update(stats=ema.stats(), shadow=[e.clone() for e in ema.shadow])
            chain.update(t=handed["stats"]["updates"], k=0, worst=0.0, ref=[e.double() for e in ema.shadow],
                         big=[e.abs().double() for e in ema.shadow])
            return out

        def step_and_follow(inputs):
            out = real_step(inputs)
            if resume:
                w = _w(chain["t"], 0.99, True)
                chain["t"], chain["k"] = chain["t"] + 1, chain["k"] + 1
                for i, x in enumerate(ema.live):
                    ref = chain["ref"][i] = _lerp64(chain["ref"][i], x.detach(), w)
                    big = chain["big"][i] = torch.maximum(chain["big"][i], torch.maximum(x.detach().abs().double(), ref.abs()))
                    err, lim = (ema.shadow[i].double() - ref).abs(), chain["k"] * BOUND * big
                    assert bool((err <= lim).all()), (chain["t"] - 1, ema.names[i], float(err.max()))
                    chain["worst"] = max(chain["worst"], float((err / lim.clamp_min(1e-300)).max()))
            return out
        tr.setting.set_train, tr.control.resume, tr.train_step = set_train, resume_and_look, step_and_follow
        tr.train()
        torch.cuda.synchronize()
        return tr, initial

    straight, initial = run(3, "straight", 0)
    two = run(2, "restart", 0)[0].setting.optim["ema"]
    resumed = run(3, "restart", 2)[0]
    # (1)
    assert handed["stats"] == two.stats() == dict(updates=4, held=0)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(handed["shadow"], two.shadow))
    # (2)
    assert chain["k"] == 2 and chain["t"] == 6
    print("resumed epoch: shadows within %.3f of k x 2^-21 x M of the float64 chain from the handed shadows, t = 4, 5" % chain["worst"])
    a, b = straight.setting.optim["ema"], resumed.setting.optim["ema"]
    assert a.stats() == b.stats() == dict(updates=6, held=0)
    assert not all(torch.equal(x, y) for x, y in zip(b.shadow, handed["shadow"]))
    # (3)
    worst, elementwise, zero_init, n_zero = {"parameters": 0.0, "statistics": 0.0}, 0.0, 0.0, 0
    for n, t, x0, x, y in zip(a.names, a.live, initial, a.shadow, b.shadow):
        d = (x - y).double()
        if not isinstance(t, torch.nn.Parameter):
            kind, err, lim = "statistics", float(d.abs().max()), 1e-2 * float(x.abs().max()) + 1e-5
        elif float(x0.abs().max()) == 0.0:
            n_zero += 1
            zero_init = max(zero_init, float(d.pow(2).mean().sqrt()) / (1e-2 * float(x.double().pow(2).mean().sqrt()) + 1e-5))
            continue
        else:
            kind, err, lim = "parameters", float(d.pow(2).mean().sqrt()), 1e-2 * float(x.double().pow(2).mean().sqrt()) + 1e-5
            elementwise = max(elementwise, float(d.abs().max()) / (1e-2 * float(x.abs().max()) + 1e-5))
        worst[kind] = max(worst[kind], err / lim)
        assert err <= lim, (n, kind, err, lim)
    print("restart against straight, of the rule: parameters (rms) %.3f, batch-norm statistics (max) %.3f; not asserted: the "
          "parameters' largest element at tensor scale %.3f, %d zero-initialised parameters (rms) %.3f"
          % (worst["parameters"], worst["statistics"], elementwise, n_zero, zero_init))
    assert torch.load(os.path.join("model_save", "restart", "state3.pt"))["ema"]["updates"] == 6
