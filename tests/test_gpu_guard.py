"""GPU: the step guard of mdx.optim.Adam (csrc/adam.hip: sum of squares, finish, guarded Adam).  The global norm against float64, its
determinism and range; the guarded step without a limit against the unguarded one, bit for bit; the clipped step against torch's
fused Adam on scaled gradients; a non-finite gradient anywhere -- vector path, scalar tail, second launch, misaligned gradient --
leaves no trace; a captured guarded step; the trainer with a loss that goes to infinity for one step.

Non-finite values are injected as gradient or loss VALUES only (never through poses, intrinsics or images, which feed index
arithmetic and running statistics)."""
import importlib
import struct

import pytest
import torch

importlib.import_module("digging-into-self-supervised-monocular-depth-estimation_amd")

pytestmark = pytest.mark.gpu

# the parameter set of tests/test_gpu_optim.py (1, 17, 3x5, 4099: a chunk boundary and a scalar tail) ...
SHAPES = [(64, 6, 7, 7), (64,), (1,), (3, 5), (128, 64, 3, 3), (17,), (4099,), (256, 128, 1, 1), (12, 256, 1, 1), (2, 3, 4, 5)]
MIS = len(SHAPES)                        # ... one parameter whose gradient starts one element into a larger buffer ...
SHAPES = SHAPES + [(5003,)]
TINY = len(SHAPES)                       # ... and 400 tensors of 1-5 elements: more than one launch's 384 gradient pointers
SHAPES = SHAPES + [(1 + k % 5,) for k in range(400)]
T4099 = 6


def _on_gpu(values, misaligned):
    g = values.cuda()
    if g.dim() == 4:
        return g.contiguous(memory_format=torch.channels_last)
    if misaligned:
        buf = torch.zeros(g.numel() + 8, device="cuda")
        view = buf[1:1 + g.numel()]
        view.copy_(g)
        assert view.data_ptr() % 16 == 4
        return view
    return g


def _params(seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [_on_gpu(torch.randn(*s, generator=gen), False).requires_grad_(True) for s in SHAPES]


def _grads(seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return [_on_gpu(torch.randn(*s, generator=gen) * scale, i == MIS) for i, s in enumerate(SHAPES)]


def _copy(grads):
    return [_on_gpu(g.detach().cpu().contiguous(), i == MIS) for i, g in enumerate(grads)]


def _run(make, steps):
    """`steps`: a list of gradient lists.  -> parameters, optimiser, [guard_stats() after each step] (guarded optimisers)."""
    ps = _params()
    opt = make(ps)
    stats = []
    for grads in steps:
        for p, g in zip(ps, grads):
            p.grad = g
        opt.step()
        if getattr(opt, "guarded", False):
            stats.append(opt.guard_stats())
    return ps, opt, stats


def _state(ps, opt):
    out = []
    for p in ps:
        st = opt.state[p]
        out.append((p.detach(), st["exp_avg"], st["exp_avg_sq"], st["step"]))
    return out


def _assert_equal(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        for u, v, what in zip(x, y, ("param", "exp_avg", "exp_avg_sq", "step")):
            assert torch.equal(u, v), (what, i, SHAPES[i])


def _norm64(grads):
    return float(torch.stack([(g.detach().cpu().double() ** 2).sum() for g in grads]).sum().sqrt())


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


@pytest.fixture(scope="module")
def good():
    """Gradients of three steps and the state an unguarded optimiser reaches over the first and the third."""
    from mdx.optim import Adam
    steps = [_grads(11), _grads(12), _grads(13)]
    ps, opt, _ = _run(lambda ps: Adam(ps, 1e-3), [steps[0], steps[2]])
    return steps, [tuple(t.clone() for t in row) for row in _state(ps, opt)]


# ---- the norm -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 1e-3, 1e4])
def test_norm_is_the_float64_norm_rounded_once(scale):
    from mdx.optim import Adam
    grads = _grads(5, scale)
    want = _norm64(grads)
    runs = [_run(lambda ps: Adam(ps, 1e-3, skip_nonfinite=True), [grads])[2][0] for _ in range(2)]
    got = runs[0]["total_norm"]
    print("norm %.9g, float64 %.17g, relative error %.3g" % (got, want, abs(got - want) / want))
    assert abs(got - want) <= 2.0 ** -23 * want
    assert _bits(runs[0]["total_norm"]) == _bits(runs[1]["total_norm"])        # no atomics: the same bits every time
    assert runs[0]["coef"] == 1.0 and runs[0]["skipped"] is False and runs[0]["steps"] == 1 and runs[0]["skipped_steps"] == 0


def test_large_finite_gradients_are_not_flagged():
    """Every gradient 1e30: the float32 squares overflow, the norm (1e30 x sqrt(n)) does not."""
    from mdx.optim import Adam
    grads = [torch.full_like(g, 1e30) for g in _grads(5)]
    grads[MIS] = _on_gpu(torch.full(SHAPES[MIS], 1e30), True)
    ps, opt, stats = _run(lambda ps: Adam(ps, 1e-3, skip_nonfinite=True, max_grad_norm=1.0), [grads])
    want = _norm64(grads)
    assert abs(stats[0]["total_norm"] - want) <= 2.0 ** -23 * want
    assert stats[0]["skipped"] is False and stats[0]["skipped_steps"] == 0 and 0 < stats[0]["coef"] < 1e-30
    assert all(float(opt.state[p]["step"]) == 1.0 for p in ps)


# ---- skip on, no limit, finite gradients: the unguarded step's bits ---------------------------------------------------------
def test_guard_without_a_limit_gives_the_unguarded_bits():
    from mdx.optim import Adam
    steps = [_grads(20 + k, 10.0 ** (k - 2)) for k in range(5)]
    a, oa, stats = _run(lambda ps: Adam(ps, 1e-3, skip_nonfinite=True), steps)
    b, ob, _ = _run(lambda ps: Adam(ps, 1e-3), steps)
    _assert_equal(_state(a, oa), _state(b, ob))
    assert all(float(oa.state[p]["step"]) == 5.0 for p in a)
    assert stats[-1]["steps"] == 5 and stats[-1]["skipped_steps"] == 0 and all(s["coef"] == 1.0 for s in stats)
    for p, g in zip(a, steps[-1]):
        assert p.grad is g                                  # .grad keeps the raw values: the native path never writes it
    assert set(oa.state_dict()["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}


def test_the_norm_is_global_over_parameter_groups():
    """Two groups with their own learning rates and betas: ONE norm over both, each group's launches with its own hyper-parameters."""
    from mdx.optim import Adam
    steps = [_grads(40 + k) for k in range(3)]

    def groups(ps):
        return [dict(params=ps[:MIS + 20], lr=1e-3), dict(params=ps[MIS + 20:], lr=5e-3, betas=(0.8, 0.99))]
    a, oa, stats = _run(lambda ps: Adam(groups(ps), 1e-3, skip_nonfinite=True), steps)
    b, ob, _ = _run(lambda ps: Adam(groups(ps), 1e-3), steps)
    _assert_equal(_state(a, oa), _state(b, ob))
    for st, grads in zip(stats, steps):
        want = _norm64(grads)
        assert abs(st["total_norm"] - want) <= 2.0 ** -23 * want
    # a bad value in the second group stops the first group's tensors too
    bad = _poison(steps[1], "last-of-last", float("nan"))
    c, oc, stats = _run(lambda ps: Adam(groups(ps), 1e-3, skip_nonfinite=True), [steps[0], bad, steps[2]])
    d, od, _ = _run(lambda ps: Adam(groups(ps), 1e-3), [steps[0], steps[2]])
    _assert_equal(_state(c, oc), _state(d, od))
    assert stats[-1]["skipped_steps"] == 1


# ---- clip ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm", [1e9, 1.0, 1e-6], ids=["below", "above", "tiny"])
def test_clip_equals_torch_fused_adam_on_scaled_gradients(max_norm):
    """coef in float32 from the norm the record reports (the norm itself: test_norm_is_the_float64_norm_rounded_once); Adam on
    g * coef held to the bar of tests/test_gpu_optim.py."""
    from mdx.optim import Adam
    steps = [_grads(30 + k, 10.0 ** (k - 2)) for k in range(5)]
    keep = [[g.clone() for g in grads] for grads in steps]
    a, oa, stats = _run(lambda ps: Adam(ps, 1e-3, max_grad_norm=max_norm), steps)
    b = _params()
    ob = torch.optim.Adam(b, 1e-3, fused=True)
    for grads, st in zip(steps, stats):
        c = torch.tensor(max_norm, dtype=torch.float32) / (torch.tensor(st["total_norm"], dtype=torch.float32) + torch.tensor(1e-6, dtype=torch.float32))
        coef = min(1.0, float(c))
        assert st["coef"] == coef, (st, coef)
        assert (coef == 1.0) == (max_norm == 1e9)
        dev = torch.tensor(coef, dtype=torch.float32, device="cuda")
        for p, g in zip(b, grads):
            p.grad = g * dev
        ob.step()
    for grads, kept in zip(steps, keep):
        for g, k in zip(grads, kept):
            assert torch.equal(g, k)                        # the gradients keep their raw values
    same = total = 0
    for x, y in zip(a, b):
        sx, sy = oa.state[x], ob.state[y]
        assert float(sx["step"]) == float(sy["step"]) == 5.0
        for u, v, what in ((x, y, "param"), (sx["exp_avg"], sy["exp_avg"], "exp_avg"), (sx["exp_avg_sq"], sy["exp_avg_sq"], "exp_avg_sq")):
            d = float((u.detach() - v.detach()).abs().max())
            assert d <= 2e-7 * max(1e-30, float(v.detach().abs().max())), (what, tuple(x.shape), d)
            same += int((u == v).sum())
            total += u.numel()
    print("equal bits: %d of %d" % (same, total))
    assert same >= 0.98 * total, (same, total)


# ---- skip ---------------------------------------------------------------------------------------------------------------------
def _last(shape):
    return tuple(s - 1 for s in shape)


WHERE = {
    "first-of-first": (0, (0, 0, 0, 0)),                    # the vector path's first load
    "tail-of-4099": (T4099, (4098,)),                       # the scalar tail behind a full chunk
    "last-of-last": (len(SHAPES) - 1, _last(SHAPES[-1])),   # the last tensor's last element (scalar path, second launch)
    "second-launch": (384 + 3, (0,)),                       # a tensor behind the first 384 gradient pointers
    "misaligned": (MIS, (4100,)),                           # the 4-byte aligned gradient, in its second chunk
}


def _poison(grads, where, value):
    bad = _copy(grads)
    t, idx = WHERE[where]
    bad[t][idx] = value
    assert not bool(torch.isfinite(bad[t]).all())
    return bad


@pytest.mark.parametrize("where", sorted(WHERE))
@pytest.mark.parametrize("value", [float("inf"), float("-inf"), float("nan")], ids=["+inf", "-inf", "nan"])
def test_a_non_finite_step_leaves_no_trace(good, value, where):
    from mdx.optim import Adam
    steps, want = good
    bad = _poison(steps[1], where, value)
    ps, opt, stats = _run(lambda ps: Adam(ps, 1e-3, skip_nonfinite=True), [steps[0], bad, steps[2]])
    _assert_equal(_state(ps, opt), want)
    assert all(float(opt.state[p]["step"]) == 2.0 for p in ps)
    assert [s["skipped"] for s in stats] == [False, True, False]
    assert stats[-1]["steps"] == 3 and stats[-1]["skipped_steps"] == 1
    assert stats[1]["total_norm"] != stats[1]["total_norm"] or abs(stats[1]["total_norm"]) == float("inf")


def test_a_non_finite_step_with_a_limit_leaves_no_trace(good):
    from mdx.optim import Adam
    steps, _ = good
    bad = _poison(steps[1], "tail-of-4099", float("nan"))
    a, oa, stats = _run(lambda ps: Adam(ps, 1e-3, skip_nonfinite=True, max_grad_norm=1.0), [steps[0], bad, steps[2]])
    b, ob, _ = _run(lambda ps: Adam(ps, 1e-3, max_grad_norm=1.0), [steps[0], steps[2]])
    _assert_equal(_state(a, oa), _state(b, ob))
    assert stats[-1]["skipped_steps"] == 1 and stats[-1]["coef"] < 1.0


@pytest.mark.parametrize("max_norm", [None, 1.0], ids=["no-limit", "limit"])
def test_without_skip_a_nan_gradient_goes_through(good, max_norm):
    """The control: what the guard prevents.  With a limit the NaN norm gives a NaN coefficient, as clip_grad_norm_ does."""
    from mdx.optim import Adam
    steps, _ = good
    bad = _poison(steps[1], "tail-of-4099", float("nan"))
    make = (lambda ps: Adam(ps, 1e-3, max_grad_norm=max_norm)) if max_norm else (lambda ps: Adam(ps, 1e-3))
    ps, opt, stats = _run(make, [steps[0], bad, steps[2]])
    assert not bool(torch.isfinite(ps[T4099]).all())
    assert all(float(opt.state[p]["step"]) == 3.0 for p in ps)
    if max_norm:
        assert stats[1]["coef"] != stats[1]["coef"] and stats[-1]["skipped_steps"] == 0
        assert not any(bool(torch.isfinite(p).all()) for p in ps)


# ---- capture ------------------------------------------------------------------------------------------------------------------
def test_captured_guarded_step_equals_the_eager_sequence(good):
    from mdx.optim import Adam
    steps, _ = good
    seq = [steps[0], _poison(steps[1], "first-of-first", float("inf")), steps[2]]

    def make(ps):
        opt = Adam(ps, 2e-3, skip_nonfinite=True, max_grad_norm=50.0)
        lr = torch.tensor(2e-3, device="cuda")
        for g in opt.param_groups:
            g["capturable"], g["lr"] = True, lr
        return opt

    a, oa, stats = _run(make, seq)
    b = _params()
    ob = make(b)
    static = _copy(seq[0])
    for p, g in zip(b, static):
        p.grad = g
    start = [p.detach().clone() for p in b]
    ob.step()                                               # the warm-up: state, plan, partials and record are allocated here
    with torch.no_grad():
        for p, s in zip(b, start):
            p.copy_(s)
            for v in ob.state[p].values():
                v.zero_()
    ob.guard_restore((None, dict(total_norm=0.0, coef=1.0, skipped=False, steps=0, skipped_steps=0), True))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ob.step()
    assert ob.guard_stats()["steps"] == 0                   # a capture runs nothing
    got = []
    for grads in seq:
        for s, g in zip(static, grads):
            s.copy_(g)
        graph.replay()
        got.append(ob.guard_stats())
    _assert_equal(_state(b, ob), _state(a, oa))
    assert all(float(ob.state[p]["step"]) == 2.0 for p in b)
    assert [s["skipped"] for s in got] == [False, True, False] and got[-1]["steps"] == 3 and got[-1]["skipped_steps"] == 1
    for x, y in zip(got, stats):
        assert _bits(x["total_norm"]) == _bits(y["total_norm"]) and (x["coef"] == y["coef"] or x["coef"] != x["coef"])


# ---- the trainer (the set-up of tests/test_gpu_eval_path.py: _trainer) --------------------------------------------------------
def _trainer(amp, graph, guard):
    bench = importlib.import_module("bench")
    from model_train import trainer
    torch.manual_seed(0)
    opt = bench.make_opt(2, height=64, width=96, amp=amp, frame_ids=(0, -1, 1))
    opt.use_automasking, opt.graph, opt.synthetic_length, opt.max_steps, opt.miopen_find = True, graph, 16, 0, False
    opt.noise = "device"
    opt.skip_nonfinite = guard
    tr = trainer(opt)
    tr.setting.set_train()
    batches = list(tr.setting.train_dataloader)[:4]
    torch.manual_seed(1)
    factor = torch.ones((), device=tr.device)               # static: a captured step reads it where it lives
    inner = tr.compute.compute_loss

    def compute_loss(inputs, outputs, setting):
        outputs = inner(inputs, outputs, setting)
        outputs["loss"] = outputs["loss"] * factor
        return outputs
    tr.compute.compute_loss = compute_loss
    return tr, batches, factor


def _trainer_state(tr):
    opt = tr.setting.optim["optimizer"]
    out = []
    for net in tr.setting.raw_model.values():
        for p in net.parameters():
            out.append(p.detach())
            st = opt.state.get(p)
            if st:
                out += [st["exp_avg"], st["exp_avg_sq"], st["step"]]
    return out


@pytest.mark.parametrize("guard", [True, False], ids=["guarded", "unguarded"])
@pytest.mark.parametrize("amp, graph", [("none", False), ("none", True), ("bf16", True)], ids=["f32-eager", "f32-captured", "bf16-captured"])
def test_trainer_survives_an_infinite_loss(amp, graph, guard):
    tr, batches, factor = _trainer(amp, graph, guard)
    opt = tr.setting.optim["optimizer"]
    for b in batches[:2]:
        loss = tr.train_step(dict(b))["loss"]
    assert bool(torch.isfinite(loss))
    assert (tr._graphed is not None) == graph
    live = _trainer_state(tr)
    before = [t.clone() for t in live]
    assert len(before) > 100 and all(bool(torch.isfinite(t).all()) for t in before)
    factor.fill_(float("inf"))
    tr.train_step(dict(batches[2]))
    factor.fill_(1.0)
    torch.cuda.synchronize()
    if not guard:
        assert not opt.guarded
        weights = [p for net in tr.setting.raw_model.values() for p in net.parameters() if p.requires_grad]
        assert not all(bool(torch.isfinite(p).all()) for p in weights)         # the control: the weights are gone
        return
    for i, (t, w) in enumerate(zip(live, before)):
        assert torch.equal(t, w), i
    st = opt.guard_stats()
    assert st["steps"] == 3 and st["skipped_steps"] == 1 and st["skipped"] is True
    loss = tr.train_step(dict(batches[3]))["loss"]
    assert bool(torch.isfinite(loss))
    after = _trainer_state(tr)
    assert all(bool(torch.isfinite(t).all()) for t in after)
    assert sum(int(not torch.equal(t, w)) for t, w in zip(after, before)) > len(before) // 2
    st = opt.guard_stats()
    assert st["steps"] == 4 and st["skipped_steps"] == 1 and st["skipped"] is False and st["total_norm"] > 0


def test_the_epoch_line_reports_the_guard(tmp_path, monkeypatch, capsys):
    bench = importlib.import_module("bench")
    from model_train import trainer
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    opt = bench.make_opt(2, height=64, width=96)
    opt.synthetic_length, opt.max_steps, opt.miopen_find, opt.graph = 8, 2, False, True
    opt.epoch, opt.scheduler_step, opt.save = 2, 1, "guard"
    opt.clip_grad_norm, opt.skip_nonfinite = 1000.0, 1
    tr = trainer(opt)
    tr.train()
    torch.cuda.synchronize()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("step guard:")]
    assert len(lines) == 2 and lines[0].startswith("step guard: 2 steps, 0 skipped, last gradient norm ")
    assert lines[1].startswith("step guard: 4 steps, 0 skipped, last gradient norm ")       # the warm-up's steps are not counted
    st = tr.setting.optim["optimizer"].guard_stats()
    assert st["steps"] == 4 and 0 < st["total_norm"] < float("inf") and 0 < st["coef"] <= 1.0
