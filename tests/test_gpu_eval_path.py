"""GPU: evaluation mode on the hand-written path.  (1) The encoders in eval mode run their batch norms as the fused eval kernel
(csrc/norm_infer.hip) -- torch's batch_norm is never called -- and give the torch-op path's features, fp32 and bf16, planar and
channels-last, ResNet-18 and ResNet-50, without touching the running statistics.  (2) model_test.inference gives the same
metrics either way.  (3) The trainer's captured validation step (model_train.graphed_valid_step) gives the eager step's loss and
metrics, also after the weights have moved.  (4) A whole run with and without it ends in the same state.  (5) --noise cpu
validates eagerly."""
import importlib
import os

import numpy as np
import pytest
import torch

importlib.import_module("digging-into-self-supervised-monocular-depth-estimation_amd")
from model_layer import depth_encoder  # noqa: E402
from model_layer.depth_encoder import BatchNorm2d, ResnetEncoder  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _randomise_batch_norms(net, seed):
    """Random running statistics and affine parameters: the defaults (mean 0, var 1, gamma 1, beta 0) would hide a wrong fold."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, BatchNorm2d):
                n = m.num_features
                u = lambda lo, hi: (lo + (hi - lo) * torch.rand(n, generator=g)).to(m.weight.device)   # noqa: E731
                m.running_mean.copy_(u(-0.5, 0.5))
                m.running_var.copy_(u(0.5, 2.0))
                m.weight.copy_(u(0.5, 1.5))
                m.bias.copy_(u(-0.3, 0.3))


def _state(net):
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


def _bf16_ulp(t):
    """Element-wise bfloat16 ulp of |t| (0 where t is 0)."""
    v = t.abs().to(torch.bfloat16).double()
    _, e = torch.frexp(v)
    return torch.where(v == 0, torch.zeros_like(v), torch.ldexp(torch.ones_like(v), e - 8))


@pytest.mark.parametrize("amp", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("plan", ["all", "none"])
@pytest.mark.parametrize("layers", [18, 50])
def test_eval_encoder_runs_the_fused_kernel(layers, plan, amp, monkeypatch):
    from mdx.layout import apply_plan
    torch.manual_seed(layers)
    enc = ResnetEncoder(layers, False).to(DEV)
    apply_plan({"encoder": enc}, plan)
    _randomise_batch_norms(enc, layers + 1)
    enc.eval()
    x = torch.rand(2, 3, 96, 320, device=DEV)
    before = _state(enc)

    def run(amp=amp):
        with torch.no_grad(), torch.autocast(device_type="cuda", dtype=torch.bfloat16, enabled=amp):
            return [f.float().clone() for f in enc(x)]

    def no_torch_batch_norm(*a, **k):
        raise AssertionError("torch.nn.functional.batch_norm called in eval mode")
    with monkeypatch.context() as m:
        m.setattr(depth_encoder.TF, "batch_norm", no_torch_batch_norm)
        fused = run()
    with monkeypatch.context() as m:
        m.setattr(BatchNorm2d, "fused_eval", False)
        plain = run()
        ref = run(False)                    # the float32 network, torch ops
    torch.cuda.synchronize()
    assert len(fused) == len(plain) == 5
    for k, (a, b) in enumerate(zip(fused, plain)):
        assert a.shape == b.shape and bool(torch.isfinite(a).all())
        err = float((a - b).abs().max())
        if not amp:
            # per layer: 1e-5 of |x s| + |t| + |res|; through the convolutions of the network the same bound on the map's scale
            tol = 1e-5 * float(b.abs().max()) + 1e-7
            assert err <= tol, "feature %d: max |fused - torch ops| %g > %g" % (k, err, tol)
        elif k == 0:
            # the stem: one batch norm behind the same convolution -- within two bf16 ulps element by element (the torch-op path
            # rounds twice)
            bad = (a - b).abs().double() > 2 * _bf16_ulp(torch.maximum(a.abs(), b.abs()))
            assert not bool(bad.any()), "stem: %d elements more than two bf16 ulps from the torch-op path" % int(bad.sum())
        else:
            # deeper, every bf16 convolution re-rounds what the layers before it left, and a one-ulp difference grows: both bf16
            # paths are held to the float32 network instead -- the fused one no farther from it than twice the torch-op path
            e_f, e_t = float((a - ref[k]).abs().max()), float((b - ref[k]).abs().max())
            assert e_f <= 2 * e_t + 1e-6, "feature %d: fused %g, torch ops %g from the float32 network" % (k, e_f, e_t)
    after = _state(enc)
    for k in before:
        assert torch.equal(before[k], after[k]), "%s changed in eval mode" % k
    assert all(m._pending_batches == 0 for m in enc.modules() if isinstance(m, BatchNorm2d))


def test_inference_metrics_match_the_torch_op_path(tmp_path, monkeypatch):
    import fake_kitti
    import model_test
    from model_layer import DepthDecoder
    bench = importlib.import_module("bench")
    names = fake_kitti.make(str(tmp_path), n_frames=6)
    os.makedirs(os.path.join(str(tmp_path), "splits", "fake"))
    for split in ("train", "val", "test"):
        open(os.path.join(str(tmp_path), "splits", "fake", split + "_files.txt"), "w").write("\n".join(names) + "\n")
    opt = bench.make_opt(2, height=192, width=640)
    opt.dataset, opt.datapath, opt.splits, opt.datatype = "kitti_mono", str(tmp_path), os.path.join(str(tmp_path), "splits"), "fake"
    torch.manual_seed(0)
    enc = ResnetEncoder(18, False)
    dec = DepthDecoder(enc.num_ch_enc)
    _randomise_batch_norms(enc, 3)
    fused = model_test.inference(opt, encoder=enc, decoder=dec)
    with monkeypatch.context() as m:
        m.setattr(BatchNorm2d, "fused_eval", False)
        plain = model_test.inference(opt, encoder=enc, decoder=dec)
    assert set(fused) == set(model_test.METRICS)
    for k in model_test.METRICS:
        assert np.isfinite(fused[k]) and abs(fused[k] - plain[k]) <= 1e-4 * max(1.0, abs(plain[k])), (k, fused[k], plain[k])


# ---- the trainer (the set-up of tests/test_gpu_driver.py:_trainer_losses) -----------------------------------------------
def _trainer(amp="none", frame_ids=(0, -1, 1), noise="device", graph=True):
    bench = importlib.import_module("bench")
    from model_train import trainer
    torch.manual_seed(0)
    opt = bench.make_opt(2, height=64, width=96, amp=amp, frame_ids=frame_ids)
    opt.use_automasking, opt.graph, opt.synthetic_length, opt.max_steps, opt.miopen_find = True, graph, 16, 0, False
    opt.noise = noise
    tr = trainer(opt)
    tr.setting.set_train()
    batches = list(tr.setting.train_dataloader)[:8]
    torch.manual_seed(1)
    return tr, batches


def _train(tr, batches):
    tr.setting.set_train()
    for b in batches:
        tr.train_step(dict(b))


def _validate(tr, batches, captured):
    """[loss + seven metrics] per batch (float32 bits) and the noise offset afterwards."""
    tr.opt.graph_valid = captured
    tr.setting.set_valid()
    names = tr.control.metric_name
    rows = []
    with torch.no_grad():
        for b in batches:
            # uploaded as the trainer's prefetcher does (the ground truth included: control.metric then runs the GPU monitor)
            b = {k: (v.to(tr.device) if torch.is_tensor(v) and tr.compute._step_reads(k) else v) for k, v in b.items()}
            log = tr.control.metric(b, tr.valid_step(b), {k: [] for k in names})
            assert all(len(log[k]) == 1 for k in names), "the synthetic batch carries ground truth: all eight values"
            rows.append(np.array([float(log[k][0]) for k in names], np.float32))
    torch.cuda.synchronize()
    return np.stack(rows).view(np.uint32), tr.compute.noise_offset()


def _eager_then_captured(tr, batches):
    start = tr.compute.noise_offset()
    eager, off_e = _validate(tr, batches, False)
    tr.compute.set_noise_offset(start)
    captured, off_c = _validate(tr, batches, True)
    assert off_e == off_c == start + len(batches), (start, off_e, off_c)
    return eager, captured


def _close(a, b, rtol):
    """loss, abs_rel, sq_rel, rmse, rmse_log within rtol; a1-a3 (fractions of the ground-truth pixels) within a few pixels.  Not bit
    for bit: two passes of ONE network over ONE batch already differ in the last bits here -- MIOpen's convolution kernels are not
    run-to-run deterministic (LABNOTES round 3), eager or replayed alike."""
    a, b = a.view(np.float32).astype(np.float64), b.view(np.float32).astype(np.float64)
    ok = np.abs(a[:, :5] - b[:, :5]) <= rtol * np.abs(b[:, :5])
    return bool(ok.all() and (np.abs(a[:, 5:] - b[:, 5:]) <= 2e-3).all())


@pytest.mark.parametrize("amp, frame_ids", [("none", (0, -1, 1)), ("bf16", (0, -1, 1)), ("none", (0, -1, 1, "s"))],
                         ids=["f32", "bf16", "stereo"])
def test_captured_validation_equals_eager(amp, frame_ids):
    rtol = 2e-5 if amp == "none" else 2e-4
    tr, batches = _trainer(amp, frame_ids)
    assert tr.compute.draws_in_kernel()
    _train(tr, batches[:2])
    eager, captured = _eager_then_captured(tr, batches[2:5])
    assert tr._graphed_valid is not None and tr._graphed_valid.replays == 3
    assert _close(captured, eager, rtol), (eager.view(np.float32), captured.view(np.float32))
    # the weights move (Adam, in place): the graph reads them where they live -- under bf16 the weight shadows are re-made inside
    # it; a graph that replayed weights cast before the capture would keep the old losses
    _train(tr, batches[5:6])
    eager2, captured2 = _eager_then_captured(tr, batches[2:5])
    assert tr._graphed_valid.replays == 6
    moved = abs(eager2.view(np.float32)[:, 0].mean() - eager.view(np.float32)[:, 0].mean())
    assert moved > 5 * rtol * abs(eager.view(np.float32)[:, 0].mean()), "the training step hardly changed the validation loss"
    assert _close(captured2, eager2, rtol), (eager2.view(np.float32), captured2.view(np.float32))


def test_train_with_and_without_captured_validation_ends_in_one_state(tmp_path, monkeypatch):
    """Validation changes nothing a run carries on with: the same parameters, batch-norm statistics and counters, Adam state, noise
    offset and logs with the validation step captured or eager -- up to MIOpen's run-to-run differences, which two trainers
    started from one seed show in their first training loss already (hence tolerances; the noise offset and the counters exact)."""
    bench = importlib.import_module("bench")
    from model_train import trainer
    monkeypatch.chdir(tmp_path)

    def run(graph_valid):
        torch.manual_seed(0)
        opt = bench.make_opt(2, height=64, width=96)
        opt.synthetic_length, opt.max_steps, opt.miopen_find, opt.graph = 8, 3, False, True
        opt.epoch, opt.scheduler_step, opt.save, opt.graph_valid = 2, 1, "gv%d" % graph_valid, graph_valid
        tr = trainer(opt)
        logs = []
        original = tr.control.print
        tr.control.print = lambda epoch, t, v: (logs.append((epoch, dict(t), dict(v))), original(epoch, t, v))[1]
        tr.train()
        torch.cuda.synchronize()
        state = {}
        for key, net in tr.setting.raw_model.items():
            for k, v in net.state_dict().items():
                state[key + "." + k] = v.detach().clone()
        adam = tr.setting.optim["optimizer"].state_dict()["state"]
        for i, st in adam.items():
            for k, v in st.items():
                state["adam.%s.%s" % (i, k)] = v.detach().clone() if torch.is_tensor(v) else torch.tensor(float(v))
        return tr, logs, state

    tv, logs_v, state_v = run(True)
    te, logs_e, state_e = run(False)
    assert tv._graphed_valid is not None and tv._graphed_valid.replays == 6      # 3 validation batches x 2 epochs
    assert te._graphed_valid is None and te._graphed is not None and tv._graphed is not None
    assert tv.compute.noise_offset() == te.compute.noise_offset() == 12          # 6 training + 6 validation steps
    assert [e for e, _, _ in logs_v] == [e for e, _, _ in logs_e] == [0, 1]
    for (_, tv_, vv), (_, te_, ve) in zip(logs_v, logs_e):
        for got, want in ((tv_, te_), (vv, ve)):
            row = lambda d: np.array([[d[k] for k in tv.control.metric_name]], np.float32).view(np.uint32)   # noqa: E731
            assert _close(row(got), row(want), 1e-3), (got, want)      # measured: 1.4e-4 on the second epoch's training loss
    assert set(state_v) == set(state_e)
    for k in state_v:
        a, b = state_v[k], state_e[k]
        if not a.is_floating_point() or k.endswith(".step"):
            assert torch.equal(a, b), k                  # batch counters, Adam's step counts
        elif "running_" in k:
            # the training runs drift apart by up to 2e-3 of a map's running mean (layer4, measured); ONE eval-mode update of the
            # statistics would move them by momentum 0.1 x (batch mean - running mean), a multiple of this bound
            assert float((a - b).abs().max()) <= 2e-2 * float(b.abs().max()) + 1e-12, k
        elif ".exp_avg" in k:
            # Adam's moments follow the gradients' drift between two runs (measured: 4-10 % of a tensor's largest moment), so
            # they bound nothing here; an extra optimiser step would show in the exact step counts above
            assert bool(torch.isfinite(a).all()), k
        else:                                            # parameters: six Adam steps of lr 1e-4 bound any difference by 6e-4
            assert float((a - b).abs().max()) <= 1e-3, k


def test_host_noise_validates_eagerly():
    tr, batches = _trainer(noise="cpu")
    assert not tr.can_graph()
    _train(tr, batches[:1])
    rows, _ = _validate(tr, batches[1:2], True)
    assert tr._graphed_valid is None
    assert np.isfinite(rows.view(np.float32)).all()
