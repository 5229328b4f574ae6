"""GPU: what the data-parallel step hands to Adam, parameter by parameter, against the gradient of a plain single-stream step.

The data-parallel step (model_tool/parallel.py, grad_sync) gathers every bucket's gradients into one flat buffer from a
post-accumulate hook and all-reduces it on a stream of its own.  With the pose network beside the depth network
(opt.overlap_pose, the default) backward runs on two streams: the pose network's nodes come first in the forward, so
autograd runs them last, and the hook that completes the last bucket fires on the pose stream while depth-network gradients
may still be in flight on the stream backward() was called on.  The gather must wait for both.  A CPU run
(tests/ddp_worker.py over gloo) has no streams and cannot show a missing wait; the trajectory tests of
tests/test_gpu_driver.py compare one data-parallel run with another, or only losses and parameters.

Here, with a process group of ONE rank over RCCL (the all-reduce of the mean is the identity), every form of the step --
eager with bucketed exchange, captured with the exchange inside the graph, split capture (MDX_DP_SPLIT=1) -- under float32
and under bf16 with shadow weights, with and without a delay:

  * `delayed`: the depth encoder's first convolution -- the one that produces the depth network's LAST weight gradient --
    gets an identity autograd node in front of it whose backward spins SLEEP_CYCLES (~21 ms) on its stream.  That gradient
    is then written long after everything on the pose stream.  (Before the fix the captured forms failed with and without
    the delay; the eager form passed even with it, every bucket issued from the pose stream -- the runtime ordered the
    exchange stream behind backward()'s stream by itself, which nothing guarantees);
  * bit for bit, every form and dtype: after each step the flat buffer's view of each parameter equals the tensor autograd
    produced for it (recorded as the gather is issued; in a captured form the tensors of the capture, which every replay
    rewrites).  This does not depend on the order of MIOpen's atomics;
  * float32, per parameter, each of the 3 steps: what Adam reads (`optimizer.step` wrapped on the instance, copying every
    `p.grad` into a buffer of its own before the real step: capturable, the same wrapper serves the eager step, the full
    capture and graph B of the split form) against a trainer without a process group that runs the pose network after the
    depth network on one stream, eagerly, on the same batches: max|a - b| <= TOL * max|b|.  Steps 2 and 3 run batches the
    graph warm-up never saw.  Adam runs with lr 0: with lr 1e-4 the atomics-order differences of step 1 grow through Adam
    into a spread of 0.13 (step 2) and 0.25 (step 3) between two reference runs, as large as a stale gradient.  Measured on
    an MI355X (2 x 64 x 96, lr 0, max over the 3 steps):
      - spread between fresh reference trainers (three pairs): 1e-5 to 2e-5 in most runs, worst 4.8e-3
        (pose_encoder.encoder.layer2.0.conv2.weight; another run saw 2.5e-3 in the depth encoder at step 1);
      - smallest distance between a reference step-k gradient and its step-(k-1) gradient, k = 2, 3 (what a one-step-stale
        read looks like): 0.063 (decoder.decoder.3.conv.conv.bias, pose_decoder.net.3.bias; most decoder parameters lie
        between 0.06 and 0.3).
    No bar is 10x from both; TOL = 2e-2 sits 4x above the worst spread and 3x below the smallest stale distance
    (test_tolerance_separates_a_stale_gradient keeps a 2x margin to the latter).  A missing wait showed up as far more:
    48 to 71 (parameter, step) pairs of depth-encoder gradients wrong in every element, up to 1.5e6 x max|b|.  bf16 has no bar at all: two
    fresh reference trainers differ by up to 0.89 in a parameter (encoder.encoder.layer4.1.conv2.weight: small gradients
    summed from bf16 terms), more than a stale gradient (0.070); bf16 is checked bit for bit only;
  * the case is exercised: in float32 at least one bucket is issued from a stream other than the one backward() was called
    on (else a pass would prove nothing)."""
import contextlib

import pytest
import torch

from test_gpu_driver import _trainer_losses

pytestmark = pytest.mark.gpu

STEPS = 3
SLEEP_CYCLES = 50000000       # torch.cuda._sleep: 20.8 ms on an MI355X (HIP events: 1e6 cycles 0.42 ms, 5e6 2.09 ms, 1e7 4.17 ms)
TOL = 2e-2                    # float32 (module docstring)
FLOOR = 1e-30                 # a gradient that is zero everywhere: equal means equal
FORMS = ("eager", "full_capture", "split_capture")


@pytest.fixture(scope="module")
def G():
    import gpu_util
    return gpu_util


@contextlib.contextmanager
def _group_of_one():
    """A process group of one rank over RCCL (what tests/test_gpu_driver.py's rccl_group_of_one opens), its rendezvous in an
    in-process store: this module opens a dozen groups in a row, and a TCP port picked free can be taken again before the
    store listens on it (EADDRINUSE)."""
    import torch.distributed as dist
    assert not dist.is_initialized()
    dist.init_process_group("nccl", store=dist.HashStore(), rank=0, world_size=1,
                            device_id=torch.device(torch.cuda.current_device()))
    try:
        yield dist
    finally:
        dist.destroy_process_group()


class _Delay(torch.autograd.Function):
    """Identity; its backward spins SLEEP_CYCLES on its stream before handing the gradient on (one bounded kernel per step)."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        torch.cuda._sleep(SLEEP_CYCLES)
        return g


class _Probe(object):
    """Installed on a trainer before its first step (on_build): per step, a host copy of what Adam read (on_step)."""

    def __init__(self, delay=False):
        self.delay, self.grads = delay, []

    def build(self, tr):
        self.names = ["%s.%s" % (key, n) for key, net in tr.setting.raw_model.items()
                      for n, p in net.named_parameters() if p.requires_grad]
        params = list(tr.setting.parameters)
        assert len(params) == len(self.names)
        bufs = [torch.empty_like(p, dtype=torch.float32) for p in params]
        opt = tr.setting.optim["optimizer"]
        for g in opt.param_groups:
            g["lr"] = 0.0              # parameters stay put: step k's gradient depends on batch k alone (module docstring)
        real = opt.step

        def step(*args, **kwargs):
            grads = [p.grad for p in params]
            missing = [nm for nm, g in zip(self.names, grads) if g is None]
            assert not missing, "no gradient for %s" % missing[:4]
            with torch.no_grad():
                torch._foreach_copy_(bufs, grads)
            return real(*args, **kwargs)

        opt.step = step
        self.bufs = bufs
        if self.delay:
            tr.setting.raw_model["encoder"].encoder.conv1.register_forward_hook(lambda m, i, o: _Delay.apply(o))

    def step(self, i, tr):
        torch.cuda.synchronize()
        self.grads.append([b.cpu() for b in self.bufs])

    def release(self):
        self.bufs = None


def _distance(a, b):
    """max|a - b| / max|b| (0 when both are zero everywhere)."""
    d, s = float((a - b).abs().max()), float(b.abs().max())
    return d / s if s > 0 else (0.0 if d == 0 else float("inf"))


def _mismatches(got, want, tol, what):
    bad = []
    for k in range(STEPS):
        for name, a, b in zip(want.names, got.grads[k], want.grads[k]):
            d, s = float((a - b).abs().max()), float(b.abs().max())
            if not d <= tol * s + FLOOR:
                bad.append("%s, step %d: %s max|a-b| %.3g = %.3g x max|b| (tol %g)" % (what, k + 1, name, d, d / max(s, 1e-38), tol))
    return bad


@pytest.fixture(scope="module")
def reference():
    """amp -> (batches, probe): the plain step -- no process group, the pose network after the depth network, eager."""
    cache = {}

    def get(amp):
        if amp not in cache:
            probe = _Probe()
            _, n, tr = _trainer_losses(False, n=STEPS, amp=amp, overlap_pose=False, on_build=probe.build, on_step=probe.step)
            assert tr.setting.sync is None and tr._graphed is None and tr._pose_stream is None and n == STEPS
            assert len(probe.grads) == STEPS
            probe.release()
            cache[amp] = (tr.last_batches, probe)
        return cache[amp]
    yield get
    cache.clear()


class _Spy(object):
    """Which stream each bucket is issued from, next to the stream the last zero() ran on (the stream backward() is then called
    on: trainer._eager_step / _step_gradients), and the tensors autograd produced for each bucket's parameters."""

    def __init__(self, monkeypatch):
        from model_tool import parallel
        cls = parallel.grad_sync
        real_zero, real_issue, real_gather = cls.zero, cls._issue, cls._issue_on_current
        self.issued, self.produced, self._zero_stream = [], {}, None
        spy = self

        def zero(sync):
            spy._zero_stream = torch.cuda.current_stream().cuda_stream if sync.flat.is_cuda else None
            return real_zero(sync)

        def _issue(sync, k):
            spy.issued.append((k, torch.cuda.current_stream().cuda_stream, spy._zero_stream))
            return real_issue(sync, k)

        def _issue_on_current(sync, k):
            for p in sync.buckets[k][2]:
                if p.grad is not None and p.grad.data_ptr() != sync._views[id(p)].data_ptr():
                    spy.produced[id(p)] = p.grad
            return real_gather(sync, k)

        monkeypatch.setattr(cls, "zero", zero)
        monkeypatch.setattr(cls, "_issue", _issue)
        monkeypatch.setattr(cls, "_issue_on_current", _issue_on_current)

    def exact_mismatches(self, i, tr, names):
        """After step i: every gathered view equals, bit for bit, what autograd produced (eager: in this step; captured: in the
        capture, rewritten by every replay)."""
        torch.cuda.synchronize()
        sync = tr.setting.sync
        name = dict(zip([id(p) for p in tr.setting.parameters], names))
        assert len(self.produced) == len(sync.params), (len(self.produced), len(sync.params))
        bad = []
        for pid, t in self.produced.items():
            v = sync._views[pid]
            if not torch.equal(v, t):
                bad.append("step %d: %s: %d / %d elements of the flat buffer differ from autograd's gradient" % (
                    i + 1, name[pid], int((v != t).sum()), t.numel()))
        return bad


def _run_form(form, amp, delay, batches, spy, monkeypatch):
    if form == "split_capture":
        monkeypatch.setenv("MDX_DP_SPLIT", "1")
    else:
        monkeypatch.delenv("MDX_DP_SPLIT", raising=False)
    monkeypatch.delenv("MDX_DP_GRAPH", raising=False)
    probe, exact = _Probe(delay), []

    def on_step(i, tr):
        probe.step(i, tr)
        exact.extend(spy.exact_mismatches(i, tr, probe.names))

    with _group_of_one():
        _, n, tr = _trainer_losses(form != "eager", n=STEPS, amp=amp, batches=batches, on_build=probe.build, on_step=on_step)
        sync = tr.setting.sync
        try:
            assert sync is not None and sync.backend == "nccl" and n == STEPS and tr._pose_stream is not None
            if form == "eager":
                assert tr._graphed is None and len(sync.buckets) >= 2
            else:
                assert tr._graphed is not None and len(sync.buckets) == 1
                assert tr._graphed.split == (form == "split_capture")
            pose = tr._pose_stream.cuda_stream
        finally:
            sync.detach()
            spy.produced = {}
    probe.release()
    return probe, exact, pose


@pytest.mark.parametrize("delay", [False, True], ids=["undelayed", "delayed"])
@pytest.mark.parametrize("amp", ["none", "bf16"])
@pytest.mark.parametrize("form", FORMS)
def test_adam_reads_the_single_stream_gradients(G, reference, monkeypatch, form, amp, delay):
    batches, want = reference(amp)
    spy = _Spy(monkeypatch)
    got, exact, pose = _run_form(form, amp, delay, batches, spy, monkeypatch)
    what = "%s amp=%s %s" % (form, amp, "delayed" if delay else "undelayed")
    assert not exact, "%s: the gather read gradients before backward wrote them (%d):\n  %s" % (
        what, len(exact), "\n  ".join(exact[:12]))
    if amp == "none":
        bad = _mismatches(got, want, TOL, what)
        assert not bad, "%d parameter gradients differ from the single-stream step's:\n  %s" % (len(bad), "\n  ".join(bad[:12]))
        off = [k for k, s, z in spy.issued if s != z]
        assert off, "%s: every bucket was issued from the stream backward() ran on -- the two-stream case was not exercised " \
                    "(issued: %s, pose stream %s)" % (what, spy.issued[-4:], pose)


def test_tolerance_separates_a_stale_gradient(G, reference):
    """The bar of the float32 comparison would see a gradient one step stale: every parameter's step-k gradient differs from its
    step-(k-1) gradient by more than 2 x TOL (the batches differ from step to step; measured: 0.063 at the closest)."""
    _, want = reference("none")
    close = []
    for k in range(1, STEPS):
        for name, a, b in zip(want.names, want.grads[k - 1], want.grads[k]):
            d = _distance(a, b)
            if not d > 2 * TOL:
                close.append("steps %d / %d: %s %.3g" % (k, k + 1, name, d))
    assert not close, "gradients too close from one step to the next for TOL %g:\n  %s" % (TOL, "\n  ".join(close[:12]))
