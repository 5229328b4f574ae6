"""Training entry (reference: model_train.py:24-101): `trainer(options()).train()`, one process per GPU.

    python model_train.py --dataset synthetic --epoch 1
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 model_train.py ...
"""
import contextlib
import json
import os
import sys

# Data-parallel runs: the captured step's streams (the capture stream, the pose network's side stream, the gradient exchange, RCCL's
# own, the prefetcher's uploads + image preparation) are mapped onto the HIP runtime's hardware queues, 4 per device by default,
# and which two share one decides what overlaps.  Measured with a process group of one rank (round 5, pose network beside the
# depth network, images/s resident | DataLoader-fed loop): 2 queues 742 | 722 (bf16 1475 | 1412), 4 queues 744 | 669 (1487 |
# 1248), 8 queues 514 | 723; an EAGER data-parallel step is the opposite (2: 686, 4: 625, 8: 733) and host-bound besides.  So a
# captured data-parallel run asks for 2.  The runtime reads the variable when it is loaded, i.e. before `import torch`.
# MDX_HW_QUEUES=0 leaves the runtime's default, MDX_HW_QUEUES=n asks for n; a value the user exported (GPU_MAX_HW_QUEUES) is never
# overridden.  (Round 3's sweep, before the side streams: LABNOTES.md.)
def _graph_requested(argv):
    for i, a in enumerate(argv):
        v = a.split("=", 1)[1] if a.startswith("--graph=") else (argv[i + 1] if a == "--graph" and i + 1 < len(argv) else None)
        if v is not None:
            return str(v).lower() in ("1", "true", "yes")
    return True


# (only when this file is the program: imported by another one -- bench.py -- the runtime is loaded already and the variable
# would merely leak into that program's child processes)
if os.path.basename(sys.argv[0] or "") == "model_train.py" and os.environ.get("MDX_HW_QUEUES", "") != "0" and (
        os.environ.get("MDX_HW_QUEUES") or (int(os.environ.get("WORLD_SIZE", "1")) > 1 and _graph_requested(sys.argv[1:]))):
    os.environ.setdefault("GPU_MAX_HW_QUEUES", os.environ.get("MDX_HW_QUEUES") or "2")

import numpy as np        # noqa: E402
import torch              # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from model_option import options      # noqa: E402
from model_tool import *              # noqa: E402,F401,F403


class device_prefetcher(object):
    """Iterates a DataLoader one batch ahead: the entries a step reads (compute._step_reads) of batch i+1 are copied
    host -> device on a SIDE stream while step i computes (the loader pins its batches), so the PCIe transfer
    (~0.13 GB per batch of 12 at 192x640) is off the critical path.  The reference copies every key at the start of
    each step on the compute stream (processor.py:34-35)."""

    def __init__(self, loader, device, wanted, prepare=None):
        self.loader, self.device, self.wanted, self.prepare = loader, device, wanted, prepare
        self.stream = torch.cuda.Stream(device) if str(device).startswith("cuda") else None

    def _upload(self, batch):
        if self.stream is None or batch is None:
            return batch
        with torch.cuda.stream(self.stream):
            batch = {k: (v.to(self.device, non_blocking=True) if torch.is_tensor(v) and self.wanted(k) else v)
                     for k, v in batch.items()}
            # decoded frames -> the step's entries (compute.prepare), also on the side stream
            return self.prepare(batch) if self.prepare is not None else batch

    def __iter__(self):
        it = iter(self.loader)
        nxt = self._upload(next(it, None))
        while nxt is not None:
            if self.stream is not None:
                torch.cuda.current_stream(self.device).wait_stream(self.stream)
                for v in nxt.values():
                    if torch.is_tensor(v) and v.is_cuda:
                        v.record_stream(torch.cuda.current_stream(self.device))
            cur, nxt = nxt, self._upload(next(it, None))
            yield cur


def _plain(v):
    """A captured step's outputs as plain tensors (detached, containers kept)."""
    if torch.is_tensor(v):
        return v.detach()
    if isinstance(v, (list, tuple)):
        return type(v)(_plain(x) for x in v)
    return v


def _static_keys(tr):
    """The batch entries a captured step reads, copied into its static buffers (the velodyne ground truth is read by
    control.metric from the batch itself and not by the step -- unless --depth_supervision puts it into the loss: then it is a
    static buffer like the others, copied per replay)."""
    supervised = float(getattr(tr.opt, "depth_supervision", 0.0) or 0.0) > 0
    return lambda k: tr.compute._step_reads(k) and (supervised or not (isinstance(k, tuple) and k[0] == "depth"))


class graphed_step(object):
    """One training step (networks, the photometric kernels launched through the C-ABI, the gradient all-reduce of a
    data-parallel job, fused Adam) captured into ONE hipGraph and replayed: ~1600 kernel launches leave the host's
    critical path, so the step stays GPU-bound while the host decodes and collates the next batches (measured: with 12
    loader workers alive the eager step needs 24.5 ms of host time for 20.7 ms of GPU time).  Inputs live in static
    device buffers the batch is copied into; the outputs the loop reads afterwards (loss, depth of scale 0, auto-masks)
    are the graph's own tensors.  What Python does during a step and a replay would skip is re-applied per replay: the
    batch-norm step counters.  Under torch.distributed the exchange (model_tool/parallel.py: bucketed RCCL all-reduce
    issued from inside backward) is part of the graph.  Any change of the learning rate goes through set_lr (a device
    tensor the captured Adam reads).

    The warm-up steps capture needs (MIOpen picks its kernels, the allocator settles, RCCL opens its communicator) are
    side-effect free: weights, batch-norm statistics, Adam moments, step counters and the offset of the in-kernel noise
    generator are put back afterwards, so the first replay is step 1 of the run -- graph on and graph off follow the same
    trajectory and draw the same noise.

    The step guard (--clip_grad_norm, --skip_nonfinite) is part of optimizer.step(): it runs after the gradient exchange, on the
    exchanged gradients, so every rank sees the same bits and takes the same decision; in the split form it is part of graph B.
    Its totals are put back after the warm-up with the moments and step counters.

    The weight average (--ema_decay) is updated directly after optimizer.step(), inside the same graph (graph B in the split form);
    its shadows and counters are put back after the warm-up too, so the first replay is update 0 from shadows equal to the
    initial weights."""

    def __init__(self, tr, example, warmup=3):
        self.tr = tr
        dev = tr.device
        # several ranks without MDX_DP_GRAPH=1: the SPLIT form -- graph A = forward, backward, gradients gathered into the flat
        # buffer; the all-reduce issued eagerly between the replays (RCCL never inside a capture: a captured multi-rank exchange
        # has not run on hardware); graph B = Adam.  Two graph launches and one collective per step on the host instead of ~1900
        # kernel launches (an eager data-parallel step is host-bound since the pose network runs beside the depth network).
        from model_tool.parallel import dp_graph_allowed
        sync = tr.setting.sync
        self.split = sync is not None and (not dp_graph_allowed(sync.world) or os.environ.get("MDX_DP_SPLIT", "") == "1")
        opt = tr.setting.optim["optimizer"]
        self.lr = torch.tensor(float(opt.param_groups[0]["lr"]), device=dev)
        for g in opt.param_groups:
            g["capturable"] = True
            g["lr"] = self.lr
        wanted = _static_keys(tr)
        self.static = {k: (v.to(dev).clone() if torch.is_tensor(v) and wanted(k) else v) for k, v in example.items()}
        self.copied = {k for k, v in example.items() if torch.is_tensor(v) and wanted(k)}
        from model_layer.depth_encoder import BatchNorm2d
        nets = list(tr.setting.raw_model.values())
        self.bns = [m for net in nets for m in net.modules() if isinstance(m, BatchNorm2d)]
        # ---- snapshot of everything a training step changes ----
        tensors = [t for net in nets for t in list(net.parameters()) + list(net.buffers())]
        saved = [t.detach().clone() for t in tensors]
        saved_bn = [m._pending_batches for m in self.bns]
        # the in-kernel noise generator's {seed, offset}: every warm-up step advances the offset on the device
        rng = tr.compute.noise_rng(dev) if tr.compute.draws_in_kernel() else None
        saved_rng = rng.tensor.clone() if rng is not None else None
        had_state = {id(p): {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in st.items()}
                     for p, st in opt.state.items()}
        saved_guard = opt.guard_snapshot() if getattr(opt, "guarded", False) else None     # the step guard's totals (mdx/optim.py)
        ema = tr.setting.optim.get("ema")          # the weight average (mdx/optim.py: WeightEMA): the warm-up's updates are undone
        saved_ema = ema.snapshot() if ema is not None else None
        # ONE side stream for the warm-up and the capture: the gradient-accumulation nodes autograd creates during
        # the captured forward then live on the stream that produces their gradients
        self.stream = torch.cuda.Stream(dev)
        self.stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(self.stream):
            for _ in range(warmup):
                tr._eager_step(dict(self.static))
            with torch.no_grad():
                for t, v in zip(tensors, saved):
                    t.copy_(v)
                for p, st in opt.state.items():
                    old = had_state.get(id(p))
                    for k, v in st.items():
                        if torch.is_tensor(v):
                            if old is not None and k in old:
                                v.copy_(old[k])
                            else:
                                v.zero_()          # Adam's initial state: zero moments, step 0
                if rng is not None:
                    rng.tensor.copy_(saved_rng)
                if saved_guard is not None:
                    opt.guard_restore(saved_guard)
                if saved_ema is not None:
                    ema.restore(saved_ema)
            for m, n in zip(self.bns, saved_bn):
                m._pending_batches = n
        torch.cuda.current_stream(dev).wait_stream(self.stream)
        torch.cuda.synchronize(dev)
        del saved, had_state
        before = [m._pending_batches for m in self.bns]
        self.graph = torch.cuda.CUDAGraph()
        # thread_local: the DataLoader's pin-memory thread keeps allocating pinned host buffers for the next batches
        # (and RCCL's watchdog thread polls events) while this thread captures; in the default "global" mode such a
        # call from ANY thread invalidates the capture
        self.graph_apply = None
        if self.split:
            with torch.cuda.graph(self.graph, stream=self.stream, capture_error_mode="thread_local"):
                outputs = tr._step_gradients(dict(self.static))
            self.graph_apply = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph_apply, stream=self.stream, capture_error_mode="thread_local", pool=self.graph.pool()):
                tr._apply_step()
        else:
            with torch.cuda.graph(self.graph, stream=self.stream, capture_error_mode="thread_local"):
                outputs = tr._eager_step(dict(self.static))
        # the graph's output tensors, without the autograd graph behind them: a loss that kept its grad_fn would keep the
        # capture pass's gradient-accumulation nodes (created on the capture stream) alive into later eager steps
        self.outputs = {k: _plain(v) for k, v in outputs.items()}
        del outputs
        self.bn_incr = [m._pending_batches - b for m, b in zip(self.bns, before)]
        for m, b in zip(self.bns, before):         # the capture pass ran no kernel: it was not a step
            m._pending_batches = b
        torch.cuda.synchronize(dev)

    def set_lr(self, value):
        self.lr.fill_(float(value))

    def __call__(self, inputs):
        for k, v in inputs.items():
            if k in self.copied and torch.is_tensor(v):
                self.static[k].copy_(v, non_blocking=True)
        self.graph.replay()
        if self.graph_apply is not None:
            self.tr.setting.sync.exchange()
            self.graph_apply.replay()
        for m, inc in zip(self.bns, self.bn_incr):
            m._pending_batches += inc
        return self.outputs


class graphed_valid_step(object):
    """The validation step -- torch.no_grad(), the networks in eval mode (batch norm as csrc/norm_infer.hip with the running
    statistics), the forward-only form of the loss kernels -- captured into ONE hipGraph of its own and replayed: a few hundred
    mostly small launches leave the host, as graphed_step does for the training step.  Same contract: the batch is copied into
    static device buffers, the outputs are the graph's own tensors (detached), control.metric reads them on the main stream.
    Its own memory pool; no collective inside (the epoch means' all-reduce stays where it is).  The warm-up passes the capture
    needs draw auto-mask noise, so the generator's offset is put back afterwards: every replay then advances it exactly as one
    eager validation step does.  Weights are read where they live: the training updates them in place, and under --amp bf16 the
    weight shadows (mdx/shadow.py) are re-made inside the graph at every replay."""

    def __init__(self, tr, example, warmup=2):
        self.tr = tr
        dev = tr.device
        self.wanted = wanted = _static_keys(tr)
        self.static = {k: (v.to(dev).clone() if torch.is_tensor(v) and wanted(k) else v) for k, v in example.items()}
        self.copied = {k for k, v in example.items() if torch.is_tensor(v) and wanted(k)}
        tr.setting.set_valid()
        rng = tr.compute.noise_rng(dev) if tr.compute.draws_in_kernel() else None
        saved_rng = rng.tensor.clone() if rng is not None else None
        self.stream = torch.cuda.Stream(dev)
        self.stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.no_grad():
            with torch.cuda.stream(self.stream):
                for _ in range(warmup):
                    tr.batch_process(dict(self.static))
                if rng is not None:
                    rng.tensor.copy_(saved_rng)
            torch.cuda.current_stream(dev).wait_stream(self.stream)
            torch.cuda.synchronize(dev)
            self.graph = torch.cuda.CUDAGraph()
            # thread_local: see graphed_step (the loader's pin-memory thread allocates while this thread captures)
            with torch.cuda.graph(self.graph, stream=self.stream, capture_error_mode="thread_local"):
                outputs = tr.batch_process(dict(self.static))
        self.outputs = {k: _plain(v) for k, v in outputs.items()}
        del outputs
        torch.cuda.synchronize(dev)
        self.replays = 0

    def matches(self, inputs):
        """Does the batch fit the static buffers (same entries, same shapes and dtypes)?"""
        have = {k for k, v in inputs.items() if torch.is_tensor(v) and self.wanted(k)}
        return have == self.copied and all(inputs[k].shape == self.static[k].shape and inputs[k].dtype == self.static[k].dtype
                                           for k in self.copied)

    def __call__(self, inputs):
        for k in self.copied:
            self.static[k].copy_(inputs[k], non_blocking=True)
        self.graph.replay()
        self.replays += 1
        return self.outputs


class trainer(object):
    def __init__(self, opt):
        self.opt = opt
        self._graphed = None
        self._graphed_valid = None
        # --grad_stats: the passes issued so far, how many of them did not take the kernels, and {pass: training step} for the
        # passes a report may have to name (grad_stats_report drops the others)
        self._grad_stat_passes, self._grad_stat_torch, self._grad_stat_steps = 0, 0, {}
        # --loss_stats: the passes issued since the last report (the history is reset with every report), how many of them did not
        # take the kernels, {pass: training step} for them, and the passes of the whole run
        self._loss_stat_passes, self._loss_stat_torch, self._loss_stat_steps, self._loss_stat_total = 0, 0, {}, 0
        # --depth_supervision: the epoch's sums of the term and of the valid pixels, kept on the device, and the steps behind them
        self._depth_acc, self._depth_steps = None, 0
        # --stereo_hints: the same sums for the hint term
        self._hint_acc, self._hint_steps = None, 0
        world = int(os.environ.get("WORLD_SIZE", "1"))
        local = int(os.environ.get("LOCAL_RANK", "0"))
        if torch.cuda.is_available():
            local = local % torch.cuda.device_count()     # a rehearsal may run several ranks on one GPU (gloo backend)
            self.device = "cuda:%d" % local
            torch.cuda.set_device(local)
        else:
            self.device = "cpu"
        if world > 1 and not torch.distributed.is_initialized():
            if torch.cuda.is_available():
                torch.distributed.init_process_group(os.environ.get("MDX_DIST_BACKEND", "nccl"),
                                                     device_id=torch.device(self.device))
            else:
                torch.distributed.init_process_group("gloo")
        self.rank = int(os.environ.get("RANK", "0"))
        from mdx.tuning import install_miopen_db
        install_miopen_db(self.rank)          # tuned conv / batch-norm solvers for the default shapes (immediate mode)
        torch.backends.cudnn.benchmark = bool(getattr(opt, "miopen_find", False))
        self.setting = setting(opt, self.device)
        self.compute = compute(opt, self.device)
        self.control = control(opt, self.device)

    _pose_stream = None

    def _pose_beside_depth(self):
        return (bool(getattr(self.opt, "overlap_pose", True)) and str(self.device).startswith("cuda")
                and self.opt.pose_type in ("separate", "posecnn") and torch.is_grad_enabled())

    def batches(self, loader):
        """The loader's batches, uploaded one step ahead on a side stream (GPU) or as they are (CPU)."""
        if str(self.device).startswith("cuda") and getattr(self.opt, "device_prefetch", True):
            return device_prefetcher(loader, self.device, self.compute._step_reads, self.compute.prepare)
        return loader

    def batch_process(self, inputs):
        # bf16 networks: every convolution weight cast ONCE, by one launch, before the two networks fork (and the weight gradients
        # back by one launch at the end of backward) instead of by autocast around each convolution (mdx/shadow.py)
        # (validation, torch.no_grad(): the same one launch, no autograd node)
        if (self.compute.amp == "bf16" and str(self.device).startswith("cuda")
                and getattr(self.opt, "shadow_weights", True)):
            from mdx.shadow import bf16_weights
            with bf16_weights(self.setting.raw_model.values()):
                return self._batch_process(inputs)
        return self._batch_process(inputs)

    def _batch_process(self, inputs):
        outputs = {}
        if self._pose_beside_depth():
            # the separate pose network does not depend on the depth network: it runs on a side stream beside it (forward here,
            # backward likewise -- autograd runs a node's backward on its forward's stream); many of both networks' kernels are
            # too small to fill the GPU on their own
            inputs = self.compute.stage_inputs(inputs)
            cur = torch.cuda.current_stream(self.device)
            if self._pose_stream is None:
                self._pose_stream = torch.cuda.Stream(self.device)
                if self.setting.sync is not None:
                    self.setting.sync.backward_streams([self._pose_stream])
            self._pose_stream.wait_stream(cur)
            with torch.cuda.stream(self._pose_stream):
                inputs, outputs = self.compute.forward_pose(inputs, outputs, self.setting)
            inputs, outputs = self.compute.forward_depth(inputs, outputs, self.setting)
            self.compute.loss_prologue(inputs, outputs)       # what the loss needs of the batch and the disparities alone
            cur.wait_stream(self._pose_stream)
        else:
            inputs, outputs = self.compute.forward_depth(inputs, outputs, self.setting)
            inputs, outputs = self.compute.forward_pose(inputs, outputs, self.setting)
        inputs, outputs = self.compute.image2warping(inputs, outputs, self.setting)
        outputs = self.compute.compute_loss(inputs, outputs, self.setting)
        return outputs

    def _step_gradients(self, inputs):
        """The step up to its gradients, gathered into the flat buffer and NOT exchanged (graph A of graphed_step's split form)."""
        outputs = self.batch_process(inputs)
        sync = self.setting.sync
        sync.zero()
        with sync.gather_only():
            outputs["loss"].backward()
            sync.finish()
        return outputs

    def _eager_step(self, inputs):
        """forward, backward, (data parallel: gradient all-reduce, overlapped with backward), Adam."""
        outputs = self.batch_process(inputs)
        sync = self.setting.sync
        if sync is None:
            self.setting.optim["optimizer"].zero_grad(set_to_none=True)
        else:
            sync.zero()                    # the gradients are views into one flat buffer: one memset
        outputs["loss"].backward()
        if sync is not None:
            sync.finish()
        self._apply_step()
        return outputs

    def _apply_step(self):
        """Adam, then the weight average's update (--ema_decay), which reads the guard's decision where the optimiser left it."""
        optimizer = self.setting.optim["optimizer"]
        optimizer.step()
        ema = self.setting.optim.get("ema")
        if ema is not None:
            ema.update(optimizer)

    _weight_checks = 0

    def check_weights(self):
        """--check_weights: digest the float32 master weights where they live and compare the digests across the ranks
        (model_tool/parallel.py: check_replicas; raises ReplicaMismatch on every rank).  Eager launches on the current stream -- the
        one the step ran on or was replayed on -- between the replays of a captured step, never inside a graph."""
        digest = self.setting.optim.get("digest")
        if digest is not None:
            from model_tool.parallel import check_replicas
            check_replicas(digest)
            self._weight_checks += 1

    def grad_stats(self, step=None):
        """--grad_stats: one pass of per-tensor statistics (mdx/optim.py: GradStats) over the float32 master parameters and the
        gradients the step just consumed, read from `.grad` where the step left them -- the eager step's own tensors, a captured
        step's graph tensors after the last replay, the views into the flat buffer after the exchange of a data-parallel step.
        Eager launches on the current stream, behind the step or its replay, never inside a graph; nothing synchronises.  `.grad`
        is only read, and the guard consumes g * coef without storing it: these are the statistics of the UNCLIPPED gradients.
        `step`: the number of the training step behind which the pass runs, kept so that the report can name the step of a pass.
        The history lives on the device in this trainer's GradStats object alone: it is not part of state_dict(), not written
        to state<N>.pt, and a resumed run starts a new one."""
        stats = self.setting.optim.get("grad_stats")
        if stats is not None:
            stats.compute()
            self._grad_stat_passes += 1
            self._grad_stat_torch += int(stats._native and not stats._last_native)
            self._grad_stat_steps[self._grad_stat_passes] = step

    def grad_stats_report(self):
        """-> (the lines rank 0 prints after an epoch, the record it appends to grad_stats.jsonl).  Reads the device records and
        history: the one place of --grad_stats that synchronises."""
        stats = self.setting.optim["grad_stats"]
        passes, steps = self._grad_stat_passes, self._grad_stat_steps
        if not passes:
            return ["grad stats: 0 passes"], dict(passes=0, records={}, history={})
        host, hist, total = stats.host(), stats.history(), stats.total_norm()
        # the device counts the passes of each tensor, the trainer the passes it issued: the step of a pass is known only while the
        # two agree (they part when somebody else calls compute() or reset_history() on the trainer's object)
        in_step = all(h["passes"] == passes for h in hist.values())

        def step_of(p):                                   # the training step of pass p (1-based; 0: never)
            return steps.get(p) if in_step and p > 0 else None
        seen = [(r["grad_norm"], n) for n, r in host.items() if r["grad_present"]]
        line = "grad stats: %d passes, last gradient norm %g" % (passes, total)
        if seen:
            line += ", largest %s %g, smallest %s %g" % (max(seen)[1], max(seen)[0], min(seen)[1], min(seen)[0])
        if self._grad_stat_torch:                         # a gradient without its parameter's dtype or strides: read on the host
            line += "; %d passes took torch's functions, not the kernels" % self._grad_stat_torch
        if not in_step:
            line += "; the history was advanced or reset outside the trainer: steps unknown"
        lines = [line]
        bad = [n for n in stats.names if hist[n]["bad_passes"] > 0]
        if bad:
            lines.append("grad stats: non-finite gradients in %d tensors: %s%s" % (len(bad), ", ".join(
                "%s (first at step %s, %d of %d passes)" % (n, step_of(hist[n]["first_bad_pass"]), hist[n]["bad_passes"], hist[n]["passes"])
                for n in bad[:5]), ", ..." if len(bad) > 5 else ""))
        badw = [n for n in stats.names if hist[n]["first_bad_weight_pass"] > 0]
        if badw:
            lines.append("grad stats: non-finite weights in %d tensors: %s%s" % (len(badw), ", ".join(
                "%s (first at step %s)" % (n, step_of(hist[n]["first_bad_weight_pass"])) for n in badw[:5]),
                ", ..." if len(badw) > 5 else ""))
        keys = (("first_bad_pass", "first_bad_step"), ("last_bad_pass", "last_bad_step"), ("first_bad_weight_pass", "first_bad_weight_step"),
                ("max_grad_pass", "max_grad_step"))
        for h in hist.values():
            h.update({name: step_of(h[key]) for key, name in keys})
        record = dict(passes=passes, torch_passes=self._grad_stat_torch, last_step=steps.get(passes), total_norm=total, records=host,
                      history=hist)
        # only the passes the history points at (and the last one) can be asked for again: the table does not grow with the run
        keep = {h[key] for h in hist.values() for key, _ in keys} | {passes}
        self._grad_stat_steps = {p: st for p, st in steps.items() if p in keep} if in_step else {}
        return lines, record

    def loss_stats(self, outputs, step=None):
        """--loss_stats: one pass of statistics (mdx/loss_stats.py: LossStats) over the maps the step just left in `outputs`:
        `("automask", s)`, the arg-min channel of every pixel, and `("disp", s)` -- the eager step's own tensors, a captured step's
        graph tensors after the last replay.  A scale without an automask entry (one source frame without the auto-mask on the
        op-by-op path) passes None.  Eager launches on the current stream, behind the step or its replay, never inside a graph;
        nothing synchronises and the maps are only read.  `step`: the number of the training step behind which the pass runs.  The
        history lives in this trainer's LossStats object alone: it is not part of any state file and a resumed run starts a new one."""
        stats = self.setting.optim.get("loss_stats")
        if stats is not None:
            stats.compute([outputs.get(("automask", k)) for k in self.opt.scales], [outputs.get(("disp", k)) for k in self.opt.scales])
            self._loss_stat_passes += 1
            self._loss_stat_total += 1
            self._loss_stat_torch += int(stats._native and not stats._last_native)
            self._loss_stat_steps[self._loss_stat_passes] = step

    def loss_stats_report(self):
        """-> (the lines rank 0 prints after an epoch, one per scale, and the record it appends to loss_stats.jsonl): the shares are
        those of the epoch (train() starts the history again after the report), the step numbers those of the run.  Reads the
        device records and history: the one place of --loss_stats that synchronises."""
        stats = self.setting.optim["loss_stats"]
        passes, steps = self._loss_stat_passes, self._loss_stat_steps
        if not passes:
            return ["loss stats: 0 passes"], dict(passes=0, scales={})
        host, hist = stats.host(), stats.history()
        # the device counts the passes of each scale, the trainer the passes it issued: the step of a pass is known only while the
        # two agree (they part when somebody else calls compute() or reset_history() on the trainer's object)
        in_step = all(h["passes"] == passes for h in hist)

        def step_of(p):                                   # the training step of pass p of this epoch (1-based; 0: never)
            return steps.get(p) if in_step and p > 0 else None
        ids = [str(f) for f in self.opt.frame_ids[1:]]
        names = (["identity %s" % f for f in ids] if stats.automask else []) + ["frame %s" % f for f in ids]
        keys = (("first_bad_pass", "first_bad_step"), ("first_static_pass", "first_static_step"), ("last_static_pass", "last_static_step"),
                ("max_masked_pass", "max_masked_step"), ("min_disp_range_pass", "min_disp_range_step"))
        lines, scales = [], {}
        for scale, rows, h in zip(self.opt.scales, host, hist):
            h.update({name: step_of(h[key]) for key, name in keys})
            h["shares"] = dict(zip(names, h["shares"].values()))
            for r in rows:
                r["shares"] = dict(zip(names, r["shares"].values()))
            seen = [r for r in rows if r["disp_present"]]
            line = "loss stats scale %s: %d passes, masked %.4f, %s" % (
                scale, h["passes"], h["masked_share"], ", ".join("%s %.4f" % kv for kv in h["shares"].items()))
            line += "; static images %d of %d" % (h["static_images"], h["images"])
            if h["static_images"]:
                line += " (first at step %s)" % h["first_static_step"]
            if seen:
                line += "; disparity %g .. %g in the last pass" % (min(r["disp_min"] for r in seen), max(r["disp_max"] for r in seen))
            if h["min_disp_range_pass"]:
                line += ", smallest range of an image %g (step %s)" % (h["min_disp_range"], h["min_disp_range_step"])
            line += "; bad passes %d" % h["bad_passes"]
            if h["bad_passes"]:
                line += " (first at step %s)" % h["first_bad_step"]
            lines.append(line)
            scales[str(scale)] = dict(history=h, records=rows)
        if self._loss_stat_torch:                         # int64 indices of the op-by-op path, CPU tensors: read on the host
            lines.append("loss stats: %d passes took torch's functions, not the kernels" % self._loss_stat_torch)
        if not in_step:
            lines.append("loss stats: the history was advanced or reset outside the trainer: steps unknown")
        record = dict(passes=passes, run_passes=self._loss_stat_total, torch_passes=self._loss_stat_torch, last_step=steps.get(passes),
                      scales=scales)
        return lines, record

    def loss_stats_new_epoch(self):
        """The history starts again, and with it the pass numbers: the shares of the next report are those of its own epoch.  No
        pass of the last one can be asked for again, so the {pass: step} table is emptied: it does not grow with the run."""
        self.setting.optim["loss_stats"].reset_history()
        self._loss_stat_passes, self._loss_stat_torch, self._loss_stat_steps = 0, 0, {}

    def depth_supervision_add(self, outputs):
        """--depth_supervision: the step's mean term and valid count join the epoch's sums where they are, on the device (float64:
        the sums of the counts stay exact); nothing is read here.  Five small eager launches behind every step, outside the
        captured graph: part of the option's per-step cost (tools/sparse_depth_cost.py --what step issues them too)."""
        term, valid = outputs["loss_depth"], outputs["depth_valid"]
        if self._depth_acc is None:
            self._depth_acc = torch.zeros(2, dtype=torch.float64, device=term.device)
        self._depth_acc += torch.stack([term.mean().double(), valid.double()])
        self._depth_steps += 1

    def depth_supervision_report(self):
        """-> the line rank 0 prints after an epoch: the mean of the term over the epoch's steps and the mean valid ground-truth
        pixels per image, of THIS rank's batches.  The one read of the host of --depth_supervision; starts the sums again.  (A
        step's count is the kernels' float32 n: exact up to 2^24 valid pixels per batch, mdx.functional.sparse_depth_loss.)"""
        steps = self._depth_steps
        term, valid = self._depth_acc.tolist() if steps else (0.0, 0.0)
        if steps:
            self._depth_acc.zero_()
        self._depth_steps = 0
        return ("depth supervision: weight %g, mean term %.6g, %.1f valid pixels per image over %d steps"
                % (self.compute.depth_supervision, term / max(steps, 1), valid / max(steps * self.opt.batch, 1), steps))

    def stereo_hints_add(self, outputs):
        """--stereo_hints: the step's mean term and valid hint pixels join the epoch's sums where they are, on the device (float64);
        nothing is read here.  Small eager launches behind every step, outside the captured graph, as depth_supervision_add's."""
        term, valid = outputs["loss_hint"], outputs["hint_valid"]
        sums = [term.mean().double(), valid.double()]
        if "hint_kept" in outputs:                       # --stereo_hints_select: the kept hints beside them
            sums.append(outputs["hint_kept"].double())
        if self._hint_acc is None:
            self._hint_acc = torch.zeros(len(sums), dtype=torch.float64, device=term.device)
        self._hint_acc += torch.stack(sums)
        self._hint_steps += 1

    def stereo_hints_report(self):
        """-> the line rank 0 prints after an epoch: the mean of the hint term over the epoch's steps and the mean share of an image's
        pixels that carried a hint, of THIS rank's batches.  The one read of the host of --stereo_hints; starts the sums again."""
        steps = self._hint_steps
        term, valid, *kept = self._hint_acc.tolist() if steps else (0.0, 0.0)
        if steps:
            self._hint_acc.zero_()
        self._hint_steps = 0
        pixels = steps * self.opt.batch * self.opt.height * self.opt.width
        line = ("stereo hints: weight %g, %d disparities, mean term %.6g, valid share %.4f per image over %d steps"
                % (self.compute.stereo_hints, self.compute.stereo_hints_disp, term / max(steps, 1), valid / max(pixels, 1), steps))
        if kept:                                         # --stereo_hints_select: the share of the hints that passed the reprojection test
            line += ", kept share %.4f of the hints" % (kept[0] / max(valid, 1.0))
        return line

    def can_graph(self):
        """The step is capturable when nothing in it runs on the host: not with the reference's host-side noise
        (--noise cpu: torch.randn on the CPU + a copy from pageable memory), not with a non-RCCL process group.  With more than
        one rank the capture takes the split form (graphed_step) unless MDX_DP_GRAPH=1 asks for the exchange inside the graph."""
        sync = self.setting.sync
        return (str(self.device).startswith("cuda") and self.compute.noise_mode != "cpu"
                and (sync is None or sync.backend == "nccl"))

    def train_step(self, inputs):
        """opt.graph (GPU): the step -- under torch.distributed including the gradient exchange -- is captured once
        into a hipGraph and replayed (graphed_step); otherwise eager."""
        use_graph = getattr(self.opt, "graph", False) and self.can_graph()
        if not use_graph:
            if getattr(self.opt, "graph", False) and not getattr(self, "_told_eager", False) and str(self.device).startswith("cuda"):
                self._told_eager = True       # once, rank 0: --graph was asked for and the step runs eager (other bucket sizes, queues)
                if self.rank == 0:
                    why = "--noise cpu draws on the host" if self.compute.noise_mode == "cpu" else "the process group is not RCCL"
                    print("model_train: --graph requested but the step is not captured (%s); running the eager step" % why, flush=True)
            return self._eager_step(inputs)
        inputs = self.compute.prepare(inputs)     # decoded frames -> step entries (a no-op after the prefetcher)
        if self._graphed is None:
            self._graphed = graphed_step(self, inputs)
        mon = getattr(self.control, "_side", None)
        if mon is not None:                       # the depth monitor of the previous step reads the graph's outputs
            torch.cuda.current_stream(self.device).wait_stream(mon)
        return self._graphed(inputs)

    def valid_step(self, inputs):
        """One validation step (the caller holds torch.no_grad() and has put the networks in eval mode).  opt.graph and
        opt.graph_valid (GPU, capturable): captured once into graphed_valid_step and replayed for every batch of the captured
        shape; otherwise -- or for a batch of another shape -- eager."""
        use_graph = (getattr(self.opt, "graph", False) and getattr(self.opt, "graph_valid", True) and self.can_graph())
        if not use_graph:
            return self.batch_process(inputs)
        inputs = self.compute.prepare(inputs)     # decoded frames -> step entries (a no-op after the prefetcher)
        if self._graphed_valid is None:
            self._graphed_valid = graphed_valid_step(self, inputs)
        if not self._graphed_valid.matches(inputs):
            return self.batch_process(inputs)
        mon = getattr(self.control, "_side", None)
        if mon is not None:                       # the depth monitor of the previous step reads the graph's outputs
            torch.cuda.current_stream(self.device).wait_stream(mon)
        return self._graphed_valid(inputs)

    def train(self):
        names = self.control.metric_name
        epoch_train = {k: [] for k in names}
        epoch_valid = {k: [] for k in names}
        start = 0
        if getattr(self.opt, "resume", 0):     # weights, optimiser, scheduler and the per-epoch logs so far
            start = self.control.resume(self.setting, self.opt.resume, epoch_train, epoch_valid, compute=self.compute)
        # --check_weights N: the ranks' weights are compared before the first step (behind broadcast_state or resume), after every
        # N-th step of the run and before each checkpoint
        every, done = int(getattr(self.opt, "check_weights", 0) or 0), 0
        self.check_weights()
        # --grad_stats N: per-tensor gradient and weight statistics behind every N-th step of the run; every rank computes (the
        # ranks stay in step), rank 0 alone reads and reports, once per epoch
        stats_every = int(getattr(self.opt, "grad_stats", 0) or 0) if "grad_stats" in self.setting.optim else 0
        # --loss_stats N: statistics of the loss path's maps behind every N-th step of the run, reported like --grad_stats; the
        # report covers rank 0's own batches
        loss_every = int(getattr(self.opt, "loss_stats", 0) or 0) if "loss_stats" in self.setting.optim else 0
        supervised = self.compute.depth_supervision > 0      # --depth_supervision: one line per epoch, read once per epoch
        hinted = self.compute.stereo_hints > 0               # --stereo_hints: likewise
        for epoch in range(start, self.opt.epoch):
            batch_train = {k: [] for k in names}
            batch_valid = {k: [] for k in names}
            self.setting.set_train()
            sampler = getattr(self.setting.train_dataloader, "sampler", None)
            if hasattr(sampler, "set_epoch"):
                sampler.set_epoch(epoch)
            for step, train_inputs in enumerate(self.batches(self.setting.train_dataloader)):
                train_outputs = self.train_step(train_inputs)
                batch_train = self.control.metric(train_inputs, train_outputs, batch_train)
                done += 1
                if every > 0 and done % every == 0:
                    self.check_weights()
                if stats_every > 0 and done % stats_every == 0:
                    self.grad_stats(done)
                if loss_every > 0 and done % loss_every == 0:
                    self.loss_stats(train_outputs, done)
                if supervised:
                    self.depth_supervision_add(train_outputs)
                if hinted:
                    self.stereo_hints_add(train_outputs)
                if self.opt.max_steps and step + 1 >= self.opt.max_steps:
                    break
            self.setting.set_valid()
            # --ema_valid: the validation reads the averaged weights -- exchanged in place by eager launches outside the validation
            # graph, which reads the weights where they live -- and the live ones are back before the next training step
            ema = self.setting.optim.get("ema")
            with ema.applied() if ema is not None and getattr(self.opt, "ema_valid", 1) else contextlib.nullcontext():
                for step, valid_inputs in enumerate(self.batches(self.setting.valid_dataloader)):
                    with torch.no_grad():
                        valid_outputs = self.valid_step(valid_inputs)
                        batch_valid = self.control.metric(valid_inputs, valid_outputs, batch_valid)
                    if self.opt.max_steps and step + 1 >= self.opt.max_steps:
                        break
            self.setting.optim["scheduler"].step()
            if self._graphed is not None:         # StepLR wrote a new Python value: hand it to the captured Adam's lr tensor
                lr = self.setting.optim["scheduler"].get_last_lr()[0]
                self._graphed.set_lr(lr)
                for g in self.setting.optim["optimizer"].param_groups:
                    g["lr"] = self._graphed.lr
            # epoch means over everything the JOB saw: one all-reduce of the 2 x 8 scalars (every rank takes part)
            mean_train, mean_valid = self.control.epoch_means(batch_train), self.control.epoch_means(batch_valid)
            for key in names:
                epoch_train[key].append(mean_train[key])
                epoch_valid[key].append(mean_valid[key])
            depth_line = self.depth_supervision_report() if supervised else None
            hint_line = self.stereo_hints_report() if hinted else None
            if self.rank == 0:
                self.control.print(epoch, mean_train, mean_valid)
                if depth_line:
                    print(depth_line, flush=True)
                if hint_line:
                    print(hint_line, flush=True)
                optimizer = self.setting.optim["optimizer"]
                if getattr(optimizer, "guarded", False):
                    g = optimizer.guard_stats()
                    print("step guard: %d steps, %d skipped, last gradient norm %g" % (g["steps"], g["skipped_steps"], g["total_norm"]),
                          flush=True)
                if stats_every > 0:
                    lines, record = self.grad_stats_report()
                    print("\n".join(lines), flush=True)
                    directory = os.path.join("./model_save", self.opt.save)
                    os.makedirs(directory, exist_ok=True)
                    with open(os.path.join(directory, "grad_stats.jsonl"), "a") as f:
                        f.write(json.dumps(dict(epoch=epoch + 1, **record)) + "\n")
                if loss_every > 0:
                    lines, record = self.loss_stats_report()
                    print("\n".join(lines), flush=True)
                    directory = os.path.join("./model_save", self.opt.save)
                    os.makedirs(directory, exist_ok=True)
                    with open(os.path.join(directory, "loss_stats.jsonl"), "a") as f:
                        f.write(json.dumps(dict(epoch=epoch + 1, **record)) + "\n")
                if ema is not None:
                    e = ema.stats()
                    print("weight EMA: %d updates, %d held" % (e["updates"], e["held"]), flush=True)
                if every > 0:
                    print("weight check: %d checks, ranks agree" % self._weight_checks, flush=True)
            if loss_every > 0:                    # every rank: the shares of the next report are those of its own epoch
                self.loss_stats_new_epoch()
            self.check_weights()
            self.control.save(epoch, epoch_train, epoch_valid, self.setting, compute=self.compute)


if __name__ == "__main__":
    trainer(options()).train()
