"""The optimiser of the training step: torch.optim.Adam(fused=True) with its step as ONE launch of csrc/adam.hip.

Same class from the outside (reference model_tool/loader.py:93-97 builds torch.optim.Adam): parameter groups, `state_dict()` /
`load_state_dict()` (per-parameter "step", "exp_avg", "exp_avg_sq"), capturable learning-rate tensors (model_train.graphed_step).
What the kernel does not cover -- weight decay, amsgrad, maximize, a closure, a GradScaler's grad_scale / found_inf, parameters that
are not dense float32 GPU tensors -- goes through torch's own step.

The step guard (off by default): `Adam(params, lr, max_grad_norm=1.0, skip_nonfinite=True)` clips by the global L2 norm of every
gradient the step consumes and / or leaves parameters, moments and step counts untouched when that norm is not finite.  On the native
path the decision is taken on the device (three launches, capturable, no host synchronisation, deterministic; `.grad` is never
written); `guard_stats()` is the only call that synchronises.  Where the step goes through torch's own functions -- CPU parameters,
anything `_native_ok` rejects -- the guard does too: a float64 norm and a HOST-side skip (so that path cannot be captured), then
`torch.nn.utils.clip_grad_norm_`, which scales `.grad` in place.  The guard's record is not part of `state_dict()`.

`WeightEMA(modules, decay)`: an exponential moving average of the weights and batch-norm statistics, updated after every optimiser
step by csrc/ema.hip -- capturable with the step, its decay warm-up and the guard's skip decided on the device -- and exchanged with
the live weights in place for validation and checkpoints (`swap()`, `applied()`).

`WeightDigest(tensors, names)`: one 64-bit digest per tensor by csrc/digest.hip -- a read-only pass, an integer sum without order or
tolerance -- for the replica check of a data-parallel run and the checkpoint verification of a resumed one.

`GradStats(params, names)`: per-tensor norms, largest magnitudes and counts of non-finite and zero elements of every parameter and
its gradient by csrc/tensor_stats.hip -- a read-only, capturable, deterministic pass with a per-tensor history kept on the device --
for finding the layer behind a skipped or clipped step."""
import contextlib
import ctypes as C
import math

import torch

from . import _lib
from ._lib import _capturing, api, host_tensor, read_structs, stream


# ---- what the four passes share (csrc/mdx_multi_tensor.hpp): a PLAN is a device table, the launches over it, a pointer key --------
def _device_table(entry_type, entry_bytes, *tensor_lists):
    """The device table of a plan: entry i holds the pointers of the i-th tensor of every list, then the first list's numel."""
    assert C.sizeof(entry_type) == entry_bytes
    host = (entry_type * len(tensor_lists[0]))()
    for i, ts in enumerate(zip(*tensor_lists)):
        host[i] = entry_type(*[t.data_ptr() for t in ts], ts[0].numel())
    return host_tensor(host).to(tensor_lists[0][0].device)


def _launches(tensors, base):
    """[(first table entry, count, block map, blocks)] covering `tensors`, whose table entries start at `base`."""
    chunk, per = api.mdx_adam_chunk(), api.mdx_adam_max_tensors()
    launches = []
    for first in range(0, len(tensors), per):
        count = min(per, len(tensors) - first)
        bm = []
        for t in range(count):
            bm += [(t, c) for c in range((tensors[first + t].numel() + chunk - 1) // chunk)]
        blockmap = torch.tensor(bm, dtype=torch.int32).to(tensors[0].device)
        launches.append((base + first, count, blockmap, len(bm)))
    return launches


def _key(*tensor_lists):
    """A plan is good for as long as every tensor stays where it is."""
    return tuple(t.data_ptr() for ts in tensor_lists for t in ts)


def _check_device(who, dev):
    if dev.index != torch.cuda.current_device():
        raise _lib.MdxError("mdx.optim.%s live on %s but the current device is cuda:%d" % (who, dev, torch.cuda.current_device()))


def _check_storage(who, tensors, key):
    if _key(tensors) != key:
        raise _lib.MdxError("mdx.optim.%s changed its storage since construction" % who)


def _dense_f32(t, dev, like=None):
    """What the kernels walk: float32 on the GPU `dev`, contiguous or channels-last -- or, per gradient of a step (one call, no
    second look at the strides), laid out as `like`, a tensor that is."""
    return (t.is_cuda and t.device == dev and t.dtype == torch.float32 and not t.is_sparse
            and (t.is_contiguous() or t.is_contiguous(memory_format=torch.channels_last) if like is None
                 else t.stride() == like.stride() and t.shape == like.shape))


def _same_layout(a, b):
    return a.stride() == b.stride() and a.shape == b.shape


def _lr_args(group):
    """(lr_ptr, lr) of a launch: a float32 device tensor travels as its pointer (a captured step's learning rate), else a double."""
    lr = group["lr"]
    if torch.is_tensor(lr) and lr.is_cuda and lr.dtype == torch.float32:
        return lr.data_ptr(), 0.0
    return None, float(lr)


class _Table(C.Structure):
    _fields_ = [("p", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("step", C.c_void_p), ("n", C.c_int64)]


class Adam(torch.optim.Adam):
    native = True          # False: every step goes through torch's own (the guard with it)

    def __init__(self, params, lr=1e-3, max_grad_norm=None, skip_nonfinite=False, **kw):
        if max_grad_norm is not None and not float(max_grad_norm) > 0:
            raise ValueError("max_grad_norm must be positive or None, got %r" % (max_grad_norm,))
        kw.setdefault("fused", True)
        super().__init__(params, lr, **kw)
        self._plans = {}
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._guard = None               # the guarded step's plan: one table over every group, partials, launches
        self._record = None              # the device record (include/mdx.h: mdx_adam_guard_finish)
        self._host_stats = dict(total_norm=0.0, coef=1.0, skipped=False, steps=0, skipped_steps=0)   # torch-path guard
        self._last_native = True

    @property
    def guarded(self):
        return self.max_grad_norm is not None or self.skip_nonfinite

    # -- what one launch needs, built once per parameter group -------------------------------------------------------------
    # Two kinds of plan, each built in the first step that needs it and rebuilt when its pointer key changes: the plain step has
    # one table per parameter group, the guarded step ONE table over the tensors of every group (the norm is global).
    def _plan(self, gi, *lists):
        """The plain step's plan for group gi; lists: params, exp_avgs, exp_avg_sqs, steps."""
        key = _key(*lists)
        plan = self._plans.get(gi)
        if plan is None or plan["key"] != key:
            plan = self._plans[gi] = dict(key=key, table=_device_table(_Table, api.mdx_adam_table_entry_bytes(), *lists),
                                          launches=_launches(lists[0], 0))
        return plan

    def _guard_plan(self, todo):
        """The guarded step's plan: the table, each group's launches with their slice of the partials buffer, the record.  Built
        in the first (eager, warm-up) step, never inside a capture."""
        cat = [sum((list(item[k]) for item in todo), []) for k in (2, 4, 5, 6)]        # params, exp_avgs, exp_avg_sqs, steps
        key = _key(*cat)
        if self._guard is not None and self._guard["key"] == key:
            return self._guard
        dev = cat[0][0].device
        launches, base, slot = [], 0, 0
        for ti, item in enumerate(todo):
            for first, count, blockmap, nblocks in _launches(item[2], base):
                launches.append((ti, first, first - base, count, blockmap, nblocks, slot))
                slot += nblocks
            base += len(item[2])
        if self._record is None or self._record.device != dev:
            assert C.sizeof(GuardRecord) == api.mdx_adam_guard_record_bytes()
            self._record = torch.zeros(C.sizeof(GuardRecord) // 8, dtype=torch.int64, device=dev)
        partials = torch.empty(api.mdx_adam_guard_partials_bytes(slot) // 8, dtype=torch.float64, device=dev)
        self._guard = dict(key=key, table=_device_table(_Table, api.mdx_adam_table_entry_bytes(), *cat), launches=launches,
                           partials=partials, ntensors=base, nblocks=slot)
        return self._guard

    def _native_ok(self, group, params, grads, exp_avgs, exp_avg_sqs, steps):
        if not self.native or group["weight_decay"] != 0 or group["amsgrad"] or group["maximize"] or group.get("differentiable"):
            return False
        if getattr(self, "grad_scale", None) is not None or getattr(self, "found_inf", None) is not None:
            return False
        dev = params[0].device
        return all(_dense_f32(p, dev) and _dense_f32(g, dev, p) and _same_layout(m, p) and _same_layout(v, p)
                   and torch.is_tensor(s) and s.is_cuda and s.dtype == torch.float32 and s.numel() == 1
                   for p, g, m, v, s in zip(params, grads, exp_avgs, exp_avg_sqs, steps))

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            if not self.guarded:
                return super().step(closure)
            with torch.enable_grad():
                loss = closure()
            self._torch_guarded_step()
            return loss
        todo = []
        for gi, group in enumerate(self.param_groups):
            params, grads, exp_avgs, exp_avg_sqs, max_sqs, steps = [], [], [], [], [], []
            self._init_group(group, params, grads, exp_avgs, exp_avg_sqs, max_sqs, steps)
            if not params:
                continue
            if not self._native_ok(group, params, grads, exp_avgs, exp_avg_sqs, steps):
                return self._torch_guarded_step() if self.guarded else super().step()
            todo.append((gi, group, params, grads, exp_avgs, exp_avg_sqs, steps))
        if self.guarded and todo:
            if len({item[2][0].device for item in todo}) > 1:        # one table, one record: one device
                return self._torch_guarded_step()
            return self._native_guarded_step(todo)
        for gi, group, params, grads, exp_avgs, exp_avg_sqs, steps in todo:
            _check_device("Adam: parameters", params[0].device)
            plan = self._plan(gi, params, exp_avgs, exp_avg_sqs, steps)
            torch._foreach_add_(steps, 1)
            lr_ptr, lr = _lr_args(group)
            beta1, beta2 = group["betas"]
            for first, count, blockmap, nblocks in plan["launches"]:
                garr = (C.c_void_p * count)(*[g.data_ptr() for g in grads[first:first + count]])
                api.mdx_adam_step(plan["table"].data_ptr(), first, count, garr, blockmap.data_ptr(), nblocks, lr_ptr, lr,
                                  beta1, beta2, group["eps"], stream())
        return None

    # -- the guarded step ---------------------------------------------------------------------------------------------------
    def _native_guarded_step(self, todo):
        """Sum of squares (one launch per <= mdx_adam_max_tensors() tensors), finish (norm, coefficient, skip flag, totals, step
        counts), guarded Adam: include/mdx.h.  Nothing here looks at a value on the host."""
        _check_device("Adam: parameters", todo[0][2][0].device)
        plan = self._guard_plan(todo)
        table, partials, record = plan["table"].data_ptr(), plan["partials"].data_ptr(), self._record.data_ptr()
        garrs = []
        for ti, first, local, count, blockmap, nblocks, slot in plan["launches"]:
            garr = (C.c_void_p * count)(*[g.data_ptr() for g in todo[ti][3][local:local + count]])
            garrs.append(garr)
            api.mdx_adam_grad_sumsq(table, first, count, garr, blockmap.data_ptr(), nblocks, partials + 8 * slot, stream())
        api.mdx_adam_guard_finish(table, plan["ntensors"], partials, plan["nblocks"], self.max_grad_norm or 0.0,
                                  int(self.skip_nonfinite), record, stream())
        for garr, (ti, first, local, count, blockmap, nblocks, slot) in zip(garrs, plan["launches"]):
            group = todo[ti][1]
            lr_ptr, lr = _lr_args(group)
            beta1, beta2 = group["betas"]
            api.mdx_adam_step_guarded(table, first, count, garr, blockmap.data_ptr(), nblocks, lr_ptr, lr, beta1, beta2,
                                      group["eps"], record, stream())
        self._last_native = True
        return None

    def _torch_guarded_step(self):
        """The guard around torch's own step: the norm in float64 (a large finite gradient stays finite), the skip decided on the
        host, then clip_grad_norm_ -- which scales .grad in place -- and torch's Adam."""
        grads = [p.grad for g in self.param_groups for p in g["params"] if p.grad is not None]
        if not grads:
            return super().step()
        norms = [torch.linalg.vector_norm(g.detach(), 2.0, dtype=torch.float64) for g in grads]
        norm = torch.linalg.vector_norm(torch.stack([n.to(norms[0].device) for n in norms])).float().cpu()
        coef = torch.ones(())
        if self.max_grad_norm is not None:
            coef = torch.clamp(torch.tensor(self.max_grad_norm) / (norm + 1e-6), max=1.0)
        skipped = self.skip_nonfinite and not bool(torch.isfinite(norm))
        st = self._host_stats
        st.update(total_norm=float(norm), coef=float(coef), skipped=skipped, steps=st["steps"] + 1,
                  skipped_steps=st["skipped_steps"] + int(skipped))
        self._last_native = False
        if skipped:
            return None
        if self.max_grad_norm is not None:
            torch.nn.utils.clip_grad_norm_([p for g in self.param_groups for p in g["params"] if p.grad is not None],
                                           self.max_grad_norm)
        return super().step()

    def guard_stats(self):
        """{total_norm, coef, skipped: of the last guarded step; steps, skipped_steps: running totals}.  Reads the device record:
        the one place of the guard that synchronises."""
        out = dict(self._host_stats)
        if self._record is not None:
            rec = GuardRecord.from_buffer_copy(self._record.cpu().numpy().tobytes())
            if self._last_native:
                out.update(total_norm=rec.total_norm, coef=rec.coef, skipped=bool(rec.skipped))
            out["steps"] += rec.steps
            out["skipped_steps"] += rec.skipped_steps
        return out

    def guard_decision(self, device):
        """What a follower of the last step needs to withhold its own work with a skipped step (WeightEMA.update): (pointer of the
        device record, False) when that step took the native path and the follower's kernels run on the record's `device` (None:
        it runs on the host); else (None, was the step skipped?) -- the host's flag or, for a native step, ONE synchronising read."""
        if not self.guarded or (self._last_native and self._record is None):
            return None, False
        if not self._last_native:
            return None, self._host_stats["skipped"]
        if device == self._record.device:
            return self._record.data_ptr(), False
        return None, self.guard_stats()["skipped"]

    def guard_snapshot(self):
        """The guard's record and totals, for a caller that undoes steps (model_train.graphed_step's warm-up)."""
        return (None if self._record is None else self._record.clone(), dict(self._host_stats), self._last_native)

    def guard_restore(self, snapshot):
        record, self._host_stats, self._last_native = snapshot[0], dict(snapshot[1]), snapshot[2]
        if self._record is not None:
            if record is not None:
                self._record.copy_(record)
            else:
                self._record.zero_()             # no guarded step had run


class _EmaTable(C.Structure):
    _fields_ = [("p", C.c_void_p), ("e", C.c_void_p), ("n", C.c_int64)]


class WeightEMA(object):
    """Shadows of every trained parameter and every float32 buffer (batch-norm running statistics; integer buffers are left alone)
    of `modules`: after each optimiser step `update(optimizer)` moves them towards the live values,

        shadow = lerp(shadow, live, 1 - d_t),   d_t = min(decay, (1 + t) / (10 + t)) with warm-up, else decay;  t = updates so far

    `swap()` exchanges live and shadow storage bit for bit -- the networks, and a captured validation graph that reads the weights
    where they live, then run on the average; a second `swap()` puts everything back -- and `applied()` does both around a block.
    Dense float32 GPU tensors go through csrc/ema.hip (include/mdx.h: mdx_ema_update, mdx_ema_tick, mdx_ema_swap): the counters
    are a device record, a step the optimiser's guard skipped is withheld on the device, nothing synchronises but `stats()`, and
    the table, block maps and record are built HERE, so nothing is allocated inside a capture.  Any other tensor set (CPU,
    another dtype, not dense) takes the same arithmetic through torch's own functions with the counters on the host.

    The parameters are taken as they are at construction -- the float32 masters, never the bfloat16 copies that
    mdx.shadow.bf16_weights shows the modules during a step -- and must keep their storage.  `shadows` (optional): {name: tensor},
    storage of the caller's for the shadows named (a slice of one arena, say) -- shape, dtype, device and strides of the live tensor;
    the other shadows are allocated here.  All of them start from the live values."""

    native = True          # False: torch's own functions for every tensor

    def __init__(self, modules, decay, warmup=True, shadows=None):
        decay = float(decay)
        if not 0.0 <= decay < 1.0:
            raise ValueError("decay must lie in [0, 1), got %r" % (decay,))
        self.decay, self.warmup = decay, bool(warmup)
        modules = [modules] if isinstance(modules, torch.nn.Module) else list(modules)
        self.names, self.live, seen = [], [], set()
        for i, net in enumerate(modules):
            named = [(n, p) for n, p in net.named_parameters() if p.requires_grad]
            named += [(n, b) for n, b in net.named_buffers() if b.dtype == torch.float32]
            for n, t in named:
                if id(t) not in seen:
                    seen.add(id(t))
                    self.names.append("%d.%s" % (i, n))
                    self.live.append(t)
        if not self.live:
            raise ValueError("WeightEMA: the modules have no trained parameter and no float32 buffer")
        with torch.no_grad():
            given = dict(shadows or {})
            self.shadow = [given.pop(n) if n in given else torch.empty_like(t)      # preserve_format: channels-last keeps its strides
                           for n, t in zip(self.names, self.live)]
            if given:
                raise KeyError("WeightEMA: no parameter or float32 buffer is called %s" % ", ".join(sorted(given)))
            for n, e, t in zip(self.names, self.shadow, self.live):
                if (e.shape, e.dtype, e.device, e.stride()) != (t.shape, t.dtype, t.device, t.stride()) or e is t:
                    raise ValueError("WeightEMA: the shadow given for %s does not match its tensor" % n)
            for e, t in zip(self.shadow, self.live):
                e.copy_(t)
        self._host = dict(updates=0, held=0)
        self._native = self._native_ok()
        self._record = self._table = self._launches = None
        if self._native:
            assert api.mdx_ema_record_bytes() == 16
            self._table = _device_table(_EmaTable, api.mdx_ema_table_entry_bytes(), self.live, self.shadow)
            self._launches = _launches(self.live, 0)
            self._record = torch.zeros(2, dtype=torch.int64, device=self.live[0].device)
            self._key = _key(self.live)

    def _native_ok(self):
        dev = self.live[0].device
        return self.native and all(_dense_f32(t, dev) and t.numel() > 0 and _same_layout(e, t) for t, e in zip(self.live, self.shadow))

    def _check_native(self):
        _check_device("WeightEMA: tensors", self.live[0].device)
        _check_storage("WeightEMA: a parameter or buffer has", self.live, self._key)

    def _weight(self, t):
        d = min(self.decay, (1.0 + t) / (10.0 + t)) if self.warmup else self.decay
        return float(torch.tensor(1.0 - d, dtype=torch.float64).float())

    @torch.no_grad()
    def update(self, optimizer=None):
        """One update, after `optimizer.step()`.  A guarded mdx.optim.Adam hands its device record over when its last step took the
        native path; where the guard decided on the host (torch's own step), so does the skip here."""
        guard = None
        if getattr(optimizer, "guarded", False):
            guard, skipped = optimizer.guard_decision(self.live[0].device if self._native else None)
            if skipped:
                self._host["held"] += 1
                return
        if not self._native:
            w = self._weight(self._host["updates"])
            for e, t in zip(self.shadow, self.live):
                e.lerp_(t.detach(), w)
            self._host["updates"] += 1
            return
        self._check_native()
        table, record = self._table.data_ptr(), self._record.data_ptr()
        for first, count, blockmap, nblocks in self._launches:
            api.mdx_ema_update(table, first, count, blockmap.data_ptr(), nblocks, self.decay, int(self.warmup), record, guard, stream())
        api.mdx_ema_tick(record, guard, stream())

    @torch.no_grad()
    def swap(self):
        """Exchange live and shadow values in place, bit for bit.  Two swaps are the identity."""
        if not self._native:
            for e, t in zip(self.shadow, self.live):
                keep = e.clone()
                e.copy_(t)
                t.copy_(keep)
            return
        self._check_native()
        for first, count, blockmap, nblocks in self._launches:
            api.mdx_ema_swap(self._table.data_ptr(), first, count, blockmap.data_ptr(), nblocks, stream())

    @contextlib.contextmanager
    def applied(self):
        """While the block runs, the modules hold the average (and the shadows the live values); put back on the way out, also
        when the block raises."""
        self.swap()
        try:
            yield self
        finally:
            self.swap()

    def stats(self):
        """{updates, held}.  Reads the device record: the one call that synchronises."""
        out = dict(self._host)
        if self._record is not None:
            updates, held = self._record.cpu().tolist()
            out["updates"] += updates
            out["held"] += held
        return out

    def _set_counters(self, updates, held):
        if self._record is not None:
            self._record.copy_(torch.tensor([int(updates), int(held)], dtype=torch.int64))
            self._host = dict(updates=0, held=0)
        else:
            self._host = dict(updates=int(updates), held=int(held))

    def state_dict(self):
        st = self.stats()
        return {"shadow": {n: e.detach().clone() for n, e in zip(self.names, self.shadow)}, "updates": st["updates"], "held": st["held"]}

    @torch.no_grad()
    def load_state_dict(self, state):
        missing = [n for n in self.names if n not in state["shadow"]]
        if missing:
            raise KeyError("WeightEMA.load_state_dict: no shadow for %s" % ", ".join(missing[:5]))
        for n, e in zip(self.names, self.shadow):
            e.copy_(state["shadow"][n])
        self._set_counters(state["updates"], state["held"])

    @torch.no_grad()
    def reset(self):
        """Start again from the live values: shadows equal to them, no update counted."""
        for e, t in zip(self.shadow, self.live):
            e.copy_(t)
        self._set_counters(0, 0)

    def snapshot(self):
        """Shadows and counters, for a caller that undoes steps (model_train.graphed_step's warm-up)."""
        return ([e.detach().clone() for e in self.shadow], None if self._record is None else self._record.clone(), dict(self._host))

    @torch.no_grad()
    def restore(self, snapshot):
        for e, s in zip(self.shadow, snapshot[0]):
            e.copy_(s)
        if self._record is not None:
            self._record.copy_(snapshot[1])
        self._host = dict(snapshot[2])


class _DigestTable(C.Structure):
    _fields_ = [("w", C.c_void_p), ("n", C.c_int64)]


class WeightDigest(object):
    """One 64-bit digest per tensor of `tensors`, for equality only: what data-parallel ranks compare after a step
    (model_tool.parallel.check_replicas) and what a checkpoint's state file records of the weight files beside it
    (model_tool.logger.control).  The digest of a tensor is the sum modulo 2^64, over storage index i = 0 .. numel - 1 of its dense
    storage, of a 32-bit hash of (i, the 32-bit word at i) -- include/mdx.h states the recipe.  The words are never read as
    floats (NaN payloads and the sign of zero count), the sum has no order and no tolerance, and a tensor is hashed in STORAGE
    order: a channels-last tensor and its contiguous copy have different digests.

    Dense float32 GPU tensors on one device, contiguous or channels-last, go through csrc/digest.hip (mdx_digest_words): the table,
    block maps and the int64 output tensor are built HERE, nothing is allocated later, `compute()` launches without synchronising
    and is capturable; `host()` is the one call that synchronises.  Any other set of dense float32 tensors (CPU tensors, or
    `native = False`) is hashed with numpy over the storage.  The tensors must keep their storage.  `names` default to "0", "1", ..."""

    native = True          # False: numpy for every tensor

    def __init__(self, tensors, names=None):
        if _capturing():
            raise _lib.MdxError("mdx.optim.WeightDigest: built while the current stream is being captured")
        self.tensors = [t.detach() for t in tensors]
        self.names = [str(i) for i in range(len(self.tensors))] if names is None else [str(n) for n in names]
        if not self.tensors:
            raise ValueError("WeightDigest: no tensors")
        if len(self.names) != len(self.tensors) or len(set(self.names)) != len(self.names):
            raise ValueError("WeightDigest: %d tensors need %d distinct names" % (len(self.tensors), len(self.tensors)))
        for n, t in zip(self.names, self.tensors):
            if t.dtype != torch.float32 or not self._dense(t):
                raise ValueError("WeightDigest: %s is %s with shape %s and strides %s; dense float32 storage is hashed"
                                 % (n, t.dtype, tuple(t.shape), t.stride()))
        self._native = self._native_ok()
        self._table = self._launches = None
        if self._native:
            self._table = _device_table(_DigestTable, api.mdx_digest_table_entry_bytes(), self.tensors)
            self._launches = _launches(self.tensors, 0)
            self._out = torch.zeros(len(self.tensors), dtype=torch.int64, device=self.tensors[0].device)
            self._key = _key(self.tensors)
        else:
            self._out = torch.zeros(len(self.tensors), dtype=torch.int64)

    @staticmethod
    def _dense(t):
        """Non-overlapping and without gaps: the strides are a permutation of the contiguous ones."""
        expect = 1
        for st, sz in sorted((st, sz) for st, sz in zip(t.stride(), t.shape) if sz != 1):
            if st != expect:
                return False
            expect *= sz
        return True

    def _native_ok(self):
        dev = self.tensors[0].device
        return self.native and all(_dense_f32(t, dev) and t.numel() > 0 for t in self.tensors)

    @staticmethod
    def _numpy_digest(t):
        """The recipe of include/mdx.h over the storage of one dense float32 tensor, as a signed 64-bit integer."""
        import numpy as np
        n = t.numel()
        words = torch.as_strided(t, (n,), (1,)).cpu().contiguous().view(torch.int32).numpy().view(np.uint32)
        k = words ^ (np.arange(n, dtype=np.uint64).astype(np.uint32) * np.uint32(0x9E3779B1))
        k ^= k >> np.uint32(16)
        k *= np.uint32(0x85EBCA6B)
        k ^= k >> np.uint32(13)
        k *= np.uint32(0xC2B2AE35)
        k ^= k >> np.uint32(16)
        total = int(k.sum(dtype=np.uint64))                 # numpy's unsigned sum wraps, as the kernel's does
        return total - (1 << 64) if total >> 63 else total

    @torch.no_grad()
    def compute(self):
        """-> the int64 tensor of the digests (the 64 bits of each sum; the same tensor at every call), on the tensors' device
        without a synchronisation on the native path, on the host otherwise."""
        if not self._native:
            if _capturing() and any(t.is_cuda for t in self.tensors):
                raise _lib.MdxError("mdx.optim.WeightDigest: the numpy path reads the tensors on the host and cannot be captured")
            self._out.copy_(torch.tensor([self._numpy_digest(t) for t in self.tensors], dtype=torch.int64))
            return self._out
        _check_device("WeightDigest: tensors", self.tensors[0].device)
        _check_storage("WeightDigest: a tensor has", self.tensors, self._key)
        for first, count, blockmap, nblocks in self._launches:
            api.mdx_digest_words(self._table.data_ptr(), first, count, blockmap.data_ptr(), nblocks, self._out.data_ptr(), stream())
        return self._out

    def host(self):
        """{name: digest as an integer in [0, 2^64)}: computes, then reads -- the one call that synchronises."""
        if _capturing():
            raise _lib.MdxError("mdx.optim.WeightDigest.host() synchronises and the current stream is being captured")
        return {n: int(d) & 0xFFFFFFFFFFFFFFFF for n, d in zip(self.names, self.compute().cpu().tolist())}


class _StatsTable(C.Structure):
    _fields_ = [("w", C.c_void_p), ("n", C.c_int64)]


class GuardRecord(C.Structure):            # csrc/mdx_multi_tensor.hpp: GuardRecord (mdx_adam_guard_record_bytes())
    _fields_ = [("total_norm", C.c_float), ("coef", C.c_float), ("skipped", C.c_int), ("reserved", C.c_int),
                ("steps", C.c_int64), ("skipped_steps", C.c_int64)]


class TensorStats(C.Structure):            # include/mdx.h: mdx_tensor_stats
    _fields_ = [("grad_sumsq", C.c_double), ("weight_sumsq", C.c_double), ("grad_absmax", C.c_float), ("weight_absmax", C.c_float),
                ("grad_nonfinite", C.c_uint32), ("weight_nonfinite", C.c_uint32), ("grad_zeros", C.c_uint32),
                ("grad_present", C.c_uint32)]


class TensorStatsHistory(C.Structure):     # include/mdx.h: mdx_tensor_stats_history
    _fields_ = [("passes", C.c_int64), ("bad_passes", C.c_int64), ("first_bad_pass", C.c_int64), ("last_bad_pass", C.c_int64),
                ("first_bad_weight_pass", C.c_int64), ("max_grad_sumsq", C.c_double), ("max_grad_pass", C.c_int64)]


class GradStats(object):
    """Per-tensor statistics of every parameter of `params` and its gradient, for finding the layer: where the step guard reports one
    global norm, `compute()` gives each tensor a record (include/mdx.h: mdx_tensor_stats) -- the sums of squares of the FINITE
    elements of gradient and weight, their largest finite magnitudes, the counts of non-finite elements and of gradient elements
    equal to zero -- and advances a per-tensor history (mdx_tensor_stats_history: passes, passes with a non-finite gradient and
    the first and last of them, the first pass with a non-finite weight, the largest gradient norm and its pass).  The pass only
    reads: `.grad` is taken where the step left it and never written.  A guarded optimiser consumes g * coef without storing it,
    so these are the statistics of the UNCLIPPED gradients.

    Dense float32 GPU parameters on one device, contiguous or channels-last, with gradients that are float32 and have their
    parameter's strides (or are None: no gradient this pass) go through csrc/tensor_stats.hip: the table, block maps, slot
    offsets, partials, records, history and the gradient-pointer arrays are built HERE, nothing is allocated later, `compute()`
    launches without synchronising and is capturable, the history stays on the device, and the same inputs give the same bits.
    Anything else -- CPU parameters, `native = False`, a gradient of another dtype or layout -- takes torch's own functions in
    float64, which read on the host and cannot be captured; the records and the history are the same.  `host()`, `total_norm()`
    and `history()` are the only calls that synchronise.  The parameters must keep their storage.  The history belongs to this
    object: it is no part of any state_dict and does not survive a resumed run.  `names` default to "0", "1", ..."""

    native = True          # False: torch's own functions for every pass

    def __init__(self, params, names=None):
        if _capturing():
            raise _lib.MdxError("mdx.optim.GradStats: built while the current stream is being captured")
        self.params = list(params)
        self.tensors = [p.detach() for p in self.params]
        self.names = [str(i) for i in range(len(self.params))] if names is None else [str(n) for n in names]
        if not self.params:
            raise ValueError("GradStats: no parameters")
        if len(self.names) != len(self.params) or len(set(self.names)) != len(self.names):
            raise ValueError("GradStats: %d parameters need %d distinct names" % (len(self.params), len(self.params)))
        n = len(self.params)
        assert C.sizeof(TensorStats) == 40 and C.sizeof(TensorStatsHistory) == 56
        self._native = self._last_native = self._native_ok()          # _last_native: did the last pass take the kernels?
        self._table = self._launches = self._offsets = self._partials = None
        dev = self.tensors[0].device if self._native else torch.device("cpu")
        # 40 bytes = 5 words and 56 bytes = 7 words of 8: int64 storage is 8-byte aligned and all-zero is the history's initial state
        self._records = torch.zeros(n, 5, dtype=torch.int64, device=dev)
        self._history = torch.zeros(n, 7, dtype=torch.int64, device=dev)
        if self._native:
            assert (api.mdx_tensor_stats_partial_bytes(), api.mdx_tensor_stats_record_bytes(), api.mdx_tensor_stats_history_bytes()) == (40, 40, 56)
            self._table = _device_table(_StatsTable, api.mdx_tensor_stats_table_entry_bytes(), self.tensors)
            chunk = api.mdx_adam_chunk()
            offsets = [0]
            for t in self.tensors:
                offsets.append(offsets[-1] + (t.numel() + chunk - 1) // chunk)
            if offsets[-1] >= 1 << 31:
                raise ValueError("GradStats: %d chunks of %d elements do not fit the int32 slot offsets" % (offsets[-1], chunk))
            self._offsets = torch.tensor(offsets, dtype=torch.int32).to(dev)
            # each launch with the slot its slice of the partials starts at and its own host array of gradient pointers
            self._launches = [(first, count, blockmap, nblocks, offsets[first], (C.c_void_p * count)())
                              for first, count, blockmap, nblocks in _launches(self.tensors, 0)]
            self._partials = torch.empty(offsets[-1], 5, dtype=torch.int64, device=dev)
            self._key = _key(self.tensors)

    def _native_ok(self):
        dev = self.tensors[0].device
        return self.native and all(_dense_f32(t, dev) and t.numel() > 0 for t in self.tensors)

    def _grads_native(self, grads):
        dev = self.tensors[0].device
        return all(g is None or _dense_f32(g, dev, t) for g, t in zip(grads, self.tensors))

    @staticmethod
    def _torch_record(w, g):
        """One tensor's record by torch's own functions, sums in float64."""
        def half(t):
            t = t.detach()
            finite = torch.isfinite(t)
            kept = t[finite].double()
            return (float((kept * kept).sum()), float(kept.abs().max()) if kept.numel() else 0.0, int((~finite).sum()),
                    int((t == 0).sum()))
        wsum, wmax, wnf, _ = half(w)
        gsum, gmax, gnf, gz = half(g) if g is not None else (0.0, 0.0, 0, 0)
        return TensorStats(gsum, wsum, gmax, wmax, gnf & 0xFFFFFFFF, wnf & 0xFFFFFFFF, gz & 0xFFFFFFFF, int(g is not None))

    def _torch_compute(self, grads):
        if _capturing() and (self._records.is_cuda or any(t.is_cuda for t in self.tensors)):
            raise _lib.MdxError("mdx.optim.GradStats: the torch path reads the tensors on the host and cannot be captured")
        n = len(self.tensors)
        recs = (TensorStats * n)(*[self._torch_record(t, g) for t, g in zip(self.tensors, grads)])
        hist = (TensorStatsHistory * n).from_buffer_copy(self._history.cpu().numpy().tobytes())
        for r, h in zip(recs, hist):                       # include/mdx.h: mdx_tensor_stats_finish
            h.passes += 1
            if r.grad_nonfinite > 0:
                h.bad_passes += 1
                h.first_bad_pass = h.first_bad_pass or h.passes
                h.last_bad_pass = h.passes
            if r.weight_nonfinite > 0:
                h.first_bad_weight_pass = h.first_bad_weight_pass or h.passes
            if r.grad_present and r.grad_sumsq > h.max_grad_sumsq:
                h.max_grad_sumsq, h.max_grad_pass = r.grad_sumsq, h.passes
        self._records.copy_(host_tensor(recs, torch.int64).view(n, 5))
        self._history.copy_(host_tensor(hist, torch.int64).view(n, 7))

    @torch.no_grad()
    def compute(self, grads=None):
        """One pass over `grads` (default: every parameter's .grad as it is now; None entries are parameters without a gradient)
        -> the record buffer (int64 [tensors, 5]: the 40 bytes of each mdx_tensor_stats; the same tensor at every call), on the
        parameters' device without a synchronisation on the native path, on the host otherwise."""
        grads = [p.grad for p in self.params] if grads is None else list(grads)
        if len(grads) != len(self.params):
            raise ValueError("GradStats: %d gradients for %d parameters" % (len(grads), len(self.params)))
        self._last_native = self._native and self._grads_native(grads)
        if not self._last_native:
            self._torch_compute(grads)
            return self._records
        _check_device("GradStats: parameters", self.tensors[0].device)
        _check_storage("GradStats: a parameter has", self.tensors, self._key)
        table, partials, s = self._table.data_ptr(), self._partials.data_ptr(), stream()
        for first, count, blockmap, nblocks, slot, garr in self._launches:
            for i in range(count):
                g = grads[first + i]
                garr[i] = None if g is None else g.data_ptr()
            api.mdx_tensor_stats_partials(table, first, count, garr, blockmap.data_ptr(), nblocks, partials + 40 * slot, s)
        for first, count, _, _, _, _ in self._launches:
            api.mdx_tensor_stats_finish(first, count, self._offsets.data_ptr(), partials, self._records.data_ptr(),
                                        self._history.data_ptr(), s)
        return self._records

    def _read(self, what, buf, struct_type):
        return read_structs("mdx.optim.GradStats." + what, buf, struct_type, len(self.tensors))

    def host(self):
        """{name: {grad_norm, weight_norm, grad_absmax, weight_absmax, grad_nonfinite, weight_nonfinite, grad_zeros, grad_present,
        numel}} of the last pass; the square roots are taken here, in double.  Reads the records: synchronises, computes nothing."""
        out = {}
        for n, t, r in zip(self.names, self.tensors, self._read("host", self._records, TensorStats)):
            out[n] = dict(grad_norm=math.sqrt(r.grad_sumsq), weight_norm=math.sqrt(r.weight_sumsq), grad_absmax=r.grad_absmax,
                          weight_absmax=r.weight_absmax, grad_nonfinite=r.grad_nonfinite, weight_nonfinite=r.weight_nonfinite,
                          grad_zeros=r.grad_zeros, grad_present=r.grad_present, numel=t.numel())
        return out

    def total_norm(self):
        """The L2 norm of every finite gradient element of the last pass, in double.  Synchronises."""
        return math.sqrt(math.fsum(r.grad_sumsq for r in self._read("total_norm", self._records, TensorStats)))

    def history(self):
        """{name: {passes, bad_passes, first_bad_pass, last_bad_pass, first_bad_weight_pass, max_grad_norm, max_grad_pass}} since
        construction or the last reset_history(); pass numbers are 1-based, 0 is "never".  Synchronises."""
        out = {}
        for n, h in zip(self.names, self._read("history", self._history, TensorStatsHistory)):
            out[n] = dict(passes=h.passes, bad_passes=h.bad_passes, first_bad_pass=h.first_bad_pass, last_bad_pass=h.last_bad_pass,
                          first_bad_weight_pass=h.first_bad_weight_pass, max_grad_norm=math.sqrt(h.max_grad_sumsq),
                          max_grad_pass=h.max_grad_pass)
        return out

    def reset_history(self):
        if _capturing():
            raise _lib.MdxError("mdx.optim.GradStats.reset_history() is not part of a pass and the current stream is being captured")
        self._history.zero_()
