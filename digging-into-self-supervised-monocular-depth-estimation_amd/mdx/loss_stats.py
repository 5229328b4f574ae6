"""`LossStats(B, H, W, S, scales_hw, automask)`: statistics of the maps the fused loss path leaves behind after a step, by
csrc/loss_stats.hip -- per (scale, image) how many pixels each arg-min channel won (with the auto-mask: how many the mask removed),
how many indices are corrupt, and the sum, sum of squares, smallest and largest finite disparity; per scale a history kept on the
device: the masked share over the passes, static images, the smallest disparity range, passes with a corrupt map.  A read-only,
capturable, deterministic pass, for the two failures the scalar loss does not show: a scene that does not move and a disparity that
collapses to a constant."""
import ctypes as C
import math

import torch

from . import _lib
from ._lib import _capturing, api, host_tensor, read_structs, stream

BINS = 2 * _lib.MAX_SRC


class LossStatsRecord(C.Structure):        # include/mdx.h: mdx_loss_stats
    _fields_ = [("disp_sum", C.c_double), ("disp_sumsq", C.c_double), ("disp_min", C.c_float), ("disp_max", C.c_float),
                ("winner", C.c_uint32 * BINS), ("bad_index", C.c_uint32), ("disp_nonfinite", C.c_uint32),
                ("index_present", C.c_uint32), ("disp_present", C.c_uint32)]


class LossStatsHistory(C.Structure):       # include/mdx.h: mdx_loss_stats_history
    _fields_ = [("passes", C.c_int64), ("images", C.c_int64), ("winner_total", C.c_int64 * BINS), ("bad_passes", C.c_int64),
                ("first_bad_pass", C.c_int64), ("static_images", C.c_int64), ("first_static_pass", C.c_int64),
                ("last_static_pass", C.c_int64), ("max_masked_share", C.c_double), ("max_masked_pass", C.c_int64),
                ("min_disp_range", C.c_double), ("min_disp_range_pass", C.c_int64)]


RECORD_WORDS, HISTORY_WORDS = C.sizeof(LossStatsRecord) // 8, C.sizeof(LossStatsHistory) // 8


class LossStats(object):
    """Statistics of `outputs[("automask", s)]` (the arg-min channel of every pixel, [B,H,W], always full resolution) and
    `outputs[("disp", s)]` ([B,1,h,w] with `scales_hw[s] = (h, w)`) for all scales of a step at once.  `compute(idx_list, disp_list)`
    gives every (scale, image) a record (include/mdx.h: mdx_loss_stats) and advances a per-scale history (mdx_loss_stats_history).
    With the auto-mask the channels c < S are the identity reprojections -- a pixel won by one of them is MASKED -- and S <= c < 2S the
    warped sources; without it c < S are the sources and nothing is masked.  An image counts as static when at least `static_share`
    of its pixels are masked: a reporting threshold, not a tolerance.

    uint8 CUDA index maps and contiguous float32 CUDA disparities of the constructed shapes on the current device go through
    csrc/loss_stats.hip: the block map, partials, records, history and the host pointer arrays are built HERE, nothing is allocated
    later, `compute()` launches two kernels on the current stream without synchronising and is capturable, the history stays on the
    device, and the same inputs give the same bytes.  Anything else -- CPU tensors, `native = False`, the int64 indices torch.min
    returns on the op-by-op path -- takes torch's own functions with sums in float64, which read on the host and cannot be captured;
    the records and the history are the same.  Entries of either list may be None: that half of the scale's records is 0 and says
    "absent".  `host()` and `history()` are the only calls that synchronise.  The history belongs to this object alone."""

    native = True          # False: torch's own functions for every pass

    def __init__(self, B, H, W, S, scales_hw, automask, static_share=0.9, device="cuda"):
        if _capturing():
            raise _lib.MdxError("mdx.loss_stats.LossStats: built while the current stream is being captured")
        self.B, self.H, self.W, self.S, self.automask = int(B), int(H), int(W), int(S), bool(automask)
        self.scales_hw = [(int(h), int(w)) for h, w in scales_hw]
        self.static_share = float(static_share)
        n = len(self.scales_hw)
        if not 1 <= n <= _lib.MAX_SCALES or not 1 <= self.S <= _lib.MAX_SRC or min(self.B, self.H, self.W) < 1 \
                or self.H * self.W >= 1 << 32 or any(h < 1 or w < 1 for h, w in self.scales_hw):
            raise ValueError("LossStats: B %d, H %d, W %d, S %d, %d scales %s are out of range"
                             % (self.B, self.H, self.W, self.S, n, self.scales_hw))
        if not (0.0 < self.static_share <= 1.0):
            raise ValueError("LossStats: static_share %r is not in (0, 1]" % (static_share,))
        self.limit = 2 * self.S if self.automask else self.S
        if self.automask:
            self.channel_names = ["identity%d" % c for c in range(self.S)] + ["source%d" % c for c in range(self.S)]
        else:
            self.channel_names = ["source%d" % c for c in range(self.S)]
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._native = self._last_native = bool(self.native and self.device.type == "cuda")
        dev = self.device if self._native else torch.device("cpu")
        # 72 bytes = 9 words and 152 bytes = 19 words of 8: int64 storage is 8-byte aligned and all-zero is the history's initial state
        self._records = torch.zeros(n * self.B, RECORD_WORDS, dtype=torch.int64, device=dev)
        self._history = torch.zeros(n, HISTORY_WORDS, dtype=torch.int64, device=dev)
        self._h = (C.c_int * n)(*[h for h, _ in self.scales_hw])
        self._w = (C.c_int * n)(*[w for _, w in self.scales_hw])
        self._idx, self._disp = (C.c_void_p * n)(), (C.c_void_p * n)()
        self._blockmap = self._partials = None
        self.nblocks = 0
        if self._native:
            assert (api.mdx_loss_stats_record_bytes(), api.mdx_loss_stats_history_bytes()) \
                == (C.sizeof(LossStatsRecord), C.sizeof(LossStatsHistory))
            self.nblocks = api.mdx_loss_stats_plan(n, self.B, self.H, self.W, self._h, self._w, None)
            entry, slot = api.mdx_loss_stats_blockmap_entry_bytes(), api.mdx_loss_stats_partial_bytes()
            assert entry % 4 == 0 and slot % 8 == 0
            host = torch.empty(self.nblocks, entry // 4, dtype=torch.int32)
            assert api.mdx_loss_stats_plan(n, self.B, self.H, self.W, self._h, self._w, host.data_ptr()) == self.nblocks
            self._blockmap = host.to(dev)
            self._partials = torch.empty(self.nblocks, slot // 8, dtype=torch.int64, device=dev)

    # ---- what the lists must be ---------------------------------------------------------------------------------------------
    def _check_lists(self, idx_list, disp_list):
        n = len(self.scales_hw)
        idx_list, disp_list = list(idx_list), list(disp_list)
        if len(idx_list) != n or len(disp_list) != n:
            raise ValueError("LossStats: %d index maps and %d disparities for %d scales" % (len(idx_list), len(disp_list), n))
        for s, (i, d) in enumerate(zip(idx_list, disp_list)):
            if i is not None and (tuple(i.shape) != (self.B, self.H, self.W) or i.dtype not in (torch.uint8, torch.int64)):
                raise ValueError("LossStats: the index map of scale %d is %s %s, not uint8 or int64 %s"
                                 % (s, i.dtype, tuple(i.shape), (self.B, self.H, self.W)))
            if d is not None and (tuple(d.shape) != (self.B, 1) + self.scales_hw[s] or d.dtype != torch.float32):
                raise ValueError("LossStats: the disparity of scale %d is %s %s, not float32 %s"
                                 % (s, d.dtype, tuple(d.shape), (self.B, 1) + self.scales_hw[s]))
        return idx_list, disp_list

    def _maps_native(self, idx_list, disp_list):
        return (all(i is None or (i.is_cuda and i.device == self.device and i.dtype == torch.uint8 and i.is_contiguous())
                    for i in idx_list)
                and all(d is None or (d.is_cuda and d.device == self.device and d.is_contiguous()) for d in disp_list))

    # ---- torch's own functions ----------------------------------------------------------------------------------------------
    def _torch_record(self, idx, disp):
        """One image's record ([H,W] indices or None, [1,h,w] disparity or None) by torch's own functions, sums in float64."""
        r = LossStatsRecord()
        if idx is not None:
            v = idx.detach().reshape(-1).to("cpu", torch.int64)
            legal = (v >= 0) & (v < self.limit)
            counts = torch.bincount(v[legal], minlength=BINS).tolist()
            for c in range(BINS):
                r.winner[c] = counts[c]
            r.bad_index = int(v.numel() - int(legal.sum()))
            r.index_present = 1
        if disp is not None:
            x = disp.detach().reshape(-1).cpu()
            finite = torch.isfinite(x)
            kept = x[finite].double()
            r.disp_sum, r.disp_sumsq = float(kept.sum()), float((kept * kept).sum())
            if kept.numel():
                r.disp_min, r.disp_max = float(kept.min()), float(kept.max())
            r.disp_nonfinite = int((~finite).sum())
            r.disp_present = 1
        return r

    def _advance(self, h, recs, elements):
        """include/mdx.h: what mdx_loss_stats_finish does to one scale's history entry with the records of the scale's images
        (`elements`: h * w of one disparity image)."""
        pixels = self.H * self.W
        h.passes += 1
        bad = False
        for r in recs:
            bad = bad or r.bad_index > 0 or r.disp_nonfinite > 0
            if r.index_present:
                h.images += 1
                for c in range(BINS):
                    h.winner_total[c] += r.winner[c]
                if self.automask:
                    masked = sum(r.winner[c] for c in range(self.S))
                    if float(masked) >= self.static_share * float(pixels):
                        h.static_images += 1
                        h.first_static_pass = h.first_static_pass or h.passes
                        h.last_static_pass = h.passes
                    if masked / pixels > h.max_masked_share:
                        h.max_masked_share, h.max_masked_pass = masked / pixels, h.passes
            if r.disp_present and r.disp_nonfinite < elements:
                rng = float(r.disp_max) - float(r.disp_min)
                if h.min_disp_range_pass == 0 or rng < h.min_disp_range:
                    h.min_disp_range, h.min_disp_range_pass = rng, h.passes
        if bad:
            h.bad_passes += 1
            h.first_bad_pass = h.first_bad_pass or h.passes

    def _torch_compute(self, idx_list, disp_list):
        if _capturing():
            raise _lib.MdxError("mdx.loss_stats.LossStats: the torch path reads the maps on the host and cannot be captured")
        n, B = len(self.scales_hw), self.B
        recs = (LossStatsRecord * (n * B))()
        hist = (LossStatsHistory * n).from_buffer_copy(self._history.cpu().numpy().tobytes())
        for s in range(n):
            i, d = idx_list[s], disp_list[s]
            for b in range(B):
                recs[s * B + b] = self._torch_record(None if i is None else i[b], None if d is None else d[b])
            self._advance(hist[s], [recs[s * B + b] for b in range(B)], self.scales_hw[s][0] * self.scales_hw[s][1])
        self._records.copy_(host_tensor(recs, torch.int64).view(n * B, RECORD_WORDS))
        self._history.copy_(host_tensor(hist, torch.int64).view(n, HISTORY_WORDS))

    # ---- the pass ---------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def compute(self, idx_list, disp_list):
        """One pass over the step's maps (one entry per scale; None: absent) -> the record buffer (int64 [scales * B, 9]: the 72
        bytes of each mdx_loss_stats, scale-major; the same tensor at every call), on the device without a synchronisation on
        the native path."""
        idx_list, disp_list = self._check_lists(idx_list, disp_list)
        self._last_native = self._native and self._maps_native(idx_list, disp_list)
        if not self._last_native:
            self._torch_compute(idx_list, disp_list)
            return self._records
        if self.device.index != torch.cuda.current_device():
            raise _lib.MdxError("mdx.loss_stats.LossStats: built for %s but the current device is cuda:%d"
                                % (self.device, torch.cuda.current_device()))
        n = len(self.scales_hw)
        for s in range(n):
            self._idx[s] = None if idx_list[s] is None else idx_list[s].data_ptr()
            self._disp[s] = None if disp_list[s] is None else disp_list[s].data_ptr()
        st = stream()
        api.mdx_loss_stats_partials(n, self.B, self.H, self.W, self.S, int(self.automask), self._h, self._w, self._idx, self._disp,
                                    self._blockmap.data_ptr(), self.nblocks, self._partials.data_ptr(), st)
        api.mdx_loss_stats_finish(n, self.B, self.H, self.W, self.S, int(self.automask), self._h, self._w, self.static_share,
                                  self._partials.data_ptr(), self._records.data_ptr(), self._history.data_ptr(), st)
        return self._records

    def records(self):
        """The records of the last pass as ctypes structures, [scale][image].  Synchronises."""
        n, B = len(self.scales_hw), self.B
        recs = read_structs("mdx.loss_stats.LossStats.records", self._records, LossStatsRecord, n * B)
        return [[recs[s * B + b] for b in range(B)] for s in range(n)]

    def host(self):
        """[scale][image] -> {masked_share, shares: {channel name: share of the pixels}, disp_min, disp_max, disp_mean, disp_std
        (over the finite elements, in double), bad_index, disp_nonfinite, index_present, disp_present} of the last pass.  Reads the
        records: synchronises, computes nothing on the device."""
        pixels = self.H * self.W
        out = []
        for s, recs in enumerate(self.records()):
            elements = self.scales_hw[s][0] * self.scales_hw[s][1]
            rows = []
            for r in recs:
                masked = sum(r.winner[c] for c in range(self.S)) if self.automask else 0
                finite = elements - r.disp_nonfinite if r.disp_present else 0
                mean = r.disp_sum / finite if finite else 0.0
                var = max(r.disp_sumsq / finite - mean * mean, 0.0) if finite else 0.0
                rows.append(dict(masked_share=masked / pixels,
                                 shares={name: r.winner[c] / pixels for c, name in enumerate(self.channel_names)},
                                 disp_min=r.disp_min, disp_max=r.disp_max, disp_mean=mean, disp_std=math.sqrt(var),
                                 bad_index=r.bad_index, disp_nonfinite=r.disp_nonfinite, index_present=r.index_present,
                                 disp_present=r.disp_present))
            out.append(rows)
        return out

    def history(self):
        """One dict per scale: the fields of mdx_loss_stats_history since construction or the last reset_history() (pass numbers
        are 1-based, 0 is "never"), and from them `masked_share` and `shares` over all images of all passes.  Synchronises."""
        pixels = self.H * self.W
        out = []
        for h in read_structs("mdx.loss_stats.LossStats.history", self._history, LossStatsHistory, len(self.scales_hw)):
            total = h.images * pixels
            masked = sum(h.winner_total[c] for c in range(self.S)) if self.automask else 0
            out.append(dict(passes=h.passes, images=h.images, winner_total=list(h.winner_total), bad_passes=h.bad_passes,
                            first_bad_pass=h.first_bad_pass, static_images=h.static_images, first_static_pass=h.first_static_pass,
                            last_static_pass=h.last_static_pass, max_masked_share=h.max_masked_share,
                            max_masked_pass=h.max_masked_pass, min_disp_range=h.min_disp_range,
                            min_disp_range_pass=h.min_disp_range_pass, masked_share=masked / total if total else 0.0,
                            shares={name: (h.winner_total[c] / total if total else 0.0)
                                    for c, name in enumerate(self.channel_names)}))
        return out

    def reset_history(self):
        if _capturing():
            raise _lib.MdxError("mdx.loss_stats.LossStats.reset_history() is not part of a pass and the current stream is being captured")
        self._history.zero_()

