"""The fp16 hi/lo planes of the encoder's GEMM weights (transformer.Encoder, "split" precision): the planes and their
scale slots, the row / column norms behind the a-priori activation scales, what is stale after a parameter write, and the
events a reader waits for.  Imports _lib and torch only."""
from __future__ import annotations

import contextlib

import torch

from . import _lib

SLOT = 4128   # floats per scale slot (include/eav_hip.h EAV_SP_SLOT)


class WeightPlanes:
    # weight kind -> (norm array, 0: max_n ||W_n||_2 over the rows / 1: max_j ||W[:, j]||_2 over the columns).  The column
    # norms feed the backward only, so they exist while the planes HAVE transposes - not when one call needs them: a no_grad
    # forward right after an optimiser step refreshes everything without asking for transposes, and the next training step
    # finds nothing stale - its backward must still see the norms of the CURRENT weights.
    NORMS = {"fc1": ("wnorm_fc1", 0),        # input of the a-priori scale of the MLP activation (eav_tf_forward_scales)
             "qkv": ("wnorm_qkv", 0),        # bound of the fused q/k/v projection's output
             "fc2": ("wcolnorm_fc2", 1)}     # bound of the MLP hidden-state gradient (eav_sp_bound_scale)

    def __init__(self, mats, layers, dev, transposes):
        """mats: [(key, byte offset of the [out, in] matrix in the flat parameter buffer, out, in)], key = kind + layer
        ("fc13"; "patch" for the embedding).  transposes: also the planes of W^T (the data-gradient products)."""
        kp = lambda k: _lib.plain("eav_sp_kpad", k)  # noqa: E731
        self.mats, self.dev, self.T = mats, dev, transposes
        self.slots = torch.zeros(len(mats), SLOT, dtype=torch.float32, device=dev)
        for arr, _ in self.NORMS.values():
            setattr(self, arr, torch.zeros(layers, dtype=torch.float32, device=dev))
        self.planes, self._ptrs, self._norm = {}, {}, {}
        for n, (k, _, out, inn) in enumerate(mats):
            pl = torch.empty(out, 2 * kp(inn), dtype=torch.float16, device=dev)
            plT = torch.empty(inn, 2 * kp(out), dtype=torch.float16, device=dev) if transposes else None
            slot = self.slots.data_ptr() + 4 * SLOT * n
            self.planes[k] = (pl, plT, n)
            self._ptrs[k] = ((pl.data_ptr(), slot), (_lib.ptr(plT), slot))
            arr, col = self.NORMS.get(k[:3], (None, 0))
            if arr is not None and (transposes or not col):
                self._norm[k] = (getattr(self, arr), int(k[3:]), col)
        self.key = None                 # (flat.data_ptr(), versions) the planes were made from
        self.ready = {}                 # key -> event of the side-stream conversion of that matrix
        self.norm_ready = None          # event of the side-stream norms
        self.main = None                # the stream whose launches read the planes (set by the model per launch sequence)
        self._tables = None             # (base, plane jobs, norm jobs, number of norm jobs, their block count)

    def invalidate(self):
        self.key = None

    def stale(self, base, versions, dirty, need_T):
        """Keys of the matrices whose planes do not hold the weights at `base` (flat.data_ptr()): all of them if the base,
        the version counters or the need for transposes changed, else those a dirty byte range [lo, hi) touches.
        Launches nothing."""
        if self.key != (base, versions) or (need_T and not self.T):
            return [k for k, _, _, _ in self.mats]
        return [k for k, off, out, inn in self.mats
                if any(lo < base + off + 4 * out * inn and base + off < hi for lo, hi in dirty)]

    def get(self, key, transposed=False):
        """(planes, scale slot) pointers of a matrix (or of its transpose), once its refresh has finished."""
        ev = self.ready.pop(key, None)
        if ev is not None:
            self.main.wait_event(ev)
        return self._ptrs[key][transposed]

    def refresh(self, stale, base, versions, side):
        """Rebuild the planes (and norms) of the `stale` keys from the weights at `base`, on `side` if that is a stream.

        After an optimiser step every matrix is stale: ~100 small launches (max|w| + conversion per matrix), or two for
        the whole table.  They go to the side stream - idle during the forward - in layer order, one event per matrix; the
        main stream waits for a matrix's event right before the first GEMM that reads its planes (get), so only the patch
        projection's conversion is ever on the critical path."""
        self.ready, self.norm_ready = {}, None
        todo = [m for m in self.mats if m[0] in set(stale)]
        if side is not None:
            start = torch.cuda.Event()
            start.record()                      # the weights are final (the optimiser ran on this stream)
            side.wait_event(start)
        with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
            st = _lib.stream_ptr()
            if len(todo) == len(self.mats):
                self._refresh_all(base, side, st)
            else:
                self._refresh_some(todo, base, side, st)
        self.key = (base, versions)

    def _mark(self, side):
        ev = torch.cuda.Event()
        ev.record(side)
        return ev

    def _refresh_all(self, base, side, st):
        """Everything is stale (the state after an optimiser step): the whole table in two launches."""
        self.slots.zero_()
        self.wnorm_fc1.zero_()
        self.wcolnorm_fc2.zero_()
        self.wnorm_qkv.zero_()
        if self._tables is None or self._tables[0] != base:
            jobs, njobs, mb = [], [], 1
            for k, off, out, inn in self.mats:
                (pl, slot), (plT, _) = self._ptrs[k]
                jobs.append([base + off, pl, plT or 0, slot, out | (inn << 32)])     # EavPlaneJob
                if k in self._norm:
                    arr, li, col = self._norm[k]
                    njobs.append([base + off, inn, arr.data_ptr() + 4 * li, out | (inn << 32), col])
                    mb = max(mb, (inn + 63) // 64 if col else min((out + 3) // 4, 128))
            self._tables = (base, torch.tensor(jobs, dtype=torch.int64).to(self.dev),
                            torch.tensor(njobs, dtype=torch.int64).to(self.dev), len(njobs), mb)
        _, jobs, njobs, nn, mb = self._tables
        # the row / column norms behind the a-priori scales FIRST (their own event: the forward's scales wait for
        # nothing else) and in one launch for the whole table (36 launches of ~10 us stood between the optimiser step
        # and the first scales of the next forward)
        if nn:
            _lib.call("eav_norm_max_multi", _lib.ptr(njobs), nn, mb, st)
        if side is not None:
            self.norm_ready = self._mark(side)
        _lib.call("eav_sp_refresh_planes", _lib.ptr(jobs), len(self.mats), max(m[2] for m in self.mats),
                  max(m[3] for m in self.mats), st)
        if side is not None:
            self.ready = dict.fromkeys((m[0] for m in self.mats), self._mark(side))

    def _refresh_some(self, todo, base, side, st):
        """Some matrices are stale (a partial update): the row / column norms first - the a-priori scales of EVERY layer
        are computed by one launch before layer 0 and wait for ONE event (`norm_ready`), not for the conversions - then
        max|w| + conversion per matrix with one event each."""
        for k, off, out, inn in todo:
            if k in self._norm:
                arr, li, col = self._norm[k]
                arr[li].zero_()
                _lib.call("eav_colnorm_max" if col else "eav_rownorm_max", base + off, out, inn, inn,
                          arr.data_ptr() + 4 * li, st)
        if todo and side is not None:
            self.norm_ready = self._mark(side)
        for k, off, out, inn in todo:
            (pl, slot), (plT, _) = self._ptrs[k]
            self.slots[self.planes[k][2]].zero_()
            _lib.call("eav_sp_absmax", base + off, out, inn, inn, slot, st)
            _lib.call("eav_sp_convert", base + off, out, inn, inn, slot, pl, plT, st)
            if side is not None:
                self.ready[k] = self._mark(side)
