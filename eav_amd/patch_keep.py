"""Patch dropout of transformer.Encoder (timm.layers.PatchDropout): the plan of who is kept, the checks of an explicit
table, and the launches of csrc/patch_keep.hip that produce the tables.

A training forward with Encoder.patch_dropout > 0 runs at encoder_config.patch_dropout_geometry: K of the P patches of every
sample, the readout tokens always.  keep (int32 [B, K], ascending per row) and inv (int32 [B, P], slot or -1) live on the
forward's workspace; the backward reads them and regenerates nothing.  The plan's keys are eav_hash32 of (the seed of the
"patch_keep" entry of encoder_dropout.SITES under Encoder.dropout_seed, the device forward counter, b P + p): a captured
step draws a fresh subset on every replay, and mix_dropout_rank gives data-parallel replicas different ones.
"""
from __future__ import annotations

import torch

from . import _lib
from .encoder_config import patch_dropout_geometry
from .encoder_dropout import site_id, site_seed


def plan_seed(seed):
    """The seed the plan kernel takes for the model seed `seed`."""
    return site_seed(seed, site_id("patch_keep"))


def keep_plan(keep, inv, P, seed, counter=None, keys=None, stream=None):
    """eav_patch_keep_plan into keep [B, K] / inv [B, P] (int32, device); counter: a device int64 scalar or None, keys: an
    explicit uint32-valued int32 / uint32 [B, P] tensor or None."""
    B, K = keep.shape
    _lib.call("eav_patch_keep_plan", keep.data_ptr(), inv.data_ptr(), B, P, K, seed, _lib.ptr(counter), _lib.ptr(keys),
              _lib.stream_ptr() if stream is None else stream)


def check_table(idx):
    """An explicit keep table as Encoder.set_patch_keep takes it -> (int32 [B, K] contiguous tensor on idx's device, its
    largest index).  Rows must be ascending and unique, indices >= 0; the upper bound P, B and K belong to the forward that
    uses the table (EncoderPatchKeep.begin checks them against the kept numbers: no read-back there).  Reads the table back:
    call outside a capture."""
    t = torch.as_tensor(idx)
    if t.dim() != 2 or t.shape[1] < 1 or t.dtype not in (torch.int32, torch.int64, torch.int16, torch.uint8):
        raise ValueError(f"set_patch_keep: expected an integer [B, K] table, got {tuple(t.shape)} {t.dtype}")
    host = t.detach().cpu().to(torch.int64)
    if int(host.min()) < 0:
        raise ValueError("set_patch_keep: negative patch index")
    if host.shape[1] > 1 and not bool((host[:, 1:] > host[:, :-1]).all()):
        raise ValueError("set_patch_keep: every row must be ascending and unique")
    return t.detach().to(torch.int32).contiguous(), int(host.max())


class EncoderPatchKeep:
    """What Encoder's patch-dropout surface delegates to; `m` is the encoder."""

    def __init__(self, m):
        self.m = m
        self.table = None           # set_patch_keep: (int32 [B, K] tensor, largest index) or None

    def set_table(self, idx):
        if idx is None:
            self.table = None
            return
        t, top = check_table(idx)
        self.table = (t.to(next(self.m.parameters()).device), top)

    def buffers(self, c, B, dev):
        """keep / inv of a workspace of the patch-dropped geometry c."""
        return (torch.empty(B, c.npatch, dtype=torch.int32, device=dev),
                torch.empty(B, c.grid_npatch, dtype=torch.int32, device=dev))

    def begin(self, ws, B, dev):
        """Fill ws.keep / ws.inv for the forward in flight: from the explicit table (one launch: its inverse), else by the
        plan kernel from the device forward counter (which the encoder advances, once per forward, for all its generators)."""
        m, c = self.m, self.m._geo
        P, K = c.grid_npatch, c.npatch
        if self.table is not None:
            t, top = self.table
            if tuple(t.shape) != (B, K) or top >= P or t.device != dev:
                raise ValueError(f"set_patch_keep: this forward needs a [{B}, {K}] table of indices in [0, {P}) on {dev}, "
                                 f"got {tuple(t.shape)} with maximum {top} on {t.device}")
            ws.keep = t
            m._call("eav_patch_keep_invert", t.data_ptr(), ws.inv.data_ptr(), B, P, K, m._st)
            return
        ws.keep = ws.keep_own
        cnt = m._counter(dev)
        m._call("eav_patch_keep_plan", ws.keep.data_ptr(), ws.inv.data_ptr(), B, P, K, plan_seed(m.dropout_seed),
                cnt.data_ptr(), None, m._st)

    def generated(self, B, counter, seed=None, geo=None):
        m = self.m
        if geo is None:
            geo = m._active_geo if getattr(m._active_geo, "grid_npatch", None) is not None else \
                patch_dropout_geometry(m.cfg, m.patch_dropout)
        dev = next(m.parameters()).device
        cnt = torch.tensor(int(counter), dtype=torch.int64, device=dev)
        keep, inv = self.buffers(geo, B, dev)
        keep_plan(keep, inv, geo.grid_npatch, plan_seed(m.dropout_seed if seed is None else seed), cnt)
        return keep
