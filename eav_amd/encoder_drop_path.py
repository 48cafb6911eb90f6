"""Stochastic depth of transformer.Encoder (timm.layers.DropPath, `drop_path_rate`): the rates, the site ids, the scale table
of one forward, and the checks of an explicit keep table.

In training mode with Encoder.drop_path_rate = r > 0, sample b of layer i drops a whole residual branch with probability
p_i = r i / (L - 1) (torch.linspace(0, r, L)), the kept ones are scaled by 1 / (1 - p_i); both branches of a layer use p_i, with
independent draws.  One launch per forward (eav_drop_path_plan, csrc/drop_path.hip) fills the scale table float32 [L, 2, B] on
the forward's workspace - row (i, 0) the attention branch, row (i, 1) the MLP branch; the layer schedules read it at the two
sites "o_proj / fc2 output before the residual add", and the backward reads the same table: nothing is regenerated.  The draws
are eav_hash32 of (the site seed under Encoder.dropout_seed, the device forward counter, b): a captured step draws a fresh
table on every replay, and mix_dropout_rank gives data-parallel replicas different ones.

The site ids sit above encoder_dropout.SITES["patch_keep"] and are no entries of SITES: dropout_sites(),
generated_dropout_masks() and set_dropout_masks() do not know them.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .encoder_dropout import SITES, site_seed

FIRST_SITE = SITES["patch_keep"][0] + 1          # the attention branch of layer 0; consecutive rows, consecutive ids


def site_ids(layer):
    """(id of the attention branch, id of the MLP branch) of a layer."""
    return FIRST_SITE + 2 * layer, FIRST_SITE + 1 + 2 * layer


def rates(rate, layers):
    """p_i = rate i / (L - 1) for the L layers (0 for L = 1), formed in float64 and rounded once: float32 [L]."""
    r = float(rate)
    return np.array([r * i / (layers - 1) if layers > 1 else 0.0 for i in range(layers)], np.float64).astype(np.float32)


def check_rate(rate):
    r = float(rate)
    if not 0.0 <= r < 1.0:
        raise ValueError(f"drop_path_rate must satisfy 0 <= r < 1, got {rate!r}")
    return r


def plan_seed(seed):
    """The seed the plan kernel takes for the model seed `seed`: the site seed of row 0 (row r adds r << 40)."""
    return site_seed(seed, FIRST_SITE)


def plan(scale, rate, seed, counter=None, keep=None, stream=None):
    """eav_drop_path_plan into scale (float32 [L, 2, B], device); counter: a device int64 scalar or None, keep: an explicit
    uint8 [L, 2, B] device tensor or None."""
    L, _, B = scale.shape
    _lib.call("eav_drop_path_plan", scale.data_ptr(), L, B, float(rate), seed, _lib.ptr(counter), _lib.ptr(keep),
              _lib.stream_ptr() if stream is None else stream)


class DropPathState:
    """Stochastic depth of one forward, kept on its workspace for the backward: the rates as Python floats and the device
    address of every row of the scale table."""

    def __init__(self, p, table):
        self.p, self.table = [float(v) for v in p], table
        L, _, B = table.shape
        self.rows = [table.data_ptr() + 4 * B * r for r in range(2 * L)]

    def on(self, layer):
        return self.p[layer] > 0.0

    def row(self, layer, branch):
        return self.rows[2 * layer + branch]


class EncoderDropPath:
    """What Encoder's stochastic-depth surface delegates to; `m` is the encoder."""

    def __init__(self, m):
        self.m = m
        self.masks = None           # set_drop_path_masks: a uint8 [L, 2, B] device tensor or None

    def rates(self):
        return rates(check_rate(self.m.drop_path_rate), self.m.cfg.layers)

    def active(self):
        """Whether the forward about to run drops branches (the rate is validated whatever the mode)."""
        m = self.m
        return check_rate(m.drop_path_rate) > 0.0 and m.training and m.cfg.layers > 1

    def generates(self):
        return self.active() and self.masks is None

    def set_masks(self, mask):
        """An explicit keep table: validated here, once (shape against the model's layer count, dtype, device) - B belongs
        to the forward that uses it."""
        if mask is None:
            self.masks = None
            return
        m = self.m
        dev = next(m.parameters()).device
        if not (isinstance(mask, torch.Tensor) and mask.dtype == torch.uint8 and mask.dim() == 3
                and tuple(mask.shape[:2]) == (m.cfg.layers, 2) and mask.shape[2] >= 1):
            got = (tuple(mask.shape), mask.dtype) if isinstance(mask, torch.Tensor) else type(mask).__name__
            raise ValueError(f"set_drop_path_masks: expected a uint8 tensor [{m.cfg.layers}, 2, B], got {got}")
        if mask.device != dev:
            raise ValueError(f"set_drop_path_masks: the table must live on {dev}, not on {mask.device}")
        self.masks = mask.detach().contiguous()

    def begin(self, ws, B, dev):
        """The DropPathState of this forward, left on the workspace (None: nothing drops): one launch fills the scale table,
        from the explicit keep table or from the device forward counter (which the encoder has advanced)."""
        ws.dpath = None
        if not self.active():
            return None
        m = self.m
        L = m.cfg.layers
        if getattr(ws, "dp_scale", None) is None:
            ws.dp_scale = torch.empty(L, 2, B, dtype=torch.float32, device=dev)
        if ws.full and ws.dhd is None:          # dh[b] s[b]: what enters the fc2 / o_proj gradient products
            ws.dhd = torch.empty(ws.M, m.cfg.hidden, dtype=torch.float32, device=dev)
        keep, cnt = self.masks, None
        if keep is not None:
            if tuple(keep.shape) != (L, 2, B) or keep.device != dev:
                raise ValueError(f"set_drop_path_masks: this forward needs a [{L}, 2, {B}] table on {dev}, got "
                                 f"{tuple(keep.shape)} on {keep.device}")
        else:
            cnt = m._counter(dev)
        m._call("eav_drop_path_plan", ws.dp_scale.data_ptr(), L, B, float(m.drop_path_rate), plan_seed(m.dropout_seed),
                _lib.ptr(cnt), _lib.ptr(keep), m._st)
        ws.dpath = DropPathState(self.rates(), ws.dp_scale)
        return ws.dpath

    def generated(self, B, counter, seed=None):
        """The keep table uint8 [L, 2, B] of the forward whose counter value is `counter` (rows with p_i = 0: all ones)."""
        m = self.m
        dev = next(m.parameters()).device
        cnt = torch.tensor(int(counter), dtype=torch.int64, device=dev)
        scale = torch.empty(m.cfg.layers, 2, B, dtype=torch.float32, device=dev)
        plan(scale, check_rate(m.drop_path_rate), plan_seed(m.dropout_seed if seed is None else seed), cnt)
        return (scale != 0).to(torch.uint8)
