"""Block 1 of an EEGNet on the run-time-parametrised kernels of csrc/eegnet_canon.hip: what cnn_eeg.EEGNet and the
generic path of eegnet.EEGNet_tor share.

    temporal conv (1 -> F1, kernLength taps) -> BatchNorm -> [ELU] -> depthwise spatial conv (F1 -> F1*D over Chans)
        -> BatchNorm -> ELU -> AvgPool4 -> Dropout

Workspace holds its buffers and those of both BatchNorm -> ELU -> pool tails; the two models add block 2's.  `m` is the
KernelModule (Chans, Samples, F1, D, F2, kernLength); `elu` is the ELU flag of eav_spatial_* (EEGNet_tor has one after
the first BatchNorm, cnn_eeg.EEGNet has none); `dropout` = (rate, seed, mask pointer, counter pointer) of the tail.
"""
from __future__ import annotations

from typing import Any, Callable, NamedTuple, Optional

import torch

from . import _lib
from .runtime import BN_M1, BN_M2, bn_field


class Saved(NamedTuple):
    """What a forward of either EEGNet keeps for its backward (KernelModule._saved: the token first)."""
    token: int
    x: Any                      # the input: a tensor [B,1,Chans,Samples] (EEGNet_tor's fast path: or an IndexedBatch)
    training: bool
    drop1: tuple                # (rate, seed, mask pointer, counter pointer) of block 1's dropout
    drop2: tuple                # ... of block 2's
    mk: Callable                # keeps explicit masks alive
    ws: Any                     # the workspace of this forward
    probs: Optional[torch.Tensor] = None     # EEGNet_tor: the probabilities it returned


class Workspace:
    """Device buffers for one batch size (all fp32): y1 / g1 the temporal conv's output and its gradient, z2 / dz2 the
    spatial conv's, a2 / da2 block 1's pooled output, bn1..3 the BatchNorm parameter blocks, part_* the partial sums."""

    def __init__(self, m, B, dev):
        f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)  # noqa: E731
        C, S, F1, C2, F2, K = m.Chans, m.Samples, m.F1, m.F1 * m.D, m.F2, m.kernLength
        T2, T3 = S // 4, S // 4 // 8
        self.T2, self.T3, self.NF = T2, T3, F2 * T3
        self.y1, self.g1 = f(B, F1, C, S), f(B, F1, C, S)
        self.z2, self.dz2 = f(B, C2, S), f(B, C2, S)
        self.a2, self.da2 = f(B, C2, T2), f(B, C2, T2)
        self.bn1, self.bn2, self.bn3 = f(6 * F1), f(6 * C2), f(6 * F2)
        self.np_t = _lib.plain("eav_tconv_fwd_nparts", B, C, S, F1, K)
        self.part_t = f(self.np_t, 2 * F1)
        self.np_s = _lib.plain("eav_spatial_nparts", B, S)
        self.part_s = f(self.np_s, 2 * C2)
        self.part_pb = f(B, 2 * max(C2, F2))
        self.part_sst = f(self.np_s, 2 * F1)
        self.part_sw = f(self.np_s, C2 * C)
        self.np_tw = _lib.plain("eav_tconv_wgrad_nparts", B, C, S, F1, K)
        self.part_tw = f(self.np_tw, F1 * K)


def block1_forward(m, ws, x, w1, bn1, w2, bn2, elu, training, dropout):
    """x [B,1,Chans,Samples] -> ws.a2."""
    L, P, st = _lib.call, _lib.ptr, _lib.stream_ptr()
    B, C, S, F1, D = x.shape[0], m.Chans, m.Samples, m.F1, m.D
    L("eav_tconv_fwd", P(x), P(w1), P(ws.y1), P(ws.part_t), B, C, S, F1, m.kernLength, st)
    m._bn_finalize(bn1, ws.part_t, ws.np_t, B * C * S, ws.bn1, training)
    L("eav_spatial_fwd", P(ws.y1), P(ws.bn1), P(w2), P(ws.z2), P(ws.part_s), B, C, S, F1, D, elu, st)
    m._bn_finalize(bn2, ws.part_s, ws.np_s, B * S, ws.bn2, training)
    L("eav_bn_elu_pool_fwd", P(ws.z2), P(ws.bn2), P(ws.a2), B, F1 * D, S, 4, *dropout, st)


def block1_backward(m, ws, x, w2, grads, elu, training, dropout):
    """ws.da2 -> grads, the flat-gradient views of block 1's six parameters in forward order (temporal conv weight,
    BatchNorm weight / bias, spatial conv weight, BatchNorm weight / bias)."""
    L, P, st = _lib.call, _lib.ptr, _lib.stream_ptr()
    B, C, S, F1, D, K = x.shape[0], m.Chans, m.Samples, m.F1, m.D, m.kernLength
    C2, b1 = F1 * D, P(ws.bn1)
    gw1, gbn1w, gbn1b, gw2, gbn2w, gbn2b = grads
    m._bn_elu_pool_bwd(ws.da2, ws.z2, ws.dz2, ws.bn2, ws.part_pb, gbn2w, gbn2b, B, C2, S, 4, dropout, training)
    # spatial conv <- [ELU] <- BatchNorm, then the temporal conv's weight gradient (BatchNorm backward folded in)
    L("eav_spatial_bwd", P(ws.y1), P(ws.dz2), b1, P(w2), P(ws.g1), P(ws.part_sst), P(ws.part_sw), B, C, S, F1, D, elu, st)
    L("eav_reduce_partials", P(ws.part_sw), ws.np_s, C2 * C, C2 * C, 1.0, P(gw2), st)
    L("eav_bn_bwd_finalize", P(ws.part_sst), ws.np_s, F1, float(B * C * S), int(training), P(gbn1w), P(gbn1b),
      bn_field(ws.bn1, F1, BN_M1), bn_field(ws.bn1, F1, BN_M2), st)
    L("eav_tconv_wgrad", P(x), P(ws.y1), P(ws.g1), b1, P(ws.part_tw), B, C, S, F1, K, st)
    L("eav_reduce_partials", P(ws.part_tw), ws.np_tw, F1 * K, F1 * K, 1.0, P(gw1), st)
