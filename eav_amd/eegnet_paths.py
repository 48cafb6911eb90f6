"""The two launch schedules of eegnet.EEGNet_tor, one class each.

    FastPath      the specialised kernels of the reference configuration (F1=8, D=8, F2=64, kernLength<=300, Chans<=32):
                  FFT or MFMA firstConv, direct or frequency-domain separableConv, the eval-mode step's shortcuts, the
                  fused no-grad forward; reads an IndexedBatch in place and can merge GraphStep's step begin into its
                  counter launch
    GenericPath   every other width the reference constructor accepts, on the run-time-parametrised kernels of
                  csrc/eegnet_canon.hip (block 1: eegnet_canon); gathers an IndexedBatch first

Each owns its workspace class and its forward / backward sequence: `forward(x) -> token`, `backward(dprobs) -> grads`.  The
model (`m`) keeps what both read: the parameters and their flat gradients, the workspace cache (`_ws` / `_wss`), the token and
the saved forward (`_saved`), the dropout state, the input tables of its data sets (`_xtabs`) and the user-visible switches
(`fir_algo`, `fir_xtab`, `conv_algo`, `conv_fuse`, `fused_eval`, `apply_max_norm`).  Plain objects, not nn.Modules: they register nothing with the model.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import _lib, eegnet_canon
from .eegnet_canon import Saved
from .runtime import BN_M1, BN_M2, bn_field

_PARAM_ORDER = [
    "firstConv.weight", "firstBN.weight", "firstBN.bias",
    "depthwiseConv.weight", "depthwiseBN.weight", "depthwiseBN.bias",
    "separableConv.weight", "separableBN.weight", "separableBN.bias",
    "dense.weight", "dense.bias",
]


class IndexedBatch:
    """A batch addressed in place: samples `idx` (device int64 [B]) of an HBM-resident data set `data` [N,1,C,S].  The FIR
    kernels - the only readers of the network input - take the index vector, so no gathered copy of the batch is made.
    `step_begin` (EEGNet_tor.forward_batch): the arguments of eav_step_begin behind the counters - (optimiser step counter,
    labels, idx, targets, batch) as raw pointers - for a forward that can issue them with its own counter launch; that
    forward sets `merged`.  `xtab` (EEGNet_tor.forward_batch): the InputTables of `data`, or None."""

    def __init__(self, data, idx, step_begin=None, xtab=None):
        self.data, self.idx = data, idx
        self.shape = (idx.numel(),) + tuple(data.shape[1:])
        self.device = data.device
        self.step_begin, self.merged = step_begin, False
        self.xtab = xtab


class InputTables:
    """What the train-mode FFT weight gradient needs of y1 = firstConv(x), as a function of x alone: per trial of the
    HBM-resident data set `data` [N,1,C,S] the K x K matrix A_b[j,k] = sum_c sum_t xp[t+j] xp[t+k] and the K window sums X1_b
    (eav_eegnet_fir_xtab_build; 4 (K K + K) bytes per trial: 361 KB at 300 taps, 72 MB for 200 trials).  With them
    eav_eegnet_fir_wgrad_fft_xtab skips the 614 MB read of y1.  Built once per data set, outside any step; `version` is
    data._version at build time.  build() rewrites `tab` IN PLACE: a captured step keeps its pointer."""

    def __init__(self, data, klen):
        self.data, self.klen = data, klen
        self.tab = torch.empty(self.floats(data.shape[0], klen), dtype=torch.float32, device=data.device)
        self.build()

    @staticmethod
    def floats(N, klen):
        return _lib.plain("eav_eegnet_fir_xtab_floats", N, klen)

    def build(self):
        N, _, C, S = self.data.shape
        _lib.call("eav_eegnet_fir_xtab_build", _lib.ptr(self.data), N, C, S, self.klen, _lib.ptr(self.tab), _lib.stream_ptr())
        self.version = self.data._version


class BnBwdJob(NamedTuple):
    """One BatchNorm of eav_reduce_and_bn_bwd_finalize: partial sums [nparts][2n] -> the gradients of weight / bias and the
    two backward means m1 / m2.  BnBwdJob() is "no such job" in that launch."""
    part: Optional[int] = None
    nparts: int = 0
    n: int = 0
    count: float = 0.0
    training: int = 0
    gw: Optional[int] = None
    gb: Optional[int] = None
    m1: Optional[int] = None
    m2: Optional[int] = None


class _Path:
    def __init__(self, m):
        self.m = m

    @staticmethod
    def input_view(x):
        """(data pointer, index pointer or None, B) of a forward's input: a tensor [B,1,C,S] or an IndexedBatch."""
        if isinstance(x, IndexedBatch):
            return _lib.ptr(x.data), _lib.ptr(x.idx), x.shape[0]
        return _lib.ptr(x), None, x.shape[0]

    def input_tables(self, xs):
        """The InputTables a GraphStep batch of the data set `xs` carries (FastPath), or None."""
        return None

    def dropout_args(self, dev, training):
        """(counter pointer, block-1 and block-2 dropout arguments (rate, seed, mask pointer, counter pointer), mk)."""
        m = self.m
        drop = m.dropoutRate if training else 0.0
        if m.spatial_dropout:
            drop = -drop
        # dropout stream: effective seed = base + 2 * (device-resident count of training forwards) - no host
        # argument changes from step to step, so the whole step can be replayed from a hipGraph
        cnt, mk = m._dropout(dev, drop != 0.0)
        return cnt, (drop, m.dropout_seed, mk(0), cnt), (drop, m.dropout_seed + 1, mk(1), cnt), mk

    def counters(self, cnt, training):
        """The dropout step counter and the three BatchNorm step counters (nn.BatchNorm2d's num_batches_tracked)."""
        m = self.m
        bns = (m.firstBN, m.depthwiseBN, m.separableBN)
        return [cnt] + ([_lib.ptr(bn.num_batches_tracked) for bn in bns] if training else [None] * 3)


# ----------------------------------------------------------------------------- reference widths
class _Workspace:
    """Device buffers for one (B, Chans, Samples) problem size (all fp32)."""

    def __init__(self, B, C, S, klen, nb, dev):
        f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)  # noqa: E731
        self.key = (B, C, S)
        T2, T3 = S // 4, S // 4 // 8
        self.T2, self.T3, self.NF = T2, T3, 64 * T3
        nchunk = (S + 1023) // 1024
        self.nchunk = nchunk
        self.y1, self.g1 = f(B, 8, C, S), f(B, 8, C, S)
        self.z = f(B, 64, S)
        self.p2, self.dp2 = f(B, 64, T2), f(B, 64, T2)
        self.u3, self.du3 = f(B, 64, T2), f(B, 64, T2)
        self.p3, self.dp3 = f(B, 64 * T3), f(B, 64 * T3)
        self.bn1, self.bn2, self.bn3 = f(6 * 8), f(6 * 64), f(6 * 64)
        self.wTf, self.wTb = f(1024, 64), f(1024, 64)
        self.np_fir = _lib.plain("eav_eegnet_fir_fwd_nparts", B, C, S)
        self.np_fir_fft = _lib.plain("eav_eegnet_fir_fwd_fft_nparts", B, C, S)
        self.part_fir = f(max(self.np_fir, self.np_fir_fft), 16)
        self.fft_ws = None         # spectrum partials of the FFT weight gradient, allocated on first use
        self.part_dw = f(B * nchunk, 128)
        self.np_c3 = _lib.plain("eav_conv64_fwd_nparts", B, T2)
        self.np_c3_fft = _lib.plain("eav_conv64_fft_nparts", B, T2)
        self.part_c3 = f(max(self.np_c3, self.np_c3_fft), 128)
        self.c64_ws = None         # spectra workspace of the frequency-domain separableConv, allocated on first use
        self.part_pb = f(B, 128)
        self.part_dst = f(B * nchunk, 16)
        self.part_dw2 = f(B * nchunk, 64 * C)
        self.np_fw = _lib.plain("eav_eegnet_fir_wgrad_nparts", B, C, S)
        self.part_fw = f(self.np_fw, 8 * klen)
        self.np_cw = _lib.plain("eav_conv64_wgrad_nparts", B, T2)
        self.part_cw = f(self.np_cw, 64 * 1024)


class FastPath(_Path):
    """The schedule on the specialised fp32-MFMA / FFT kernels.  Per step it chooses once per stage: training or eval-mode
    step, FFT or MFMA firstConv (use_fft), frequency-domain or direct separableConv (use_conv_fft, with or without
    m.conv_fuse), and - a no-grad eval-mode forward with m.fused_eval - block 1 as one kernel."""
    st = None       # stream handle of the forward / backward in flight

    def use_fft(self):
        m = self.m
        if m.fir_algo not in ("auto", "fft", "mfma"):
            raise ValueError(f"fir_algo {m.fir_algo!r}: expected 'auto', 'fft' or 'mfma'")
        if m.fir_algo == "mfma" or m.kernLength > _lib.plain("eav_eegnet_fir_fft_max_taps"):
            return False
        return m.fir_algo == "fft" or m.Samples >= 1408

    def use_conv_fft(self, B):
        """separableConv (forward, data and weight gradient) in the frequency domain (csrc/eegnet_conv64_fft.hip: per-bin
        [128 x 128] GEMMs instead of a 1024-deep contraction, 6x fewer multiply-adds) when the batch is large enough to
        amortise its extra launches; the direct fp32-MFMA kernels otherwise (the reference's own [32,1,30,500]).
        `conv_algo` / EAV_CONV_ALGO: "auto" (default), "fft", "mfma"."""
        m = self.m
        if m.conv_algo not in ("auto", "fft", "mfma"):
            raise ValueError(f"conv_algo {m.conv_algo!r}: expected 'auto', 'fft' or 'mfma'")
        if m.conv_algo == "mfma":
            return False
        return m.conv_algo == "fft" or B * (m.Samples // 4) >= 40000

    def step_begin_args(self, optimizer, ys, idx, targets):
        """What EEGNet_tor.forward_batch hands to the forward's counter launch (IndexedBatch.step_begin)."""
        return (optimizer.device_step_counter().data_ptr(), ys.data_ptr(), idx.data_ptr(), targets.data_ptr(), idx.numel())

    def input_tables(self, xs):
        """Train-mode step on the FFT FIR path with m.fir_xtab on: the InputTables of the data set `xs`, kept in m._xtabs
        for the life of the model (a captured step holds their pointer).  Built here on first use and rebuilt in place when
        xs._version has moved on - never during capture, where only tables that exist are used.  None (the y1-reading weight
        gradient) for any other step, and when the tables would exceed m.fir_xtab_budget bytes."""
        m = self.m
        if not (m.fir_xtab and m.training and self.use_fft()):
            return None
        key = (xs.data_ptr(), tuple(xs.shape), m.kernLength)
        t = m._xtabs.get(key)
        capturing = torch.cuda.is_current_stream_capturing()
        if t is None:
            if capturing or 4 * InputTables.floats(xs.shape[0], m.kernLength) > m.fir_xtab_budget:
                return None
            t = m._xtabs[key] = InputTables(xs, m.kernLength)
        elif t.version != xs._version and not capturing:
            t.build()
        return t

    # ------------------------------------------------------------------ forward
    def forward(self, x):
        m = self.m
        self.st = _lib.stream_ptr()         # the stream of this sequence, looked up once for its stages
        xp, xidx, B = self.input_view(x)
        C, S = m.Chans, m.Samples
        ws = m._workspace((B, C, S, str(x.device)), lambda: _Workspace(B, C, S, m.kernLength, m.nb_classes, x.device))
        training = bool(m.training)
        m._token += 1
        cnt, drop1, drop2, mk = self.dropout_args(x.device, training)
        conv_fft = self.use_conv_fft(B)
        # (an IndexedBatch - xidx is set - may carry GraphStep's step begin)
        begin = x.step_begin if xidx is not None else None
        if self.begin_step(ws, cnt, training, conv_fft, begin):
            x.merged = True
        if m.fused_eval and m._infer and not training and S % 4 == 0:
            self.block1_infer(ws, xp, xidx, B)
        else:
            self.fir_forward(ws, xp, xidx, B, training)
            self.block1_tail_forward(ws, B, training, drop1)
        self.separable_forward(ws, B, training, conv_fft)
        probs = self.head_forward(ws, B, drop2, x.device)
        m._saved = Saved(m._token, x, training, drop1, drop2, mk, ws, probs)      # (mk keeps explicit masks alive)
        return m._token

    def begin_step(self, ws, cnt, training, conv_fft, begin):
        """The step's counters in one launch, with what else that launch can carry; True: it took `begin` (eav_step_begin)."""
        L, P, st = _lib.call, _lib.ptr, self.st
        counters = self.counters(cnt, training)
        if not conv_fft:    # (the frequency-domain separableConv takes the weight tensor as it is)
            # per-step prologue: the transposed separableConv weights of the direct kernels + the counters.  (`begin` is not
            # taken: GraphStep issues its own launches)
            L("eav_eegnet_step_prologue", P(self.m.separableConv.weight), P(ws.wTf), P(ws.wTb), *counters, st)
        elif begin is not None:
            # ... and, in a captured step (GraphStep), the optimiser's step count and the gather of the batch's labels with them
            L("eav_step_begin", *counters, *begin, st)
            return True
        elif cnt is not None or training:
            # library kernels, no torch op inside a captured step
            L("eav_counter_inc4", *counters, st)
        return False

    def block1_infer(self, ws, xp, xidx, B):
        """validate(): x -> block-1 output in ONE kernel (FIR -> firstBN -> ELU -> depthwiseConv -> depthwiseBN -> ELU ->
        AvgPool4; BatchNorms on running statistics): y1 (614 MB at [64,1,30,10000]) and z are never written."""
        m, P = self.m, _lib.ptr
        C, S = m.Chans, m.Samples
        m._bn_finalize(m.firstBN, ws.part_fir, ws.np_fir, B * C * S, ws.bn1, False)       # eval mode: running statistics only
        m._bn_finalize(m.depthwiseBN, ws.part_dw, B * ws.nchunk, B * S, ws.bn2, False)
        _lib.call("eav_eegnet_block1_infer", xp, xidx, P(m.firstConv.weight), P(ws.bn1), P(m.depthwiseConv.weight), P(ws.bn2),
                  P(ws.p2), B, C, S, m.kernLength, self.st)

    def fir_forward(self, ws, xp, xidx, B, training):
        """firstConv -> ws.y1, firstBN's parameters -> ws.bn1."""
        m, L, P, st = self.m, _lib.call, _lib.ptr, self.st
        C, S, K, w1 = m.Chans, m.Samples, m.kernLength, P(m.firstConv.weight)
        if self.use_fft():
            np_fir = ws.np_fir_fft
            pf = P(ws.part_fir) if training else None      # eval mode: firstBN needs no batch statistics
            L("eav_eegnet_fir_fwd_fft", xp, xidx, w1, P(ws.y1), pf, B, C, S, K, st)
        else:
            np_fir = ws.np_fir
            if xidx is None:
                L("eav_eegnet_fir_fwd", xp, w1, P(ws.y1), P(ws.part_fir), B, C, S, K, st)
            else:
                L("eav_eegnet_fir_fwd_indexed", xp, xidx, w1, P(ws.y1), P(ws.part_fir), B, C, S, K, st)
        m._bn_finalize(m.firstBN, ws.part_fir, np_fir, B * C * S, ws.bn1, training)

    def block1_tail_forward(self, ws, B, training, drop1):
        """ws.y1 -> firstBN -> ELU -> depthwiseConv (ws.z) -> depthwiseBN -> ELU -> AvgPool4 -> Dropout -> ws.p2."""
        m, L, P, st = self.m, _lib.call, _lib.ptr, self.st
        C, S, w2, bn2 = m.Chans, m.Samples, P(m.depthwiseConv.weight), m.depthwiseBN
        drop, m1 = drop1[0], drop1[2]
        if not training and drop == 0.0 and m1 is None and S % 4 == 0:
            # eval-mode step (what 349 of the reference's 350 epochs run, Q4): depthwiseBN's scale / shift come from the
            # running statistics, i.e. they are known BEFORE the depthwise pass - which then leaves the pooled block-1
            # output too (z is still written: the backward forms dz from it); one launch and one pass over z less
            m._bn_finalize(bn2, ws.part_dw, B * ws.nchunk, B * S, ws.bn2, training)
            L("eav_eegnet_dw_fwd_pool_eval", P(ws.y1), P(ws.bn1), w2, P(ws.z), P(ws.part_dw), P(ws.bn2), P(ws.p2), B, C, S,
              st)
        else:
            L("eav_eegnet_dw_fwd", P(ws.y1), P(ws.bn1), w2, P(ws.z), P(ws.part_dw), B, C, S, st)
            m._bn_finalize(bn2, ws.part_dw, B * ws.nchunk, B * S, ws.bn2, training)
            L("eav_bn_elu_pool_fwd", P(ws.z), P(ws.bn2), P(ws.p2), B, 64, S, 4, *drop1, st)

    def separable_forward(self, ws, B, training, conv_fft):
        """ws.p2 -> separableConv (ws.u3), separableBN's parameters -> ws.bn3."""
        m, L, P, st = self.m, _lib.call, _lib.ptr, self.st
        if conv_fft:
            if ws.c64_ws is None:
                ws.c64_ws = torch.zeros(_lib.plain("eav_conv64_fft_ws_floats", B, ws.T2), dtype=torch.float32,
                                        device=ws.y1.device)
            np_c3 = ws.np_c3_fft
            L("eav_conv64_fft_fwd", P(ws.p2), P(m.separableConv.weight), P(ws.u3), P(ws.part_c3), P(ws.c64_ws), B, ws.T2, 0,
              st)
        else:
            np_c3 = ws.np_c3
            L("eav_conv64_fwd", P(ws.p2), P(ws.wTf), P(ws.u3), P(ws.part_c3), B, ws.T2, 7, st)
        m._bn_finalize(m.separableBN, ws.part_c3, np_c3, B * ws.T2, ws.bn3, training)

    def head_forward(self, ws, B, drop2, dev):
        """ws.u3 -> separableBN -> ELU -> AvgPool8 -> Dropout (ws.p3) -> dense -> softmax, then the max-norm renorm."""
        m, L, P, st = self.m, _lib.call, _lib.ptr, self.st
        nb, wd = m.nb_classes, P(m.dense.weight)
        L("eav_bn_elu_pool_fwd", P(ws.u3), P(ws.bn3), P(ws.p3), B, 64, ws.T2, 8, *drop2, st)
        probs = torch.empty(B, nb, dtype=torch.float32, device=dev)   # fresh per forward: returned, kept for backward
        L("eav_dense_softmax_fwd", P(ws.p3), wd, P(m.dense.bias), None, P(probs), B, ws.NF, nb, st)
        if m.apply_max_norm:  # the forward hooks of the reference (:33-34, :47-48), intended meaning: one launch
            L("eav_renorm_rows2", P(m.depthwiseConv.weight), 64, m.Chans, wd, nb, ws.NF, m.norm_rate, st)
        return probs

    # ------------------------------------------------------------------ backward
    def backward(self, dprobs):
        m, s = self.m, self.m._saved
        self.st = _lib.stream_ptr()
        xp, xidx, B = self.input_view(s.x)
        g = m._grad_views()
        conv_fft = self.use_conv_fft(B)
        fuse = bool(m.conv_fuse) and conv_fft
        self.head_backward(s, g, B, dprobs)
        self.block2_tail_backward(s, g, B, fuse)
        self.separable_backward(s, g, B, conv_fft, fuse)
        self.depthwise_backward(s, g, B)
        self.fir_wgrad(s, g, xp, xidx, B)
        return m._grads_out(g)

    def head_backward(self, s, g, B, dprobs):
        m, ws, P = self.m, s.ws, _lib.ptr
        _lib.call("eav_dense_softmax_bwd", P(dprobs), P(s.probs), P(ws.p3), P(m.dense.weight), P(g["dense.weight"]),
                  P(g["dense.bias"]), P(ws.dp3), B, ws.NF, m.nb_classes, self.st)

    def block2_tail_backward(self, s, g, B, fuse):
        """Dropout <- AvgPool8 <- ELU <- separableBN: ws.dp3 -> ws.du3 (left to the fused separableConv backward of a
        training step: `fuse`) and separableBN's gradients."""
        m, ws, L, P, st = self.m, s.ws, _lib.call, _lib.ptr, self.st
        gw, gb = g["separableBN.weight"], g["separableBN.bias"]
        if s.training:
            m._bn_elu_pool_bwd(ws.dp3, ws.u3, None if fuse else ws.du3, ws.bn3, ws.part_pb, gw, gb, B, 64, ws.T2, 8, s.drop2,
                               s.training)
        else:
            # eval-mode step (Q4: every epoch after the first): BatchNorm backward is a plain scale, so the gradient and the
            # sums for the BatchNorm weight / bias leave from ONE pass over u3 / dp3
            L("eav_bn_elu_pool_bwd_eval", P(ws.dp3), P(ws.u3), P(ws.bn3), P(ws.du3), P(ws.part_pb), B, 64, ws.T2, 8,
              *s.drop2, st)
            L("eav_bn_bwd_finalize", P(ws.part_pb), B, 64, float(B * ws.T2), int(s.training), P(gw), P(gb),
              bn_field(ws.bn3, 64, BN_M1), bn_field(ws.bn3, 64, BN_M2), st)

    def separable_backward(self, s, g, B, conv_fft, fuse):
        """separableConv: data gradient (flipped / transposed taps, pad 8) -> ws.dp2, and weight gradient."""
        m, ws, L, P, st = self.m, s.ws, _lib.call, _lib.ptr, self.st
        T2, gw3 = ws.T2, P(g["separableConv.weight"])
        if fuse:
            # one pack launch for both (the filter spectra of the data gradient were prepared by this step's forward call);
            # training step: du3 = the apply pass that _bn_elu_pool_bwd left out is formed inside it and never written
            L("eav_conv64_fft_bwd", None if s.training else P(ws.du3), P(ws.dp3), P(ws.u3), P(ws.bn3),
              bn_field(ws.bn3, 64, BN_M1), *s.drop2, P(ws.dp2), gw3, P(ws.c64_ws), B, T2, st)
        elif conv_fft:
            # (bwd = 2: the filter spectra of the data gradient were prepared by this step's forward call)
            L("eav_conv64_fft_fwd", P(ws.du3), P(m.separableConv.weight), P(ws.dp2), None, P(ws.c64_ws), B, T2, 2, st)
            L("eav_conv64_fft_wgrad", P(ws.du3), gw3, P(ws.c64_ws), B, T2, st)
        else:
            L("eav_conv64_fwd", P(ws.du3), P(ws.wTb), P(ws.dp2), None, B, T2, 8, st)
            L("eav_conv64_wgrad", P(ws.du3), P(ws.p2), P(ws.part_cw), B, T2, 7, st)
            L("eav_reduce_partials", P(ws.part_cw), ws.np_cw, 65536, 65536, 1.0, gw3, st)

    def depthwise_backward(self, s, g, B):
        """Dropout <- AvgPool4 <- ELU <- depthwiseBN <- depthwiseConv <- ELU <- firstBN (post-renorm depthwise weight, Q2):
        ws.dp2 -> ws.g1; dz is formed inside the depthwise pass, no dz tensor in HBM.  Then the finishing launch."""
        m, ws, L, P, st = self.m, s.ws, _lib.call, _lib.ptr, self.st
        C, S, tr, w2 = m.Chans, m.Samples, int(s.training), P(m.depthwiseConv.weight)
        b1, b2, nparts = P(ws.bn1), P(ws.bn2), B * ws.nchunk
        gw, gb = g["depthwiseBN.weight"], g["depthwiseBN.bias"]
        if s.training:
            m._bn_elu_pool_bwd(ws.dp2, ws.z, None, ws.bn2, ws.part_pb, gw, gb, B, 64, S, 4, s.drop1, s.training)
            L("eav_eegnet_dw_bwd_fused", P(ws.y1), P(ws.z), P(ws.dp2), b2, b1, w2, P(ws.g1), P(ws.part_dst),
              P(ws.part_dw2), B, C, S, *s.drop1, st)
            bn2job = BnBwdJob()
        else:
            # eval-mode step: no sums are needed before dz = scale2 g - they leave from the depthwise pass itself (no reduce
            # launch, no extra read of z and dp2)
            L("eav_eegnet_dw_bwd_fused_eval", P(ws.y1), P(ws.z), P(ws.dp2), b2, b1, w2, P(ws.g1), P(ws.part_dst),
              P(ws.part_dw2), P(ws.part_dw), B, C, S, *s.drop1, st)
            bn2job = BnBwdJob(P(ws.part_dw), nparts, 64, float(B * S), tr, P(gw), P(gb), bn_field(ws.bn2, 64, BN_M1),
                              bn_field(ws.bn2, 64, BN_M2))
        # the finishing work behind the depthwise pass in ONE launch: depthwiseConv.weight (fixed-order sum of the partial
        # rows), firstBN's backward sums -> its gradients and the m1 / m2 the FIR weight gradient folds in, and - eval-mode
        # step - depthwiseBN's, which left from the same pass
        bn1job = BnBwdJob(P(ws.part_dst), nparts, 8, float(B * C * S), tr, P(g["firstBN.weight"]), P(g["firstBN.bias"]),
                          bn_field(ws.bn1, 8, BN_M1), bn_field(ws.bn1, 8, BN_M2))
        L("eav_reduce_and_bn_bwd_finalize", P(ws.part_dw2), nparts, 64 * C, 64 * C, P(g["depthwiseConv.weight"]), *bn1job,
          *bn2job, st)

    def fir_wgrad(self, s, g, xp, xidx, B):
        """firstConv weight gradient (firstBN's backward folded into the operand staging)."""
        m, ws, L, P, st = self.m, s.ws, _lib.call, _lib.ptr, self.st
        C, S, K, gw1 = m.Chans, m.Samples, m.kernLength, P(g["firstConv.weight"])
        # eval-mode step (every epoch after the first, Q4): BatchNorm backward is a plain scale, y1 is not needed
        y1 = P(ws.y1) if s.training else None
        if self.use_fft():
            if ws.fft_ws is None:       # (the table form's size: the other one + K K + K doubles)
                ws.fft_ws = torch.empty(_lib.plain("eav_eegnet_fir_wgrad_fft_xtab_ws_floats", B, C, S, K), dtype=torch.float32,
                                        device=ws.y1.device)
            xtab = getattr(s.x, "xtab", None) if s.training else None
            if xtab is not None:
                # a GraphStep batch of a data set with InputTables: y1's share of dW comes from them, in the same three
                # launches - y1 (614 MB at the bench shape) is not read.  Agrees with the other branch to rounding.
                L("eav_eegnet_fir_wgrad_fft_xtab", xp, xidx, P(xtab.tab), P(m.firstConv.weight), P(ws.g1), P(ws.bn1),
                  P(ws.fft_ws), gw1, B, C, S, K, st)
            else:
                L("eav_eegnet_fir_wgrad_fft", xp, xidx, y1, P(ws.g1), P(ws.bn1), P(ws.fft_ws), gw1, B, C, S, K, st)
        else:
            if xidx is None:
                L("eav_eegnet_fir_wgrad", xp, y1, P(ws.g1), P(ws.bn1), P(ws.part_fw), B, C, S, K, st)
            else:
                L("eav_eegnet_fir_wgrad_indexed", xp, xidx, y1, P(ws.g1), P(ws.bn1), P(ws.part_fw), B, C, S, K, st)
            L("eav_reduce_partials", P(ws.part_fw), ws.np_fw, 8 * K, 8 * K, 1.0, gw1, st)


# ----------------------------------------------------------------------------- generic widths (csrc/eegnet_canon.hip)
class _GenericWorkspace(eegnet_canon.Workspace):
    """Device buffers of the run-time-parametrised path: eegnet_canon.Workspace + block 2 (the dense "separableConv" output
    u3, pooled p3)."""

    def __init__(self, m, B, dev):
        super().__init__(m, B, dev)
        f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)  # noqa: E731
        C2, F2, T2 = m.F1 * m.D, m.F2, self.T2
        self.u3, self.du3 = f(B, F2, T2), f(B, F2, T2)
        self.p3, self.dp3 = f(B, self.NF), f(B, self.NF)
        self.np_c = _lib.plain("eav_dconv_fwd_nparts", B, T2)
        self.part_c = f(self.np_c, 2 * F2)
        self.part_cw = f(B, F2 * C2 * 16)


class GenericPath(_Path):
    """EEGNet_tor.forward (:50-67) for any F1 / D / F2 / kernLength / Chans the reference constructor accepts, on the
    run-time-parametrised kernels: eav_tconv_* (firstConv), eav_spatial_* with the ELU flag (firstBN -> ELU ->
    depthwiseConv), eav_dconv_* (the dense "separableConv"), the shared BN -> ELU -> pool -> dropout and classifier
    kernels.  Same quirks as the specialised path: max-norm after the forward (Q1/Q2), softmax output (Q3)."""

    def use_fft(self):
        return False

    def step_begin_args(self, optimizer, ys, idx, targets):
        return None         # no counter launch that could carry them: forward_batch gathers the labels itself

    def forward(self, x):
        m, L, P, st = self.m, _lib.call, _lib.ptr, _lib.stream_ptr()
        xp, xidx, B = self.input_view(x)
        if xidx is not None:        # the eav_tconv kernels take no index vector
            data, x = x.data, torch.empty(x.shape, dtype=torch.float32, device=x.device)
            L("eav_gather_rows", xp, xidx, P(x), B, data[0].numel(), st)
        C, nb, C2, F2 = m.Chans, m.nb_classes, m.F1 * m.D, m.F2
        ws = m._workspace(("generic", B, C, m.Samples, str(x.device)), lambda: _GenericWorkspace(m, B, x.device))
        training = bool(m.training)
        w1, _, _, w2, _, _, w3, _, _, wd, bd = m._params()
        m._token += 1
        cnt, drop1, drop2, mk = self.dropout_args(x.device, training)
        if cnt is not None or training:
            L("eav_counter_inc4", *self.counters(cnt, training), st)
        eegnet_canon.block1_forward(m, ws, x, w1, m.firstBN, w2, m.depthwiseBN, 1, training, drop1)     # :51-58
        L("eav_dconv_fwd", P(ws.a2), P(w3), P(ws.u3), P(ws.part_c), B, C2, F2, ws.T2, 16, 0, st)        # :59
        m._bn_finalize(m.separableBN, ws.part_c, ws.np_c, B * ws.T2, ws.bn3, training)                  # :60
        L("eav_bn_elu_pool_fwd", P(ws.u3), P(ws.bn3), P(ws.p3), B, F2, ws.T2, 8, *drop2, st)            # :61-63
        probs = torch.empty(B, nb, dtype=torch.float32, device=x.device)
        L("eav_dense_softmax_fwd", P(ws.p3), P(wd), P(bd), None, P(probs), B, ws.NF, nb, st)            # :64-66
        if m.apply_max_norm:
            L("eav_renorm_rows", P(w2), C2, C, m.norm_rate, st)
            L("eav_renorm_rows", P(wd), nb, ws.NF, m.norm_rate, st)
        m._saved = Saved(m._token, x, training, drop1, drop2, mk, ws, probs)
        return m._token

    def backward(self, dprobs):
        m, s, L, P, st = self.m, self.m._saved, _lib.call, _lib.ptr, _lib.stream_ptr()
        ws = s.ws
        B, nb, C2, F2, T2 = s.x.shape[0], m.nb_classes, m.F1 * m.D, m.F2, ws.T2
        g = m._grad_views()
        w2, w3, wd = m.depthwiseConv.weight, m.separableConv.weight, m.dense.weight
        L("eav_dense_softmax_bwd", P(dprobs), P(s.probs), P(ws.p3), P(wd), P(g["dense.weight"]), P(g["dense.bias"]),
          P(ws.dp3), B, ws.NF, nb, st)
        m._bn_elu_pool_bwd(ws.dp3, ws.u3, ws.du3, ws.bn3, ws.part_pb, g["separableBN.weight"], g["separableBN.bias"],
                           B, F2, T2, 8, s.drop2, s.training)
        # the dense temporal conv: data gradient = the same kernel on the transposed, tap-flipped weights
        L("eav_dconv_fwd", P(ws.du3), P(w3), P(ws.da2), None, B, F2, C2, T2, 16, 1, st)
        L("eav_dconv_wgrad", P(ws.du3), P(ws.a2), P(ws.part_cw), B, C2, F2, T2, 16, st)
        n3 = F2 * C2 * 16
        L("eav_reduce_partials", P(ws.part_cw), B, n3, n3, 1.0, P(g["separableConv.weight"]), st)
        # block 1 (post-renorm depthwise weight, Q2)
        eegnet_canon.block1_backward(m, ws, s.x, w2, [g[k] for k in _PARAM_ORDER[:6]], 1, s.training, s.drop1)
        return m._grads_out(g)
