"""EEGNet_tor + Trainer_uni on MI355X: the reference's class API over libeav_hip.so.

Mirrors CNN_torch/EEGNet_tor.py one-for-one at the Python boundary:

    EEGNet_tor(nb_classes, Chans=30, Samples=500, dropoutRate=0.5, kernLength=300,
               F1=8, D=8, F2=64, norm_rate=1.0, dropoutType='Dropout')      (:16-17)
        __call__(x[B,1,Chans,Samples]) -> softmax probabilities [B,nb_classes]   (:50-67)
    Trainer_uni(model, data, lr=1e-4, batch_size=32, num_epochs=10, device=None) (:70)
        .train() / .validate()                                                   (:96,:118)

The module owns the same sub-modules, so ``state_dict()`` keys and the default
initialisation stream (torch RNG) are those of the reference; the arithmetic of
forward and backward is entirely in hand-written gfx950 kernels (eav_amd/csrc).
Reference behaviour kept on purpose: max-norm renorm after the
forward and before the backward (Q1/Q2), softmax output fed to CrossEntropyLoss
(Q3), ``model.train()`` called once so that epochs >= 2 train in eval mode (Q4).

There is no CPU path: calling the model with a non-device tensor raises.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from . import _lib, eegnet_canon
from .optim import CrossEntropyLoss, FusedAdam
# re-exported: bench.py, tools/ and the tests import GraphStep, gather_batch and DeviceLoader from this module
from .runtime import (DeviceLoader, GraphStep, KernelFn, KernelModule, cached_workspace, eager_step,  # noqa: F401
                      gather_batch, train_step)

_PARAM_ORDER = [
    "firstConv.weight", "firstBN.weight", "firstBN.bias",
    "depthwiseConv.weight", "depthwiseBN.weight", "depthwiseBN.bias",
    "separableConv.weight", "separableBN.weight", "separableBN.bias",
    "dense.weight", "dense.bias",
]


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


class _GenericWorkspace(eegnet_canon.Workspace):
    """Device buffers of the run-time-parametrised path (EEGNet_tor._generic): eegnet_canon.Workspace + block 2 (the dense
    "separableConv" output u3, pooled p3)."""

    def __init__(self, m, B, dev):
        super().__init__(m, B, dev)
        f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)  # noqa: E731
        C2, F2, T2 = m.F1 * m.D, m.F2, self.T2
        self.u3, self.du3 = f(B, F2, T2), f(B, F2, T2)
        self.p3, self.dp3 = f(B, self.NF), f(B, self.NF)
        self.np_c = _lib.plain("eav_dconv_fwd_nparts", B, T2)
        self.part_c = f(self.np_c, 2 * F2)
        self.part_cw = f(B, F2 * C2 * 16)


class IndexedBatch:
    """A batch addressed in place: samples `idx` (device int64 [B]) of an HBM-resident data set `data` [N,1,C,S].  The FIR
    kernels - the only readers of the network input - take the index vector, so no gathered copy of the batch is made."""

    def __init__(self, data, idx):
        self.data, self.idx = data, idx
        self.shape = (idx.numel(),) + tuple(data.shape[1:])
        self.device = data.device


class _EEGNetFn(KernelFn):
    @staticmethod
    def forward(ctx, x, model, *params):
        # EEGNet_tor._forward_output: the probabilities tensor this forward wrote, no copy kernel.  (A detached alias, not
        # the saved object itself: returning the very tensor that the model also keeps for its backward crashes hipGraph
        # capture in torch 2.10.)  The alias shares its version counter with the saved tensor: an in-place edit of the
        # returned scores before backward (clamp_, += eps ...) would silently corrupt dense_softmax_bwd's input - checked
        # in backward.
        out = KernelFn.forward(ctx, x, model, *params)
        ctx.probs_version = model._saved[-1]._version
        return out

    @staticmethod
    def backward(ctx, dprobs):
        saved = ctx.model._saved
        if saved is not None and saved[0] == ctx.token and saved[-1]._version != ctx.probs_version:
            raise _lib.EavError("EEGNet_tor: the scores returned by forward() were modified in place before backward(); "
                                "they alias the probabilities the backward reads - clone() them first")
        return KernelFn.backward(ctx, dprobs)


class EEGNet_tor(KernelModule):
    _PARAM_ORDER = _PARAM_ORDER

    def __init__(self, nb_classes, Chans=30, Samples=500, dropoutRate=0.5, kernLength=300, F1=8, D=8, F2=64,
                 norm_rate=1.0, dropoutType='Dropout'):
        super().__init__()
        # The reference configuration (F1=8, D=8, F2=64, kernLength<=300, Chans<=32: EEGNet_tor.py:159) runs the specialised
        # fp32-MFMA kernels; every other width the reference constructor accepts (:16-17) takes the run-time-parametrised
        # kernels of csrc/eegnet_canon.hip (`_generic`), whose LDS tiles bound it at the sizes below.
        self._generic = not (F1 == 8 and D == 8 and F2 == 64 and 1 <= kernLength <= 300 and 1 <= Chans <= 32)
        if not (1 <= F1 <= 16 and 1 <= D <= 8 and F1 * D <= 64 and 1 <= F2 <= 64 and 1 <= kernLength <= 1024
                and 1 <= Chans <= 256 and 1 <= nb_classes <= 16 and Samples >= 32):
            raise NotImplementedError("eav_amd.EEGNet_tor: the gfx950 kernels cover F1<=16, D<=8, F1*D<=64, F2<=64, "
                                      "kernLength<=1024, Chans<=256, nb_classes<=16, Samples>=32")
        # same sub-modules in the same construction order as the reference (:21-48): identical
        # state_dict keys and identical consumption of the torch RNG by the default initialisers
        self.dropout = nn.Dropout(dropoutRate) if dropoutType == 'Dropout' else nn.Dropout2d(dropoutRate)
        self.firstConv = nn.Conv2d(1, F1, (1, kernLength), padding='same', bias=False)
        self.firstBN = nn.BatchNorm2d(F1)
        self.elu = nn.ELU()
        self.depthwiseConv = nn.Conv2d(F1, F1 * D, (Chans, 1), groups=F1, padding=0, bias=False)
        self.depthwiseBN = nn.BatchNorm2d(F1 * D)
        self.depthwisePool = nn.AvgPool2d((1, 4))
        self.separableConv = nn.Conv2d(F1 * D, F2, (1, 16), padding='same', bias=False)
        self.separableBN = nn.BatchNorm2d(F2)
        self.separablePool = nn.AvgPool2d((1, 8))
        self.flatten = nn.Flatten()
        self.dense = nn.Linear(F2 * (Samples // 4 // 8), nb_classes)
        self.softmax = nn.Softmax(dim=1)

        self.nb_classes, self.Chans, self.Samples, self.kernLength = nb_classes, Chans, Samples, kernLength
        self.F1, self.D, self.F2 = F1, D, F2
        self.norm_rate, self.dropoutRate = float(norm_rate), float(dropoutRate)
        # any other dropoutType is nn.Dropout2d in the reference (:21): one keep decision per (sample, channel) map - the
        # kernels take it as a negative probability (eav_hip.h)
        self.spatial_dropout = dropoutType != 'Dropout'
        self.dropout_seed = 0x0EA5EED          # base seed of the counter-based dropout generator
        # (set_dropout_masks, tests: (mask1 uint8 [B,64,S/4], mask2 uint8 [B,64,S/32]))
        self.apply_max_norm = True
        # (the round-2 "split" mode - FIR / separableConv products on the fp16 matrix cores with two-piece operands - was
        # retired in round 5: with the FFT FIR and the frequency-domain separableConv it was the slower path)
        self.fir_precision = "fp32"
        # How the exact-fp32 firstConv and its weight gradient are evaluated.  "fft": overlap-save blocks of 1024-point
        # FFTs (csrc/eegnet_fir_fft.hip: ~350 flops per output sample for the 8 filters together instead of 4800 - the two
        # kernels become HBM-bound); "mfma": the Toeplitz GEMMs on the fp32 matrix cores (csrc/eegnet_fir.hip); "auto"
        # (default): FFT for recordings of at least two 704-sample blocks and kernels of <= 321 taps, MFMA for short epochs
        # (the reference's own [B,1,30,500], where one FFT block would be mostly padding).  EAV_FIR_ALGO overrides.
        self.fir_algo = os.environ.get("EAV_FIR_ALGO", "auto")
        self.conv_algo = os.environ.get("EAV_CONV_ALGO", "auto")      # separableConv: see _use_conv_fft
        # frequency-domain separableConv backward from ONE pack launch that writes the spectra of both gradients and - in a
        # training step - forms du3 from dp3 / u3 while it loads (eav_conv64_fft_bwd: no eav_bn_elu_pool_bwd_apply launch, no
        # du3 tensor, one pack launch less); False / EAV_CONV_FUSE=0: the separate launches (bit-identical results)
        self.conv_fuse = os.environ.get("EAV_CONV_FUSE", "1") != "0"
        self._infer = False                    # set per call: no-grad eval-mode forward
        # forward_batch: (optimiser step counter, labels, idx, targets, batch) - raw pointers for eav_step_begin, taken by the next
        # forward's counter launch (left in place if that forward has none to merge them into)
        self._step_begin = None
        # validate()'s forward with block 1 as ONE kernel (eav_eegnet_block1_infer: y1 / z never written).  Opt-in: at the
        # benchmark shape [64,1,30,10000] it measures 1.35 ms against 1.30 ms for the training kernels in eval mode - with its
        # 128 z accumulators per lane it runs one wave per SIMD and cannot hide its VALU tail behind another wave's MFMAs
        self.fused_eval = False

    # ------------------------------------------------------------------ plumbing
    def _use_fft(self):
        if self.fir_algo not in ("auto", "fft", "mfma"):
            raise ValueError(f"fir_algo {self.fir_algo!r}: expected 'auto', 'fft' or 'mfma'")
        if self.fir_algo == "mfma" or self.kernLength > _lib.plain("eav_eegnet_fir_fft_max_taps"):
            return False
        return self.fir_algo == "fft" or self.Samples >= 1408

    def _use_conv_fft(self, B):
        """separableConv (forward, data and weight gradient) in the frequency domain (csrc/eegnet_conv64_fft.hip: per-bin
        [128 x 128] GEMMs instead of a 1024-deep contraction, 6x fewer multiply-adds) when the batch is large enough to
        amortise its extra launches; the direct fp32-MFMA kernels otherwise (the reference's own [32,1,30,500]).
        `conv_algo` / EAV_CONV_ALGO: "auto" (default), "fft", "mfma"."""
        if self.conv_algo not in ("auto", "fft", "mfma"):
            raise ValueError(f"conv_algo {self.conv_algo!r}: expected 'auto', 'fft' or 'mfma'")
        if self.conv_algo == "mfma":
            return False
        return self.conv_algo == "fft" or B * (self.Samples // 4) >= 40000

    def forward(self, x):
        self._require_gpu(x)
        if x.dim() == 3:
            x = x.unsqueeze(1)
        if x.dim() != 4 or x.shape[1] != 1 or x.shape[2] != self.Chans or x.shape[3] != self.Samples:
            raise ValueError(f"expected input [B,1,{self.Chans},{self.Samples}], got {tuple(x.shape)}")
        self._require_same_device(x)
        x = x.contiguous().float()
        self._ensure_flat()
        # no-grad evaluation (validate(), EEGNet_tor.py:118-135): block 1 runs as one fused kernel, see _launch_forward
        self._infer = (not torch.is_grad_enabled()) and (not self.training)
        return _EEGNetFn.apply(x, self, *self._params())

    def forward_indexed(self, data, idx):
        """forward(data[idx]) without materialising data[idx] (Trainer_uni's per-step batch assembly,
        EEGNet_tor.py:100-101): `data` [N,1,Chans,Samples] fp32 contiguous on the device, `idx` device int64 [B]."""
        if data.dim() != 4 or data.shape[1] != 1 or data.shape[2] != self.Chans or data.shape[3] != self.Samples or \
                not data.is_cuda or data.dtype != torch.float32 or not data.is_contiguous():
            raise ValueError(f"expected a contiguous fp32 device array [N,1,{self.Chans},{self.Samples}]")
        if idx.dtype != torch.int64 or idx.device != data.device or idx.dim() != 1:
            raise ValueError("idx must be a 1-D int64 tensor on the data's device")
        if self._generic:
            out = torch.empty((idx.numel(),) + tuple(data.shape[1:]), dtype=torch.float32, device=data.device)
            _lib.call("eav_gather_rows", data.data_ptr(), idx.data_ptr(), out.data_ptr(), idx.numel(), data[0].numel(),
                      _lib.stream_ptr())
            return self.forward(out)
        self._require_same_device(data)
        self._ensure_flat()
        self._infer = (not torch.is_grad_enabled()) and (not self.training)
        return _EEGNetFn.apply(IndexedBatch(data, idx), self, *self._params())

    # ------------------------------------------------------------------ kernels
    def _forward_output(self):
        return self._saved[-1].detach()          # see _EEGNetFn

    def forward_batch(self, xs, ys, idx, optimizer):
        """GraphStep's batch: read in place through the index vector (forward_indexed); only the labels are gathered - by
        the model's own step-counter launch where it has one (eav_step_begin: the label gather, the optimiser's step
        count and the dropout / BatchNorm counters in ONE graph node instead of three)."""
        if not (xs.is_cuda and xs.dim() == 4 and xs.is_contiguous()):
            return super().forward_batch(xs, ys, idx, optimizer)
        batch = idx.numel()
        targets = torch.empty(batch, dtype=torch.long, device=xs.device)
        optimizer.step_counted = False       # (a step that failed between its two halves must not leave the flag set)
        if not self._generic:
            # raw pointers for eav_step_begin, taken by the forward's counter launch (left in place if that forward has
            # none to merge them into); FusedAdam.step() then skips its own eav_counter_inc for this one step
            cnt = optimizer.device_step_counter()
            self._step_begin = (cnt.data_ptr(), ys.data_ptr(), idx.data_ptr(), targets.data_ptr(), batch)
        scores = self.forward_indexed(xs, idx)
        merged = not self._generic and self._step_begin is None        # taken: eav_step_begin ran
        self._step_begin = None
        optimizer.step_counted = merged
        if not merged:
            _lib.call("eav_gather_i64", ys.data_ptr(), idx.data_ptr(), targets.data_ptr(), batch, _lib.stream_ptr())
        return scores, targets

    def _dropout_args(self, dev, training):
        """(counter pointer, block-1 and block-2 dropout arguments (rate, seed, mask pointer, counter pointer), mk)."""
        drop = self.dropoutRate if training else 0.0
        if self.spatial_dropout:
            drop = -drop
        # dropout stream: effective seed = base + 2 * (device-resident count of training forwards) - no host
        # argument changes from step to step, so the whole step can be replayed from a hipGraph
        cnt, mk = self._dropout(dev, drop != 0.0)
        return cnt, (drop, self.dropout_seed, mk(0), cnt), (drop, self.dropout_seed + 1, mk(1), cnt), mk

    def _launch_forward(self, x):
        if self._generic:
            return self._launch_forward_generic(x)
        L, P, st = _lib.call, _lib.ptr, _lib.stream_ptr()
        B, C, S, K, nb = x.shape[0], self.Chans, self.Samples, self.kernLength, self.nb_classes
        ws = self._workspace((B, C, S, str(x.device)), lambda: _Workspace(B, C, S, K, nb, x.device))
        training = bool(self.training)
        w1, _, _, w2, _, _, w3, _, _, wd, bd = [P(p) for p in self._params()]
        bn1, bn2, bn3 = self.firstBN, self.depthwiseBN, self.separableBN
        bnfin = self._bn_finalize
        self._token += 1
        cnt, drop1, drop2, mk = self._dropout_args(x.device, training)
        drop, m1 = drop1[0], drop1[2]
        if self.fir_precision != "fp32":
            raise ValueError(f"fir_precision {self.fir_precision!r}: only 'fp32' exists (the split mode was retired)")
        counters = [cnt] + ([P(bn.num_batches_tracked) for bn in (bn1, bn2, bn3)] if training else [None] * 3)
        begin, self._step_begin = self._step_begin, None
        if not self._use_conv_fft(B):    # (the frequency-domain separableConv takes the weight tensor as it is)
            # per-step prologue, one launch: the transposed separableConv weights of the direct kernels + the dropout step
            # counter and the three BatchNorm step counters (nn.BatchNorm2d's num_batches_tracked)
            L("eav_eegnet_step_prologue", w3, P(ws.wTf), P(ws.wTb), *counters, st)
            self._step_begin = begin     # (not taken: GraphStep issues its own launches)
        elif begin is not None:
            # ... and, in a captured step (GraphStep), the optimiser's step count and the gather of the batch's labels with them
            L("eav_step_begin", *counters, *begin, st)
        elif cnt is not None or training:
            # library kernels, no torch op inside a captured step
            L("eav_counter_inc4", *counters, st)
        np_fir = ws.np_fir
        infer = self.fused_eval and self._infer and not training and S % 4 == 0
        if infer:
            # validate(): x -> block-1 output in ONE kernel (FIR -> firstBN -> ELU -> depthwiseConv -> depthwiseBN -> ELU ->
            # AvgPool4; BatchNorms on running statistics): y1 (614 MB at [64,1,30,10000]) and z are never written
            bnfin(bn1, ws.part_fir, ws.np_fir, B * C * S, ws.bn1, training)       # eval mode: running statistics only
            bnfin(bn2, ws.part_dw, B * ws.nchunk, B * S, ws.bn2, training)
            if isinstance(x, IndexedBatch):
                L("eav_eegnet_block1_infer", P(x.data), P(x.idx), w1, P(ws.bn1), w2, P(ws.bn2), P(ws.p2), B, C, S, K, st)
            else:
                L("eav_eegnet_block1_infer", P(x), None, w1, P(ws.bn1), w2, P(ws.bn2), P(ws.p2), B, C, S, K, st)
        elif self._use_fft():
            np_fir = ws.np_fir_fft
            pf = P(ws.part_fir) if training else None      # eval mode: firstBN needs no batch statistics
            if isinstance(x, IndexedBatch):
                L("eav_eegnet_fir_fwd_fft", P(x.data), P(x.idx), w1, P(ws.y1), pf, B, C, S, K, st)
            else:
                L("eav_eegnet_fir_fwd_fft", P(x), None, w1, P(ws.y1), pf, B, C, S, K, st)
        else:
            if isinstance(x, IndexedBatch):
                L("eav_eegnet_fir_fwd_indexed", P(x.data), P(x.idx), w1, P(ws.y1), P(ws.part_fir), B, C, S, K, st)
            else:
                L("eav_eegnet_fir_fwd", P(x), w1, P(ws.y1), P(ws.part_fir), B, C, S, K, st)
        if not infer:
            bnfin(bn1, ws.part_fir, np_fir, B * C * S, ws.bn1, training)
            if not training and drop == 0.0 and m1 is None and S % 4 == 0:
                # eval-mode step (what 349 of the reference's 350 epochs run, Q4): depthwiseBN's scale / shift come from the
                # running statistics, i.e. they are known BEFORE the depthwise pass - which then leaves the pooled block-1
                # output too (z is still written: the backward forms dz from it); one launch and one pass over z less
                bnfin(bn2, ws.part_dw, B * ws.nchunk, B * S, ws.bn2, training)
                L("eav_eegnet_dw_fwd_pool_eval", P(ws.y1), P(ws.bn1), w2, P(ws.z), P(ws.part_dw), P(ws.bn2), P(ws.p2), B, C, S,
                  st)
            else:
                L("eav_eegnet_dw_fwd", P(ws.y1), P(ws.bn1), w2, P(ws.z), P(ws.part_dw), B, C, S, st)
                bnfin(bn2, ws.part_dw, B * ws.nchunk, B * S, ws.bn2, training)
                L("eav_bn_elu_pool_fwd", P(ws.z), P(ws.bn2), P(ws.p2), B, 64, S, 4, *drop1, st)
        np_c3 = ws.np_c3
        if self._use_conv_fft(B):
            if ws.c64_ws is None:
                ws.c64_ws = torch.zeros(_lib.plain("eav_conv64_fft_ws_floats", B, ws.T2), dtype=torch.float32,
                                        device=ws.y1.device)
            np_c3 = ws.np_c3_fft
            L("eav_conv64_fft_fwd", P(ws.p2), w3, P(ws.u3), P(ws.part_c3), P(ws.c64_ws), B, ws.T2, 0, st)
        else:
            L("eav_conv64_fwd", P(ws.p2), P(ws.wTf), P(ws.u3), P(ws.part_c3), B, ws.T2, 7, st)
        bnfin(bn3, ws.part_c3, np_c3, B * ws.T2, ws.bn3, training)
        L("eav_bn_elu_pool_fwd", P(ws.u3), P(ws.bn3), P(ws.p3), B, 64, ws.T2, 8, *drop2, st)
        probs = torch.empty(B, nb, dtype=torch.float32, device=x.device)   # fresh per forward: returned, kept for backward
        L("eav_dense_softmax_fwd", P(ws.p3), wd, bd, None, P(probs), B, ws.NF, nb, st)
        if self.apply_max_norm:  # the forward hooks of the reference (:33-34, :47-48), intended meaning: one launch
            L("eav_renorm_rows2", w2, 64, C, wd, nb, ws.NF, self.norm_rate, st)
        self._saved = (self._token, x, training, drop1, drop2, mk, ws, probs)      # (mk keeps explicit masks alive)
        return self._token

    # ------------------------------------------------------------------ generic widths (csrc/eegnet_canon.hip)
    def _launch_forward_generic(self, x):
        """EEGNet_tor.forward (:50-67) for any F1 / D / F2 / kernLength / Chans the reference constructor accepts, on the
        run-time-parametrised kernels: eav_tconv_* (firstConv), eav_spatial_* with the ELU flag (firstBN -> ELU ->
        depthwiseConv), eav_dconv_* (the dense "separableConv"), the shared BN -> ELU -> pool -> dropout and classifier
        kernels.  Same quirks as the specialised path: max-norm after the forward (Q1/Q2), softmax output (Q3)."""
        L, P, st = _lib.call, _lib.ptr, _lib.stream_ptr()
        B, C, nb, C2, F2 = x.shape[0], self.Chans, self.nb_classes, self.F1 * self.D, self.F2
        ws = self._workspace(("generic", B, C, self.Samples, str(x.device)), lambda: _GenericWorkspace(self, B, x.device))
        training = bool(self.training)
        w1, _, _, w2, _, _, w3, _, _, wd, bd = self._params()
        bn1, bn2, bn3 = self.firstBN, self.depthwiseBN, self.separableBN
        self._token += 1
        cnt, drop1, drop2, mk = self._dropout_args(x.device, training)
        if cnt is not None or training:
            L("eav_counter_inc4", cnt, *([P(bn.num_batches_tracked) for bn in (bn1, bn2, bn3)] if training else [None] * 3),
              st)
        eegnet_canon.block1_forward(self, ws, x, w1, bn1, w2, bn2, 1, training, drop1)                 # :51-58
        L("eav_dconv_fwd", P(ws.a2), P(w3), P(ws.u3), P(ws.part_c), B, C2, F2, ws.T2, 16, 0, st)        # :59
        self._bn_finalize(bn3, ws.part_c, ws.np_c, B * ws.T2, ws.bn3, training)                         # :60
        L("eav_bn_elu_pool_fwd", P(ws.u3), P(ws.bn3), P(ws.p3), B, F2, ws.T2, 8, *drop2, st)            # :61-63
        probs = torch.empty(B, nb, dtype=torch.float32, device=x.device)
        L("eav_dense_softmax_fwd", P(ws.p3), P(wd), P(bd), None, P(probs), B, ws.NF, nb, st)            # :64-66
        if self.apply_max_norm:
            L("eav_renorm_rows", P(w2), C2, C, self.norm_rate, st)
            L("eav_renorm_rows", P(wd), nb, ws.NF, self.norm_rate, st)
        self._saved = (self._token, x, training, drop1, drop2, mk, ws, probs)
        return self._token

    def _launch_backward_generic(self, dprobs):
        L, P, st = _lib.call, _lib.ptr, _lib.stream_ptr()
        _, x, training, drop1, drop2, _, ws, probs = self._saved
        B, nb, C2, F2, T2 = x.shape[0], self.nb_classes, self.F1 * self.D, self.F2, ws.T2
        g = self._grad_views()
        w2, w3, wd = self.depthwiseConv.weight, self.separableConv.weight, self.dense.weight
        L("eav_dense_softmax_bwd", P(dprobs), P(probs), P(ws.p3), P(wd), P(g["dense.weight"]), P(g["dense.bias"]),
          P(ws.dp3), B, ws.NF, nb, st)
        self._bn_elu_pool_bwd(ws.dp3, ws.u3, ws.du3, ws.bn3, ws.part_pb, g["separableBN.weight"], g["separableBN.bias"],
                              B, F2, T2, 8, drop2, training)
        # the dense temporal conv: data gradient = the same kernel on the transposed, tap-flipped weights
        L("eav_dconv_fwd", P(ws.du3), P(w3), P(ws.da2), None, B, F2, C2, T2, 16, 1, st)
        L("eav_dconv_wgrad", P(ws.du3), P(ws.a2), P(ws.part_cw), B, C2, F2, T2, 16, st)
        n3 = F2 * C2 * 16
        L("eav_reduce_partials", P(ws.part_cw), B, n3, n3, 1.0, P(g["separableConv.weight"]), st)
        # block 1 (post-renorm depthwise weight, Q2)
        eegnet_canon.block1_backward(self, ws, x, w2, [g[k] for k in _PARAM_ORDER[:6]], 1, training, drop1)
        return self._grads_out(g)

    def _launch_backward(self, dprobs, token):
        self._check_token(token)
        if self._generic:
            return self._launch_backward_generic(dprobs)
        L, P, st = _lib.call, _lib.ptr, _lib.stream_ptr()
        _, x, training, drop1, drop2, _, ws, probs = self._saved
        B, C, S, K, nb = x.shape[0], self.Chans, self.Samples, self.kernLength, self.nb_classes
        T2, NF = ws.T2, ws.NF
        g = self._grad_views()
        w2, wd = P(self.depthwiseConv.weight), P(self.dense.weight)
        tr = int(training)

        L("eav_dense_softmax_bwd", P(dprobs), P(probs), P(ws.p3), wd, P(g["dense.weight"]), P(g["dense.bias"]),
          P(ws.dp3), B, NF, nb, st)
        # block 2: Dropout <- AvgPool8 <- ELU <- separableBN
        b3 = P(ws.bn3)
        fuse = bool(self.conv_fuse) and self._use_conv_fft(B)
        if training:
            self._bn_elu_pool_bwd(ws.dp3, ws.u3, None if fuse else ws.du3, ws.bn3, ws.part_pb, g["separableBN.weight"],
                                  g["separableBN.bias"], B, 64, T2, 8, drop2, training)
        else:
            # eval-mode step (Q4: every epoch after the first): BatchNorm backward is a plain scale, so the gradient and the
            # sums for the BatchNorm weight / bias leave from ONE pass over u3 / dp3
            L("eav_bn_elu_pool_bwd_eval", P(ws.dp3), P(ws.u3), b3, P(ws.du3), P(ws.part_pb), B, 64, T2, 8, *drop2, st)
            L("eav_bn_bwd_finalize", P(ws.part_pb), B, 64, float(B * T2), tr, P(g["separableBN.weight"]),
              P(g["separableBN.bias"]), b3 + 4 * 256, b3 + 4 * 320, st)
        # separableConv: data gradient (flipped/transposed taps, pad 8) and weight gradient
        if fuse:
            # one pack launch for both (the filter spectra of the data gradient were prepared by this step's forward call);
            # training step: du3 = the apply pass that _bn_elu_pool_bwd left out is formed inside it and never written
            L("eav_conv64_fft_bwd", None if training else P(ws.du3), P(ws.dp3), P(ws.u3), b3, b3 + 4 * 256, *drop2,
              P(ws.dp2), P(g["separableConv.weight"]), P(ws.c64_ws), B, T2, st)
        elif self._use_conv_fft(B):
            # (bwd = 2: the filter spectra of the data gradient were prepared by this step's forward call)
            L("eav_conv64_fft_fwd", P(ws.du3), P(self.separableConv.weight), P(ws.dp2), None, P(ws.c64_ws), B, T2, 2, st)
            L("eav_conv64_fft_wgrad", P(ws.du3), P(g["separableConv.weight"]), P(ws.c64_ws), B, T2, st)
        else:
            L("eav_conv64_fwd", P(ws.du3), P(ws.wTb), P(ws.dp2), None, B, T2, 8, st)
            L("eav_conv64_wgrad", P(ws.du3), P(ws.p2), P(ws.part_cw), B, T2, 7, st)
            L("eav_reduce_partials", P(ws.part_cw), ws.np_cw, 65536, 65536, 1.0, P(g["separableConv.weight"]), st)
        # block 1 tail: Dropout <- AvgPool4 <- ELU <- depthwiseBN
        b2 = P(ws.bn2)
        # depthwiseConv <- ELU <- firstBN (uses the post-renorm depthwise weight, Q2)
        b1 = P(ws.bn1)
        # dz = backward of BN2 -> ELU -> pool -> dropout is formed inside dw_bwd: no dz tensor in HBM
        if training:
            self._bn_elu_pool_bwd(ws.dp2, ws.z, None, ws.bn2, ws.part_pb, g["depthwiseBN.weight"], g["depthwiseBN.bias"],
                                  B, 64, S, 4, drop1, training)
            L("eav_eegnet_dw_bwd_fused", P(ws.y1), P(ws.z), P(ws.dp2), b2, b1, w2, P(ws.g1), P(ws.part_dst),
              P(ws.part_dw2), B, C, S, *drop1, st)
        else:
            # eval-mode step: no sums are needed before dz = scale2 g - they leave from the depthwise pass itself (no reduce
            # launch, no extra read of z and dp2)
            L("eav_eegnet_dw_bwd_fused_eval", P(ws.y1), P(ws.z), P(ws.dp2), b2, b1, w2, P(ws.g1), P(ws.part_dst),
              P(ws.part_dw2), P(ws.part_dw), B, C, S, *drop1, st)
        # the finishing work behind the depthwise pass in ONE launch: depthwiseConv.weight (fixed-order sum of the partial
        # rows), firstBN's backward sums -> its gradients and the m1 / m2 the FIR weight gradient folds in, and - eval-mode
        # step - depthwiseBN's, which left from the same pass
        bn2job = (None, 0, 0, 0.0, 0, None, None, None, None) if training else \
            (P(ws.part_dw), B * ws.nchunk, 64, float(B * S), tr, P(g["depthwiseBN.weight"]), P(g["depthwiseBN.bias"]),
             b2 + 4 * 256, b2 + 4 * 320)
        L("eav_reduce_and_bn_bwd_finalize", P(ws.part_dw2), B * ws.nchunk, 64 * C, 64 * C, P(g["depthwiseConv.weight"]),
          P(ws.part_dst), B * ws.nchunk, 8, float(B * C * S), tr, P(g["firstBN.weight"]), P(g["firstBN.bias"]), b1 + 4 * 32,
          b1 + 4 * 40, *bn2job, st)
        # firstConv weight gradient (BN backward folded into the operand staging)
        if self._use_fft():
            if ws.fft_ws is None:
                ws.fft_ws = torch.empty(_lib.plain("eav_eegnet_fir_wgrad_fft_ws_floats", B, C, S), dtype=torch.float32,
                                        device=ws.y1.device)
            xi = isinstance(x, IndexedBatch)
            L("eav_eegnet_fir_wgrad_fft", P(x.data) if xi else P(x), P(x.idx) if xi else None,
              P(ws.y1) if training else None, P(ws.g1), b1, P(ws.fft_ws), P(g["firstConv.weight"]), B, C, S, K, st)
        else:
            # eval-mode training (every epoch after the first, Q4): BatchNorm backward is a plain scale, y1 is not needed
            if isinstance(x, IndexedBatch):
                L("eav_eegnet_fir_wgrad_indexed", P(x.data), P(x.idx), P(ws.y1) if training else None, P(ws.g1), b1,
                  P(ws.part_fw), B, C, S, K, st)
            else:
                L("eav_eegnet_fir_wgrad", P(x), P(ws.y1) if training else None, P(ws.g1), b1, P(ws.part_fw), B, C, S, K,
                  st)
            L("eav_reduce_partials", P(ws.part_fw), ws.np_fw, 8 * K, 8 * K, 1.0, P(g["firstConv.weight"]), st)
        return self._grads_out(g)


class Trainer_uni:
    def __init__(self, model, data, lr=1e-4, batch_size=32, num_epochs=10, device=None):
        self.lr = lr
        self.batch_size = batch_size
        self.num_epochs = num_epochs
        self.device = device if device else torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.device = torch.device(self.device)
        if self.device.type != "cuda":
            raise _lib.EavError("eav_amd.Trainer_uni needs an MI355X (torch device 'cuda' on ROCm); no CPU fallback")
        self.tr_x, self.tr_y, self.te_x, self.te_y = data
        self.train_dataloader = self._prepare_dataloader(self.tr_x, self.tr_y, shuffle=True)
        self.test_dataloader = self._prepare_dataloader(self.te_x, self.te_y, shuffle=False)

        self.model = model
        self.criterion = CrossEntropyLoss()                       # EEGNet_tor.py:81
        self.optimizer = FusedAdam(self.model.parameters(), lr=self.lr, capturable=True)   # :82 (Adam, wd 0)
        # :86-88 wraps in nn.DataParallel when several GPUs are visible; here multi-GPU is one
        # process per GPU with an RCCL gradient all-reduce (eav_amd.dist), enabled by the launcher.
        self.model.to(self.device)
        self.grad_sync = None  # set by eav_amd.dist.attach(trainer) under torchrun
        self.use_graph = True  # replay full-size batches from a hipGraph (partial batches run eagerly)
        self._graphs = {}

    def _prepare_dataloader(self, x, y, shuffle=False):
        return DeviceLoader(x, y, self.batch_size, shuffle, self.device)

    def train(self):
        self.model.train()  # once, before the epoch loop - as the reference (:97)
        dl = self.train_dataloader
        for epoch in range(self.num_epochs):
            for batch_idx, idx in enumerate(dl.index_batches()):
                # one captured graph per (batch size, BN mode): epochs >= 2 train in eval mode (Q4)
                scores, loss, _ = train_step(self._graphs, self.model, self.optimizer, self.criterion, dl, idx,
                                             self.use_graph, self.grad_sync)
                if batch_idx % 100 == 0:
                    print(f"Epoch [{epoch+1}/{self.num_epochs}], Step [{batch_idx}/{len(self.train_dataloader)}], "
                          f"Loss: {loss.item():.4f}")
            self.criterion.check()        # out-of-range labels recorded by the captured steps of this epoch
            if self.test_dataloader:
                self.validate()

    def validate(self):
        self.model.eval()
        # EEGNet_tor.py:118-135 reads loss.item() and the hit count back after every batch; here both stay on the device
        # (one slot per batch, one hit counter) and are read once - the sums are formed in the reference's order
        nb = len(self.test_dataloader)
        losses = torch.zeros(max(nb, 1), dtype=torch.float32, device=self.device)
        correct = torch.zeros((), dtype=torch.int32, device=self.device)
        with torch.no_grad():
            for k, (data, targets) in enumerate(self.test_dataloader):
                scores = self.model(data)
                self.criterion.accumulate(scores, targets, losses[k], correct)
        total_loss = 0
        for v in losses[:nb].cpu().tolist():
            total_loss += v
        total_correct = int(correct.item())
        self.criterion.check()
        avg_loss = total_loss / len(self.test_dataloader)
        accuracy = total_correct / len(self.test_dataloader.dataset)
        print(f"Validation - Loss: {avg_loss:.4f}, Accuracy: {accuracy:.4f}")
