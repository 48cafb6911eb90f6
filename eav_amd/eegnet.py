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

from . import _lib
from .criteria import CrossEntropyLoss
from .eegnet_paths import _PARAM_ORDER, FastPath, GenericPath, IndexedBatch
from .optim import FusedAdam
# re-exported: bench.py, tools/ and the tests import GraphStep, gather_batch and DeviceLoader from this module
from .runtime import (DeviceLoader, GraphStep, KernelFn, KernelModule, cached_workspace, eager_step,  # noqa: F401
                      gather_batch, train_step)


class _EEGNetFn(KernelFn):
    @staticmethod
    def forward(ctx, x, model, *params):
        # EEGNet_tor._forward_output: the probabilities tensor this forward wrote, no copy kernel.  (A detached alias, not
        # the saved object itself: returning the very tensor that the model also keeps for its backward crashes hipGraph
        # capture in torch 2.10.)  The alias shares its version counter with the saved tensor: an in-place edit of the
        # returned scores before backward (clamp_, += eps ...) would silently corrupt dense_softmax_bwd's input - checked
        # in backward.
        out = KernelFn.forward(ctx, x, model, *params)
        ctx.probs_version = model._saved.probs._version
        return out

    @staticmethod
    def backward(ctx, dprobs):
        saved = ctx.model._saved
        if saved is not None and saved.token == ctx.token and saved.probs._version != ctx.probs_version:
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
        # kernels of csrc/eegnet_canon.hip (`_generic`), whose LDS tiles bound it at the sizes below.  `_path` is the
        # schedule of the one or the other (eegnet_paths): a plain object, absent from state_dict() and parameters()
        self._generic = not (F1 == 8 and D == 8 and F2 == 64 and 1 <= kernLength <= 300 and 1 <= Chans <= 32)
        self._path = GenericPath(self) if self._generic else FastPath(self)
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
        # How the exact-fp32 firstConv and its weight gradient are evaluated.  "fft": overlap-save blocks of 1024-point
        # FFTs (csrc/eegnet_fir_fft.hip: ~350 flops per output sample for the 8 filters together instead of 4800 - the two
        # kernels become HBM-bound); "mfma": the Toeplitz GEMMs on the fp32 matrix cores (csrc/eegnet_fir.hip); "auto"
        # (default): FFT for recordings of at least two 704-sample blocks and kernels of <= 321 taps, MFMA for short epochs
        # (the reference's own [B,1,30,500], where one FFT block would be mostly padding).  EAV_FIR_ALGO overrides.
        self.fir_algo = os.environ.get("EAV_FIR_ALGO", "auto")
        self.conv_algo = os.environ.get("EAV_CONV_ALGO", "auto")      # separableConv: see FastPath.use_conv_fft
        # frequency-domain separableConv backward from ONE pack launch that writes the spectra of both gradients and - in a
        # training step - forms du3 from dp3 / u3 while it loads (eav_conv64_fft_bwd: no eav_bn_elu_pool_bwd_apply launch, no
        # du3 tensor, one pack launch less); False / EAV_CONV_FUSE=0: the separate launches (bit-identical results)
        self.conv_fuse = os.environ.get("EAV_CONV_FUSE", "1") != "0"
        # Train-mode GraphStep steps on the FFT FIR path: the weight gradient takes y1's share of dW from per-trial tables of
        # the HBM-resident data set (eegnet_paths.InputTables, built on the first eager step) instead of reading y1 back.
        # False / EAV_FIR_XTAB=0: the y1-reading kernel, as forward() and forward_indexed() always use it.  The tables cost
        # 4 (K K + K) bytes per trial (72 MB for 200 trials at 300 taps); a data set whose tables would exceed
        # `fir_xtab_budget` bytes (1 GiB: ~2900 trials at 300 taps) keeps the y1-reading kernel.  They follow in-place torch
        # writes to the data set (GraphStep.run compares its _version); a write that bypasses torch (a raw kernel, a
        # DLPack alias) needs refresh_input_tables(xs).
        self.fir_xtab = os.environ.get("EAV_FIR_XTAB", "1") != "0"
        self.fir_xtab_budget = 1 << 30
        self._xtabs = {}                       # InputTables by data set, for the life of the model (FastPath.input_tables)
        self._infer = False                    # set per call: no-grad eval-mode forward
        # validate()'s forward with block 1 as ONE kernel (eav_eegnet_block1_infer: y1 / z never written).  Opt-in: at the
        # benchmark shape [64,1,30,10000] it measures 1.35 ms against 1.30 ms for the training kernels in eval mode - with its
        # 128 z accumulators per lane it runs one wave per SIMD and cannot hide its VALU tail behind another wave's MFMAs
        self.fused_eval = False

    # ------------------------------------------------------------------ plumbing
    def _use_fft(self):
        return self._path.use_fft()

    def _run(self, x):
        self._require_same_device(x)
        self._ensure_flat()
        # no-grad evaluation (validate(), EEGNet_tor.py:118-135): block 1 can run as one fused kernel, see FastPath.forward
        self._infer = (not torch.is_grad_enabled()) and (not self.training)
        return _EEGNetFn.apply(x, self, *self._params())

    def forward(self, x):
        self._require_gpu(x)
        if x.dim() == 3:
            x = x.unsqueeze(1)
        if x.dim() != 4 or x.shape[1] != 1 or x.shape[2] != self.Chans or x.shape[3] != self.Samples:
            raise ValueError(f"expected input [B,1,{self.Chans},{self.Samples}], got {tuple(x.shape)}")
        return self._run(x.contiguous().float())

    def refresh_input_tables(self, xs=None, force=True):
        """Rebuild, in place, the InputTables of the data set `xs` (None: of every data set) - after a write to it that
        torch does not see.  force=False: only those whose data._version has moved on (GraphStep.run)."""
        for t in self._xtabs.values():
            if (xs is None or t.data.data_ptr() == xs.data_ptr()) and (force or t.version != t.data._version):
                t.build()

    def refresh_batch_tables(self, xs):
        self.refresh_input_tables(xs, force=False)

    def _indexed(self, data, idx, step_begin=None):
        if data.dim() != 4 or data.shape[1] != 1 or data.shape[2] != self.Chans or data.shape[3] != self.Samples or \
                not data.is_cuda or data.dtype != torch.float32 or not data.is_contiguous():
            raise ValueError(f"expected a contiguous fp32 device array [N,1,{self.Chans},{self.Samples}]")
        if idx.dtype != torch.int64 or idx.device != data.device or idx.dim() != 1:
            raise ValueError("idx must be a 1-D int64 tensor on the data's device")
        return IndexedBatch(data, idx, step_begin)

    def forward_indexed(self, data, idx):
        """forward(data[idx]) without materialising data[idx] where the kernels read in place (Trainer_uni's per-step batch
        assembly, EEGNet_tor.py:100-101): `data` [N,1,Chans,Samples] fp32 contiguous on the device, `idx` device int64 [B]."""
        return self._run(self._indexed(data, idx))

    def forward_batch(self, xs, ys, idx, optimizer):
        """GraphStep's batch: read in place through the index vector (forward_indexed); only the labels are gathered - by
        the forward's own step-counter launch where it can take them (eav_step_begin: the label gather, the optimiser's
        step count and the dropout / BatchNorm counters in ONE graph node instead of three; FusedAdam.step() then skips its
        own eav_counter_inc for this one step), else here."""
        if not (xs.is_cuda and xs.dim() == 4 and xs.is_contiguous()):
            return super().forward_batch(xs, ys, idx, optimizer)
        targets = torch.empty(idx.numel(), dtype=torch.long, device=xs.device)
        optimizer.step_counted = False       # (a step that failed between its two halves must not leave the flag set)
        # (the data set of a GraphStep stays put: a train-mode step takes y1's share of the firstConv gradient from its tables)
        batch = self._indexed(xs, idx, self._path.step_begin_args(optimizer, ys, idx, targets))
        batch.xtab = self._path.input_tables(xs)
        scores = self._run(batch)
        optimizer.step_counted = batch.merged
        if not batch.merged:
            _lib.call("eav_gather_i64", ys.data_ptr(), idx.data_ptr(), targets.data_ptr(), idx.numel(), _lib.stream_ptr())
        return scores, targets

    # ------------------------------------------------------------------ kernels: the schedule of eegnet_paths
    def _launch_forward(self, x):
        return self._path.forward(x)

    def _forward_output(self):
        return self._saved.probs.detach()          # see _EEGNetFn

    def _launch_backward(self, dprobs, token):
        self._check_token(token)
        return self._path.backward(dprobs)


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
