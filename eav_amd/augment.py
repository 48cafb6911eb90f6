"""Input augmentation of the fine-tuning trainers: mixup, SpecAugment-style time / frequency masking and a horizontal
flip, applied while a batch is assembled in HBM (``eav_augment_gather``, csrc/augment.hip).

The AST checkpoint the audio trainer starts from was trained with mixup and time / frequency masking (Gong et al., "AST:
Audio Spectrogram Transformer", 2021); an EAV subject gives 280 training trials to an 86 M-parameter encoder.  The random
part is drawn on the host, once per epoch, into one int32 table (`plan_epoch`) that travels to the device in one copy;
the kernel reads one record of it per output sample (`apply`).  The table is the whole interface between the two: a test
replays it with NumPy.

A sample of the device-resident split is viewed as a matrix [R, C] with C contiguous: an AST clip [time, mel] has
R = time and C = mel, so `time_mask` draws row bands and `freq_mask` column bands; a ViT frame [3, H, W] has R = 3 H and
C = W, so `hflip` reverses the columns.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .runtime import gather_labels

RECORD_INTS = 12        # EAV_AUGMENT_RECORD_INTS of include/eav_hip.h
# words of a record
SRC, PARTNER, LAMBDA, FLIP, ROW_BANDS, COL_BANDS = 0, 1, 2, 3, 4, 8      # bands: [r0, r1, r0', r1'] / [c0, c1, c0', c1']


def sample_matrix_shape(x):
    """(R, C) of the samples of a split x [N, ...]: the last axis is the columns, everything between the rows."""
    if x.dim() < 2:
        raise ValueError(f"augment: samples of shape {tuple(x.shape[1:])} have no column axis")
    C = int(x.shape[-1])
    return int(x[0].numel()) // C, C


class BatchAugment:
    """mixup_alpha > 0: mixup (Zhang et al., 2018) with lambda ~ Beta(alpha, alpha), one partner per sample from the same
    micro-batch; time_mask / freq_mask > 0: up to two row bands / column bands per sample set to `fill` (torchaudio's
    TimeMasking / FrequencyMasking applied twice, as AST's recipe does); hflip: each sample mirrored along its columns with
    probability 0.5.  With every option off the records are plain gathers (lambda 1, no flip, empty bands).

    `fill` (attribute, default 0.0) is the value of a masked cell: 0.0 is the mean of a normalised spectrogram."""

    def __init__(self, mixup_alpha=0.0, time_mask=0, freq_mask=0, hflip=False, seed=0):
        if not float(mixup_alpha) >= 0.0:
            raise ValueError(f"BatchAugment: mixup_alpha {mixup_alpha!r} must be >= 0")
        for name, v in (("time_mask", time_mask), ("freq_mask", freq_mask)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
                raise ValueError(f"BatchAugment: {name} {v!r} must be an integer >= 0")
        self.mixup_alpha, self.time_mask, self.freq_mask = float(mixup_alpha), int(time_mask), int(freq_mask)
        self.hflip, self.seed = bool(hflip), int(seed)
        self.fill = 0.0

    @property
    def active(self):
        return self.mixup_alpha > 0.0 or self.time_mask > 0 or self.freq_mask > 0 or self.hflip

    @staticmethod
    def _bands(rng, n, param, size):
        """[n, 4] = two bands [start, start + width) per sample: width ~ U{0 .. param - 1} (cut to `size`), start ~
        U{0 .. size - width - 1} (0 where the band fills the axis) - torchaudio's draw, in integers."""
        width = np.minimum(rng.integers(0, param, size=(n, 2)), size)
        start = rng.integers(0, np.maximum(size - width, 1))
        return np.stack([start[:, 0], start[:, 0] + width[:, 0], start[:, 1], start[:, 1] + width[:, 1]], axis=1)

    def plan_epoch(self, index_batches, epoch, shape=None):
        """The epoch's table: int32 [samples of the epoch, RECORD_INTS], one record per output sample in the order of
        `index_batches` (a list of index lists, DeviceLoader.index_batches()).  shape = (R, C) of a sample, needed by the
        masks.  Host only; the same (seed, epoch) gives the same table.

        Draw order - the contract a replay relies on.  One numpy Generator, default_rng([seed, epoch]), is consumed
        micro-batch by micro-batch in the order given; inside a micro-batch of n samples, each draw made only when its
        option is on:
          1. mixup_alpha > 0   perm = permutation(n): sample k's partner is index_batch[perm[k]] - inside the micro-batch
          2. mixup_alpha > 0   lam = beta(alpha, alpha), folded to max(lam, 1 - lam) so that the first label stays the
                               primary one, rounded to fp32: ONE lambda per micro-batch
          3. hflip             random(n) < 0.5, one coin per sample
          4. time_mask > 0     width = integers(0, time_mask, (n, 2)) cut to R; start = integers(0, max(R - width, 1)):
                               two row bands per sample
          5. freq_mask > 0     the same with freq_mask and C: two column bands per sample
        Without mixup the partner is the sample itself and lambda is 1."""
        rng = np.random.default_rng([self.seed, int(epoch)])
        if (self.time_mask or self.freq_mask) and shape is None:
            raise ValueError("BatchAugment.plan_epoch: the masks need shape=(R, C)")
        R, C = (int(shape[0]), int(shape[1])) if shape is not None else (0, 0)
        parts = []
        for idx in index_batches:
            src = np.asarray(idx, dtype=np.int64)
            n = len(src)
            rec = np.zeros((n, RECORD_INTS), dtype=np.int32)
            rec[:, SRC] = rec[:, PARTNER] = src
            lam = np.float32(1.0)
            if self.mixup_alpha > 0.0:
                rec[:, PARTNER] = src[rng.permutation(n)]
                lam = rng.beta(self.mixup_alpha, self.mixup_alpha)
                lam = np.float32(max(lam, 1.0 - lam))
            rec[:, LAMBDA] = np.array([lam], dtype=np.float32).view(np.int32)[0]
            if self.hflip:
                rec[:, FLIP] = rng.random(n) < 0.5
            if self.time_mask > 0:
                rec[:, ROW_BANDS:ROW_BANDS + 4] = self._bands(rng, n, self.time_mask, R)
            if self.freq_mask > 0:
                rec[:, COL_BANDS:COL_BANDS + 4] = self._bands(rng, n, self.freq_mask, C)
            parts.append(rec)
        return np.concatenate(parts, axis=0) if parts else np.zeros((0, RECORD_INTS), dtype=np.int32)

    def apply(self, loader, table_slice, need_soft_targets, num_classes=None):
        """One batch from `loader` (a DeviceLoader): table_slice is the batch's records, a contiguous int32 device tensor
        [B, RECORD_INTS].  Returns (xb, tb): xb [B, ...] the augmented inputs; tb the soft targets [B, num_classes]
        (lambda onehot(y[i]) + (1 - lambda) onehot(y[j]), class-index labels only) when need_soft_targets, else the
        labels of the source samples."""
        x, y = loader.x, loader.y
        if not x.is_cuda:
            raise _lib.EavError("BatchAugment.apply needs a device-resident loader (no CPU fallback)")
        if table_slice.dtype != torch.int32 or table_slice.dim() != 2 or table_slice.shape[1] != RECORD_INTS \
                or table_slice.device != x.device or not table_slice.is_contiguous():
            raise _lib.EavError(f"BatchAugment.apply: the records must be a contiguous int32 [B, {RECORD_INTS}] tensor on "
                                f"{x.device}")
        B = int(table_slice.shape[0])
        R, C = sample_matrix_shape(x)
        out = torch.empty((B,) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
        tout = None
        if need_soft_targets:
            if y.dtype != torch.int64 or y.dim() != 1 or not num_classes or num_classes < 1:
                raise _lib.EavError("BatchAugment.apply: soft targets need int64 class labels and num_classes")
            tout = torch.empty(B, int(num_classes), dtype=torch.float32, device=x.device)
        _lib.call("eav_augment_gather", x.data_ptr(), y.data_ptr() if tout is not None else None, table_slice.data_ptr(),
                  float(self.fill), out.data_ptr(), _lib.ptr(tout), B, R, C, int(num_classes or 0), _lib.stream_ptr())
        if tout is not None:
            return out, tout
        return out, gather_labels(y, table_slice[:, SRC].long())


class EpochPlan:
    """A planned epoch on the device: the table in one copy, handed out batch by batch in the order it was planned."""

    def __init__(self, augment, loader, index_batches, epoch, soft, num_classes):
        self.augment, self.loader, self.soft, self.num_classes = augment, loader, bool(soft), num_classes
        self.host_table = augment.plan_epoch(index_batches, epoch, sample_matrix_shape(loader.x))
        self.table = torch.from_numpy(self.host_table).to(loader.x.device)
        self._pos = 0

    def next(self, n):
        """(xb, tb) of the next micro-batch of n samples."""
        part = self.table[self._pos:self._pos + n]
        assert part.shape[0] == n, "EpochPlan: more batches asked for than planned"
        self._pos += n
        return self.augment.apply(self.loader, part, self.soft, self.num_classes)
