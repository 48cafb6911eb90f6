"""The criteria: cross-entropy, BCE-with-logits and MSE, each one fused launch that gives the loss and its input gradient.

Host-side mirrors of what the reference trainers construct:
  * ``nn.CrossEntropyLoss()``                          EEGNet_tor.py:81, Transformer_Audio.py:31

  * ``nn.BCEWithLogitsLoss()`` / ``nn.MSELoss()``      the other two losses HF's classification models pick by
    ``config.problem_type`` (transformers/loss/loss_utils.py, ForSequenceClassificationLoss)

The arithmetic runs in libeav_hip.so (``eav_ce_fwd_bwd`` / ``eav_bce_logits_fwd_bwd`` / ``eav_mse_fwd_bwd``;
``eav_ce_general_fwd_bwd`` for ``CrossEntropyLoss(weight=..., label_smoothing=...)`` and class-probability targets).
Imports nothing of the package but ``_lib``; ``eav_amd.optim`` re-exports the public names (the old import path).
"""
from __future__ import annotations

import os

import torch

from . import _lib


class _LossFn(torch.autograd.Function):
    """The criteria's one autograd function: `launch(loss, dsc)` is the criterion's forward launch, which produces the
    loss and d loss / d scores together."""

    @staticmethod
    def forward(ctx, scores, launch):
        loss = torch.empty((), dtype=torch.float32, device=scores.device)
        dsc = torch.empty_like(scores) if ctx.needs_input_grad[0] else None      # no gradient buffer under no_grad (validate())
        launch(loss, dsc)
        ctx.dsc = dsc
        return loss

    @staticmethod
    def backward(ctx, gout):
        return _seeded(ctx.dsc, gout), None


def _seeded(dsc, gout):
    """The gradient a criterion's backward returns.  d loss / d scores (`dsc`) was produced by the forward launch; the
    incoming gradient (1.0 for loss.backward()) is applied by the library - no torch kernel inside a captured step.
    `unit_gradient(device)` is a constant 1.0 that callers may pass as the seed (loss.backward(gradient=...)): recognised
    here, nothing is launched."""
    if gout.data_ptr() != _UNIT.get(gout.device, (None, 0))[1]:
        # any other upstream gradient scales a COPY: dsc stays the unit-gradient result, so a second backward
        # (retain_graph=True) or a re-used graph never scales twice
        out = dsc.clone()
        _lib.call("eav_scale_by_scalar", out.data_ptr(), gout.contiguous().data_ptr(), out.numel(), _lib.stream_ptr())
        return out
    return dsc


_UNIT = {}


def unit_gradient(device):
    """A device-resident constant 1.0 to seed ``loss.backward(gradient=unit_gradient(dev))`` with: autograd then needs no
    fill kernel for the implicit ones_like(loss), and the CE backward recognises it and skips its scaling launch."""
    device = torch.device(device)
    if device not in _UNIT:
        t = torch.ones((), dtype=torch.float32, device=device)
        _UNIT[device] = (t, t.data_ptr())
    return _UNIT[device][0]


class _Scratch:
    """A kernel's per-row scratch, kept on the criterion: one fp32 buffer per (batch, device), sized by the library's
    `entry`(batch) - nothing is allocated for it in the launch path."""

    def __init__(self, entry):
        self._entry, self._buffers = entry, {}

    def __len__(self):
        return len(self._buffers)

    def get(self, scores):
        key = (scores.shape[0], scores.device)
        if key not in self._buffers:
            self._buffers[key] = torch.empty(_lib.plain(self._entry, key[0]), dtype=torch.float32, device=scores.device)
        return self._buffers[key]


def _check_scores(scores, targets_on_device, who):
    """`scores` as every criterion takes them; `targets_on_device`: the targets are a device tensor too (one refusal
    covers both).  Every operand goes to the kernel as a raw pointer: a host tensor would be dereferenced on the GPU."""
    if not isinstance(scores, torch.Tensor) or not scores.is_cuda or not targets_on_device:
        raise _lib.EavError(f"{who} needs device tensors (no CPU fallback)")
    if scores.dim() != 2 or scores.dtype != torch.float32 or not scores.is_contiguous():
        raise _lib.EavError(f"{who}: scores must be a contiguous fp32 [batch, classes] tensor, got "
                            f"{tuple(scores.shape)} {scores.dtype}")


def _check_out(t, dtype, what, scores, who):
    """An output buffer of an evaluation form (`accumulate`): a tensor of `dtype` on the scores' device."""
    if not isinstance(t, torch.Tensor) or t.device != scores.device or t.dtype != dtype or t.numel() < 1:
        raise _lib.EavError(f"{who}: {what} must be a {str(dtype).replace('torch.', '')} tensor on {scores.device}")


# classes the narrow head kernels are meant for (eav_dense_softmax_* keeps them in registers, eav_ce_fwd_bwd walks a row
# with one thread); Encoder.head_algo and CrossEntropyLoss.head_algo switch to the wide kernels above it
HEAD_NARROW_CLASSES = 16


def head_is_wide(algo, classes, found):
    """Whether `classes` classes go to the wide kernels under head_algo `algo`; `found` ("the head has") words the refusal."""
    if algo not in ("auto", "wide", "narrow"):
        raise ValueError(f"head_algo {algo!r}: expected 'auto', 'wide' or 'narrow'")
    if algo == "narrow" and classes > HEAD_NARROW_CLASSES:
        raise NotImplementedError(f"head_algo 'narrow' takes at most {HEAD_NARROW_CLASSES} classes, {found} {classes}")
    return algo == "wide" or (algo == "auto" and classes > HEAD_NARROW_CLASSES)


def _ce_launch(scratch, scores, targets, loss, dsc, ncorrect, flag, general=None):
    """eav_ce_fwd_bwd (scratch None), or eav_ce_wide_fwd_bwd (one wave per row) with its per-row scratch; with `general` =
    (class weights or None, label smoothing), eav_ce_general_fwd_bwd on int64 labels or fp32 class probabilities."""
    B, NC = scores.shape
    if general is not None:
        weight, smoothing = general
        soft = targets.dtype == torch.float32
        _lib.call("eav_ce_general_fwd_bwd", scores.data_ptr(), None if soft else targets.data_ptr(),
                  targets.data_ptr() if soft else None, _lib.ptr(weight), float(smoothing), loss.data_ptr(), _lib.ptr(dsc),
                  _lib.ptr(ncorrect), flag.data_ptr(), scratch.data_ptr(), B, NC, _lib.stream_ptr())
    elif scratch is not None:
        _lib.call("eav_ce_wide_fwd_bwd", scores.data_ptr(), targets.data_ptr(), loss.data_ptr(), _lib.ptr(dsc),
                  _lib.ptr(ncorrect), flag.data_ptr(), scratch.data_ptr(), B, NC, _lib.stream_ptr())
    else:
        _lib.call("eav_ce_fwd_bwd", scores.data_ptr(), targets.data_ptr(), loss.data_ptr(), _lib.ptr(dsc),
                  _lib.ptr(ncorrect), flag.data_ptr(), B, NC, _lib.stream_ptr())


class CrossEntropyLoss:
    """``nn.CrossEntropyLoss()`` (mean reduction) as one fused HIP kernel that
    produces the loss and its input gradient together.

    Like torch, targets equal to -100 (the default ignore_index) are excluded from the mean and get a zero gradient, and
    any other class index outside [0, classes) is rejected: the kernel never indexes with such a label (the row
    contributes nothing to the loss and receives a zero gradient) and records it in a device flag; ``check()`` reads the flag (one host synchronisation) and
    raises.  The trainers call it once per epoch - a per-step check would serialise host and GPU; code that drives the
    criterion directly calls ``check()`` whenever it synchronises anyway.

    ``head_algo`` routes by the class count like ``Encoder.head_algo``: "auto" (default; EAV_HEAD_ALGO overrides) takes
    eav_ce_wide_fwd_bwd above 16 classes and eav_ce_fwd_bwd up to there, "wide" forces the former at any width and
    "narrow" the latter, which raises above 16 classes as the Encoder's does.  The wide kernel's per-row scratch is kept
    on the criterion, one buffer per (batch, device): nothing is allocated for it in the launch path.

    ``weight`` (per-class weights, anything torch.as_tensor takes) and ``label_smoothing`` (0 <= eps <= 1) are torch's
    arguments of those names, keyword-only and fixed at construction - read-only attributes: a captured step has the
    scalar baked in, a later change could silently not apply.  Targets may also be fp32 class probabilities
    [batch, classes] (mixup's soft targets).  The defaults on class indices launch what they always did; anything else
    goes to eav_ce_general_fwd_bwd (csrc/head_ce_soft.hip) at every width - ``head_algo`` does not apply there - with
    its own per-(batch, device) scratch.  The weights are kept as an fp32 tensor and moved to the device of the first
    scores; a length other than the class count raises.  With class indices the mean is over the weights of the valid
    labels (torch's rule); labels whose weights add up to 0 give a NaN loss like an all-ignored batch."""

    def __init__(self, *, weight=None, label_smoothing=0.0):
        smoothing = float(label_smoothing)
        if not 0.0 <= smoothing <= 1.0:
            raise ValueError(f"CrossEntropyLoss: label_smoothing {label_smoothing!r} is outside [0, 1]")
        if weight is not None:
            weight = torch.as_tensor(weight).detach().to(torch.float32).reshape(-1).contiguous().clone()
            if weight.numel() < 1:
                raise ValueError("CrossEntropyLoss: weight is empty")
        self._weight, self._smoothing = weight, smoothing
        self._flag = None
        self._scratch = _Scratch("eav_ce_wide_ws_floats")
        self._general_scratch = _Scratch("eav_ce_general_ws_floats")
        self.head_algo = os.environ.get("EAV_HEAD_ALGO", "auto")

    weight = property(lambda self: self._weight, doc="per-class weights (fp32 tensor) or None; fixed at construction")
    label_smoothing = property(lambda self: self._smoothing, doc="the smoothing factor; fixed at construction")

    def _wide(self, classes):
        return head_is_wide(self.head_algo, classes, "the scores have")

    def _launcher(self, scores, targets, ncorrect=None):
        """launch(loss, dsc) over _ce_launch, routed before anything is allocated: the default criterion on class indices
        keeps its two kernels (the wide one with its row terms for this batch size), everything else takes the general
        one with the weights on the scores' device.  The label flag is created here, on first use."""
        if self._flag is None or self._flag.device != scores.device:
            self._flag = torch.zeros((), dtype=torch.int32, device=scores.device)
        flag, NC = self._flag, scores.shape[1]
        if targets.dim() == 1 and self._weight is None and self._smoothing == 0.0:
            scratch, general = self._scratch.get(scores) if self._wide(NC) else None, None
        else:
            if self._weight is not None:
                if self._weight.numel() != NC:
                    raise ValueError(f"CrossEntropyLoss: {self._weight.numel()} class weights for {NC} classes")
                if self._weight.device != scores.device:
                    self._weight = self._weight.to(scores.device)
            scratch, general = self._general_scratch.get(scores), (self._weight, self._smoothing)
        return lambda loss, dsc: _ce_launch(scratch, scores, targets, loss, dsc, ncorrect, flag, general)

    @staticmethod
    def _targets(scores, targets, who):
        """int64 [B] class indices or fp32 [B, NC] class probabilities, contiguous."""
        if targets.dim() == 2:
            if tuple(targets.shape) != tuple(scores.shape):
                raise _lib.EavError(f"{who}: class-probability targets {tuple(targets.shape)} for scores {tuple(scores.shape)}")
            if targets.dtype != torch.float32:
                targets = targets.float()
            return targets.contiguous()
        if targets.dim() != 1 or targets.numel() != scores.shape[0]:
            raise _lib.EavError(f"{who}: {targets.numel()} targets for {scores.shape[0]} rows of scores")
        if targets.dtype != torch.int64:
            targets = targets.long()
        return targets.contiguous()

    def check(self):
        if self._flag is not None:
            bad = int(self._flag.item())
            if bad != 0:
                self._flag.zero_()
                raise _lib.EavError(f"CrossEntropyLoss: target {bad - 1 if bad > 0 else bad} is outside [0, classes) "
                                    "(the reference's labels 1,3,5,7,9 must be mapped to 0..4 first)")

    def accumulate(self, scores, targets, loss_out, ncorrect):
        """Evaluation form (no gradient, nothing read back): writes the mean loss of this batch into the 0-dim device
        tensor `loss_out` and adds the number of argmax hits to the device int32 `ncorrect` - a validation loop reads
        both once per epoch instead of synchronising twice per batch (EEGNet_tor.py:126-130 calls .item() per batch)."""
        who = "CrossEntropyLoss.accumulate"
        _check_scores(scores, True, who)
        soft = isinstance(targets, torch.Tensor) and targets.dim() == 2
        if soft and not targets.is_floating_point():
            raise TypeError(f"{who}: [batch, classes] targets are class probabilities, got {targets.dtype}")
        if not isinstance(targets, torch.Tensor) or targets.device != scores.device \
                or (tuple(targets.shape) != tuple(scores.shape) if soft else
                    targets.dim() != 1 or targets.numel() != scores.shape[0]):
            raise _lib.EavError(f"{who}: targets must be {scores.shape[0]} labels on {scores.device} "
                                "(no CPU fallback: move the loader's tensors to the device)")
        _check_out(loss_out, torch.float32, "loss_out", scores, who)
        _check_out(ncorrect, torch.int32, "ncorrect", scores, who)
        self._launcher(scores, self._targets(scores, targets, who), ncorrect)(loss_out, None)

    def __call__(self, scores, targets):
        if isinstance(targets, torch.Tensor) and targets.dim() == 2 and not targets.is_floating_point():
            raise TypeError(f"CrossEntropyLoss: [batch, classes] targets are class probabilities, got {targets.dtype}")
        _check_scores(scores, targets.is_cuda, "CrossEntropyLoss")
        return _LossFn.apply(scores, self._launcher(scores, self._targets(scores, targets, "CrossEntropyLoss")))


class _ElementLoss:
    """What BCEWithLogitsLoss and MSELoss share: the mean over all batch x classes elements and its gradient from one
    launch of csrc/head_loss.hip (one wave per row, row sums added in row order - no atomics, two runs give the same bits).

    Targets are fp32 [batch, classes] on the scores' device ([batch] accepted for one class; integer targets are
    converted to fp32) and are not validated - torch accepts any float - so `check()` has nothing to report and is a
    no-op that trainers may call blindly.  The kernels' per-row scratch is kept on the criterion, one buffer per
    (batch, device): nothing is allocated for it in the launch path, and nothing synchronises with the host."""

    _NAME = None

    def __init__(self):
        self._scratch = _Scratch("eav_head_loss_ws_floats")

    def check(self):
        pass

    def _operands(self, scores, targets, who):
        _check_scores(scores, isinstance(targets, torch.Tensor) and targets.is_cuda, who)
        B, NC = scores.shape
        # a tensor on another device would be dereferenced on this GPU
        if targets.device != scores.device:
            raise _lib.EavError(f"{who}: targets are on {targets.device}, the scores on {scores.device}")
        if tuple(targets.shape) != (B, NC) and not (NC == 1 and tuple(targets.shape) == (B,)):
            raise _lib.EavError(f"{who}: targets {tuple(targets.shape)} for scores {(B, NC)}")
        if targets.dtype != torch.float32:
            targets = targets.float()
        return targets.reshape(B, NC).contiguous()

    def __call__(self, scores, targets):
        targets = self._operands(scores, targets, self._NAME)
        return _LossFn.apply(scores, lambda loss, dsc: self._launch(scores, targets, loss, dsc, None))


class BCEWithLogitsLoss(_ElementLoss):
    """``nn.BCEWithLogitsLoss()`` (mean over batch x classes; no pos_weight): HF's loss for
    problem_type "multi_label_classification".  Term max(x, 0) - x t + log1p(exp(-|x|)), torch's form, finite for any
    finite logit; gradient (sigmoid(x) - t) / (batch x classes).  See _ElementLoss for targets, scratch and check()."""

    _NAME = "BCEWithLogitsLoss"

    def _launch(self, scores, targets, loss, dsc, nhits):
        B, NC = scores.shape
        _lib.call("eav_bce_logits_fwd_bwd", scores.data_ptr(), targets.data_ptr(), _lib.ptr(loss), _lib.ptr(dsc),
                  _lib.ptr(nhits), self._scratch.get(scores).data_ptr(), B, NC, _lib.stream_ptr())

    def accumulate(self, scores, targets, loss_out, nhits):
        """Evaluation form (no gradient, nothing read back): the batch's mean loss into the 0-dim device tensor
        `loss_out`, and the number of elements with (score > 0) == (target > 0.5) - the multi-label counterpart of
        CrossEntropyLoss's argmax hits - added to the device int32 `nhits`."""
        who = "BCEWithLogitsLoss.accumulate"
        targets = self._operands(scores, targets, who)
        _check_out(loss_out, torch.float32, "loss_out", scores, who)
        _check_out(nhits, torch.int32, "nhits", scores, who)
        self._launch(scores, targets, loss_out, None, nhits)


class MSELoss(_ElementLoss):
    """``nn.MSELoss()`` (mean over batch x classes): HF's loss for problem_type "regression".  Term (x - t)^2, gradient
    2 (x - t) / (batch x classes).  See _ElementLoss for targets, scratch and check()."""

    _NAME = "MSELoss"

    def _launch(self, scores, targets, loss, dsc, nhits):
        B, NC = scores.shape
        _lib.call("eav_mse_fwd_bwd", scores.data_ptr(), targets.data_ptr(), _lib.ptr(loss), _lib.ptr(dsc),
                  self._scratch.get(scores).data_ptr(), B, NC, _lib.stream_ptr())

    def accumulate(self, scores, targets, loss_out):
        """Evaluation form (no gradient, nothing read back): the batch's mean loss into the 0-dim device tensor `loss_out`."""
        who = "MSELoss.accumulate"
        targets = self._operands(scores, targets, who)
        _check_out(loss_out, torch.float32, "loss_out", scores, who)
        self._launch(scores, targets, loss_out, None, None)
