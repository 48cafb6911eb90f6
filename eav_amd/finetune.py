"""Shared two-phase fine-tuning machinery of the audio and vision trainers.

Both reference trainers (Transformer_Audio.py:44-103, Transformer_Vision.py:61-129) run the same schedule: set
the learning rate of ONE AdamW that spans both phases (Q10/Q11), freeze everything but `model.classifier` or
unfreeze all, loop epochs of (train batches -> eval batches), and keep the test logits of the last unfrozen
epoch in `outputs_test` (Q15).  They differ only in bookkeeping (how accuracy is averaged, what is printed and
logged).  This module holds the common part on top of eav_amd.transformer.Encoder; the two public classes in
audio.py / vision.py keep the reference's constructors, method signatures and console output.
"""
from __future__ import annotations

import contextlib
import os
import shutil

import numpy as np
import torch

from . import _lib
from .augment import BatchAugment, EpochPlan
from .criteria import BCEWithLogitsLoss, CrossEntropyLoss, MSELoss
from .optim import FusedAdam, LRSchedule, WeightAveraging
from .runtime import DeviceLoader
from .transformer import PROBLEM_TYPES, Encoder


def balanced_class_weights(labels, n_classes):
    """n / (n_classes * count_c) over the valid labels, float64 [n_classes]: sklearn's compute_class_weight("balanced")
    for the classes 0 .. n_classes - 1; a class without a sample gets 0 (it is never a target)."""
    y = np.asarray(labels).reshape(-1)
    y = y[(y >= 0) & (y < n_classes)].astype(np.int64)
    counts = np.bincount(y, minlength=n_classes).astype(np.float64)
    w = np.zeros(n_classes, dtype=np.float64)
    w[counts > 0] = len(y) / (n_classes * counts[counts > 0])
    return w


def encoder_layer_id(name, layers):
    """The layer id of an Encoder parameter for layer-wise learning-rate decay (BEiT's get_num_layer_for_vit): 0 for the
    embeddings (cls / distillation tokens, position table, patch projection), i + 1 for encoder layer i, layers + 1 for
    the final LayerNorm and the classifier (AST's classifier.layernorm included)."""
    parts = name.split(".")
    if "embeddings" in parts:
        return 0
    if "layers" in parts:
        return int(parts[parts.index("layers") + 1]) + 1
    return layers + 1


def encoder_no_decay(name):
    """Whether HF Trainer's rule keeps weight decay off this Encoder parameter: biases, LayerNorm weights, and the
    parameters that are no matrices at all - the tokens and the position table."""
    if name.endswith(".bias") or name.endswith("_token") or name.endswith("position_embeddings"):
        return True
    return name.endswith(".weight") and "layernorm" in name.split(".")[-2]


def encoder_param_groups(model, lr, weight_decay, layer_decay=1.0, decay_bias_and_norm=True):
    """torch param-group dicts for an Encoder (a pure function of its parameter names: runs on a CPU model).

    layer_decay: the group of layer id `i` (encoder_layer_id) gets lr * layer_decay ** (layers + 1 - i) - the head is
    updated at lr, the embeddings at lr * layer_decay ** (layers + 1).  decay_bias_and_norm=False moves every parameter
    encoder_no_decay names into groups with weight_decay 0.  Every parameter lands in exactly one group; next to
    "params", "lr" and "weight_decay" a group carries "names" (its parameters' names, in named_parameters() order),
    "layer_id" (None when layer_decay is 1: ids are not told apart) and "lr_scale".  With both options at their defaults
    there is one group."""
    layer_decay = float(layer_decay)
    if not 0.0 < layer_decay <= 1.0:
        raise ValueError(f"layer_decay {layer_decay!r} is outside (0, 1]")
    layers = model.cfg.layers
    groups = {}
    for name, p in model.named_parameters():
        lid = encoder_layer_id(name, layers) if layer_decay != 1.0 else None
        decays = bool(decay_bias_and_norm) or not encoder_no_decay(name)
        key = (-1 if lid is None else lid, not decays)
        if key not in groups:
            scale = 1.0 if lid is None else layer_decay ** (layers + 1 - lid)
            groups[key] = {"params": [], "names": [], "lr": float(lr) * scale,
                           "weight_decay": float(weight_decay) if decays else 0.0, "layer_id": lid, "lr_scale": scale}
        groups[key]["params"].append(p)
        groups[key]["names"].append(name)
    return [groups[k] for k in sorted(groups)]


def require_gpu(who):
    dev = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    if dev.type != "cuda":
        raise _lib.EavError(f"eav_amd.{who} needs an MI355X (no CPU fallback)")
    return dev


class FineTuneBase:
    """Owns model, optimiser, loaders; subclasses provide the reference-specific reporting.

    `problem_type` (keyword-only argument of both trainers, HF's config.problem_type): None or
    "single_label_classification" is the reference's schedule - integer labels, cross-entropy, argmax accuracy, the
    reference's printed lines.  "multi_label_classification" and "regression" take fp32 label rows [N, num_labels]
    ([N] for one label), train with BCEWithLogitsLoss / MSELoss, and report, where the reference's lines say
    "Accuracy: x%",
        multi-label   "Label Accuracy: x%"   elements with (logit > 0) == (target > 0.5) over all samples x labels,
                                             counted on the device by the criterion (nhits)
        regression    "MSE: v"               the mean squared error over all samples x labels (no accuracy exists)
    e.g. "Epoch 1/20, Training Label Accuracy: 50.00%, Test Label Accuracy: 50.00%" (audio) and "Epoch 1, Test MSE:
    0.123456" (vision); the log files get the same wording.  The model's cfg.problem_type is set, so save_pretrained
    writes it; `outputs_test` holds raw logits in every mode."""

    problem_type = None

    # Training-loop options, set between construction and train() like `cache_frozen_features` (the constructors keep
    # the reference's parameter lists):
    #   max_grad_norm                 None (the reference: no clipping) or the bound of the gradients' global L2 norm, HF
    #                                 Trainer's option of that name - FusedAdam(max_grad_norm=...), inside the step
    #   gradient_accumulation_steps   k >= 1: one optimiser step per k consecutive micro-batches of `batch_size`
    #                                 (_train_one_epoch); the effective batch is k * batch_size
    max_grad_norm = None
    gradient_accumulation_steps = 1

    # Regularisers, set the same way (single-label classification only, except the masks and the flip):
    #   label_smoothing   HF TrainingArguments' label_smoothing_factor: CrossEntropyLoss(label_smoothing=...)
    #   class_weights     None, one weight per class, or "balanced": n / (classes * count_c) over the training labels
    #                     (sklearn's compute_class_weight; a class without a training sample gets 0)
    #   mixup_alpha       > 0: mixup with lambda ~ Beta(alpha, alpha), the partner drawn from the sample's own micro-batch,
    #                     the loss taken on the mixed soft targets
    #   augment_seed      seeds the augmentation draws (with the count of augmented epochs: augment.BatchAugment.plan_epoch)
    # AudioModelTrainer adds time_mask / freq_mask, ImageClassifierTrainer hflip.  The criterion options hold in every
    # phase; the inputs are augmented only in epochs with freeze=False and never in _evaluate - the frozen phase keeps its
    # feature cache.  Training accuracy counts against the primary (first) label of a mixed sample.  With every option
    # at its default nothing of this is entered: the trainers launch what they always did.
    #   patch_dropout     0 <= p < 1, timm's PatchDropout (Encoder.patch_dropout): every sample of an unfrozen epoch keeps a
    #                     random max(1, int(P (1 - p))) of its P patch tokens - a regulariser that shortens the step.  Any
    #                     problem type.  The frozen phase (its feature cache, its launches) and _evaluate see every token.
    #   drop_path         0 <= r < 1, stochastic depth, timm's DropPath (Encoder.drop_path_rate): every sample of an unfrozen
    #                     epoch drops the whole residual branch of layer i with probability r i / (layers - 1).  Any problem
    #                     type, any geometry, with patch_dropout too.  The frozen phase and _evaluate drop nothing.
    label_smoothing = 0.0
    class_weights = None
    mixup_alpha = 0.0
    augment_seed = 0
    patch_dropout = 0.0
    drop_path = 0.0
    # Learning-rate options, set the same way; with all of them at their defaults _enter_phase does what it always did
    # and the optimiser keeps its one-launch-per-run path:
    #   lr_scheduler_type     "constant", "constant_with_warmup", "linear" or "cosine" (optim.LRSchedule, the lambdas of
    #                         transformers.get_scheduler): a fresh schedule per train() call over epochs x optimiser steps
    #                         per epoch (gradient_accumulation_steps counts groups, not micro-batches)
    #   warmup_ratio          the share of those steps spent warming up (rounded up, HF's rule); warmup_steps, when not
    #                         None, is the count itself
    #   layer_decay           < 1: layer-wise learning-rate decay, layer i at lr * layer_decay ** (layers + 1 - id)
    #   decay_bias_and_norm   False: no weight decay on biases, LayerNorm weights, tokens and the position table
    # Any of them switches the optimiser to its multi-tensor step (optim.FusedAdam(multi_tensor=True)): two launches per
    # step whatever the groups look like.  The epoch line gains ", lr x" under a non-constant schedule.
    lr_scheduler_type = "constant"
    warmup_ratio = 0.0
    warmup_steps = None
    layer_decay = 1.0
    decay_bias_and_norm = True
    _lr_options_applied = False         # the optimiser's groups / schedule were rebuilt by _apply_lr_options
    # Weight averaging, set the same way (optim.WeightAveraging, FusedAdam.set_averaging - the averages are updated inside
    # the optimiser step's own two launches):
    #   weight_averaging        None, "ema" (timm's ModelEma, AveragedModel with get_ema_multi_avg_fn) or "swa"
    #   ema_decay, ema_warmup   the EMA's decay; True: min(decay, (1 + n) / (10 + n)) while few steps have been averaged
    #   averaging_start_epoch   epochs - counted over the train() calls since averaging was attached - trained before the
    #                           first averaging step (converted to optimiser steps; gradient_accumulation_steps counts groups)
    #   averaging_every         average every k-th optimiser step from there
    # When set, _evaluate runs on the averaged weights - the epoch line and `outputs_test` come from them; in the frozen
    # phase only the head differs, so the feature cache stays valid - and save_pretrained writes them.  Training itself
    # is not perturbed: the trained parameters are bit-equal to a run without the option (the multi-tensor step it switches
    # to forms the bias corrections on the device, the default step on the host - the same fp64 expressions, rounded to
    # fp32 - and the element update is one function).  Attached by the first train()
    # call that sees the option and kept across the phases.  With None nothing of this is entered.
    weight_averaging = None
    ema_decay = 0.999
    ema_warmup = False
    averaging_start_epoch = 0
    averaging_every = 1

    _criterion_key = (0.0, None)        # (label_smoothing, class weights) loss_fn was built with
    _augmented_epochs = 0               # epochs planned so far: the `epoch` of BatchAugment.plan_epoch
    _augment = None                     # the phase's BatchAugment (None: batches are plain gathers)

    def _build(self, model_path, n_classes, lr, device, problem_type=None):
        """The reference's order (Transformer_Audio.py:22-24, Transformer_Vision.py:29-30): load the checkpoint with the
        head its config.json describes - 527 AudioSet or 1000 ImageNet classes for the stock downloads - then replace
        that head by a fresh Linear(hidden, n_classes); 1 <= n_classes <= transformer.HEAD_MAX_CLASSES."""
        self.device = device
        self.model = Encoder.from_pretrained(model_path)
        in_features = self.model.cfg.hidden
        fresh = torch.nn.Linear(in_features, n_classes)       # torch-default init, drawn from the torch RNG
        self.model.reset_head(fresh.weight.detach(), fresh.bias.detach())
        self.model.to(device)
        self.initial_lr = lr
        # AdamW with torch's default weight decay 0.01: the reference never forwards its own argument (Q10)
        self.optimizer = FusedAdam(self.model.parameters(), lr=lr, weight_decay=0.01, decoupled=True)
        if problem_type is not None and problem_type not in PROBLEM_TYPES:
            raise ValueError(f"problem_type {problem_type!r}: expected None or one of {PROBLEM_TYPES}")
        self.problem_type = problem_type
        if problem_type is not None:
            self.model.cfg.problem_type = problem_type
        self.loss_fn = {"multi_label_classification": BCEWithLogitsLoss, "regression": MSELoss}.get(
            problem_type, CrossEntropyLoss)()
        self.grad_sync = None

    def _classifies(self):
        """Integer class labels and cross-entropy (the reference's schedule)."""
        return self.problem_type in (None, "single_label_classification")

    def _resolved_class_weights(self):
        """class_weights as a tuple of floats (None: unweighted)."""
        cw = self.class_weights
        if cw is None:
            return None
        n_classes = self.model.cfg.num_labels
        if isinstance(cw, str):
            if cw != "balanced":
                raise ValueError(f'class_weights {cw!r}: expected None, a sequence or "balanced"')
            return tuple(balanced_class_weights(self.train_dataloader.y.cpu().numpy(), n_classes).tolist())
        cw = tuple(float(v) for v in np.asarray(cw, dtype=np.float64).reshape(-1))
        if len(cw) != n_classes:
            raise ValueError(f"class_weights: {len(cw)} weights for {n_classes} classes")
        return cw

    def _apply_regularisers(self, freeze):
        """The criterion of this phase (rebuilt when label_smoothing / class_weights changed since it was built) and the
        phase's BatchAugment (None: batches are plain gathers)."""
        smoothing, mixup = float(self.label_smoothing), float(self.mixup_alpha)
        if not self._classifies() and (smoothing != 0.0 or self.class_weights is not None or mixup != 0.0):
            raise ValueError(f"label_smoothing, class_weights and mixup_alpha need single-label classification, not "
                             f"problem_type {self.problem_type!r}")
        if mixup < 0.0:
            raise ValueError(f"mixup_alpha {self.mixup_alpha!r} must be >= 0")
        if self._classifies():
            key = (smoothing, self._resolved_class_weights())
            if key != self._criterion_key:
                self.loss_fn = CrossEntropyLoss(weight=key[1], label_smoothing=smoothing)
                self._criterion_key = key
        aug = BatchAugment(mixup, getattr(self, "time_mask", 0), getattr(self, "freq_mask", 0),
                           getattr(self, "hflip", False), self.augment_seed)
        aug.fill = float(getattr(self, "mask_fill", 0.0))
        self._augment = aug if aug.active and not freeze else None
        pd = float(self.patch_dropout)
        if not 0.0 <= pd < 1.0:
            raise ValueError(f"patch_dropout {self.patch_dropout!r} must satisfy 0 <= p < 1")
        self.model.patch_dropout = 0.0 if freeze else pd
        dp = float(self.drop_path)
        if not 0.0 <= dp < 1.0:
            raise ValueError(f"drop_path {self.drop_path!r} must satisfy 0 <= r < 1")
        self.model.drop_path_rate = 0.0 if freeze else dp

    def _epoch_plan(self, batches):
        """The augmentation plan of a training epoch over `batches` (None: plain gathers)."""
        aug = self._augment
        if aug is None:
            return None
        plan = EpochPlan(aug, self.train_dataloader, batches, self._augmented_epochs,
                         soft=self._classifies() and aug.mixup_alpha > 0.0, num_classes=self.model.cfg.num_labels)
        self._augmented_epochs += 1
        return plan

    def _train_batch(self, dl, idx, fc, plan):
        """(logits, targets, primary labels) of one training micro-batch: the head on cached features, or the model on the
        gathered - under a plan: augmented - inputs.  The primary labels are what accuracy counts against; they differ
        from the targets only under mixup, whose targets are class probabilities."""
        if fc is not None and fc["have_train"]:       # cached features: only the labels of the batch are gathered
            tb = dl.gather_labels(idx)
            return self.model.head(fc["train"][self._index(idx)]).logits, tb, tb
        if plan is not None:
            xb, tb = plan.next(len(idx))
            primary = dl.gather_labels(idx) if plan.soft else tb
        else:
            xb, tb = dl.gather(idx)
            primary = tb
        logits = self.model(xb).logits
        if fc is not None:
            fc["train"][self._index(idx)] = self.model.last_features()
        return logits, tb, primary

    def _loader(self, x, y, shuffle):
        if self._classifies():
            return DeviceLoader(x, y, self.batch_size, shuffle, self.device)
        return DeviceLoader(x, y, self.batch_size, shuffle, self.device, label_dtype=torch.float32)

    def save_pretrained(self, save_directory, averaged=True):
        """The fine-tuned model as an HF directory (Encoder.save_pretrained), with the preprocessor_config.json of the
        directory it was loaded from, if that had one.  An audio trainer built with max_length saves a model of that
        length (the position table fitted to it).  Under `weight_averaging` the averaged weights are written;
        averaged=False writes the last iterate."""
        length = getattr(self, "max_length", None)
        with self._averaged() if averaged else contextlib.nullcontext():
            self.model.save_pretrained(save_directory, **({} if length is None else {"max_length": length}))
        src = os.path.join(self.model.source_dir or "", "preprocessor_config.json")
        if self.model.source_dir and os.path.exists(src):
            dst = os.path.join(save_directory, "preprocessor_config.json")
            shutil.copyfile(src, dst)
            if length is not None:              # the feature extractor of the saved model pads to the saved length
                import json
                pre = json.load(open(dst))
                pre["max_length"] = int(length)
                with open(dst, "w") as f:
                    json.dump(pre, f, indent=2)
                    f.write("\n")

    def _metric_text(self, value):
        """The new modes' replacement of the reference's "Accuracy: x%" (class docstring)."""
        return f"MSE: {value:.6f}" if self.problem_type == "regression" else f"Label Accuracy: {value * 100:.2f}%"

    def _count(self, logits, tb, out, loss=None):
        """The epoch metrics of the new modes, on the device: multi-label adds the batch's element hits to the int32
        `out`, regression its squared-error sum (mean loss x elements; `loss`: the step's own, where there was one) to
        the fp32 `out`.  Returns the element count."""
        if self.problem_type == "regression":
            if loss is None:
                self.loss_fn.accumulate(logits, tb, self._batch_loss)
                loss = self._batch_loss
            out += loss * tb.numel()
        else:
            self.loss_fn.accumulate(logits, tb, self._batch_loss, out)
        return tb.numel()

    def _lr_options_active(self):
        return (self.lr_scheduler_type != "constant" or float(self.layer_decay) != 1.0 or not self.decay_bias_and_norm)

    def _schedule_for(self, epochs):
        """The LRSchedule of a train() call of `epochs` epochs (None: constant)."""
        if self.lr_scheduler_type == "constant":
            return None
        if self.lr_scheduler_type not in LRSchedule.KINDS:
            raise ValueError(f"lr_scheduler_type {self.lr_scheduler_type!r}: expected one of {LRSchedule.KINDS}")
        if epochs is None:
            raise ValueError(f"lr_scheduler_type {self.lr_scheduler_type!r} needs the number of epochs of the phase")
        k_acc = max(1, int(self.gradient_accumulation_steps))
        total = int(epochs) * -(-len(self.train_dataloader) // k_acc)
        if self.warmup_steps is not None:
            warmup = int(self.warmup_steps)
        else:
            if not 0.0 <= float(self.warmup_ratio) <= 1.0:
                raise ValueError(f"warmup_ratio {self.warmup_ratio!r} is outside [0, 1]")
            warmup = int(np.ceil(total * float(self.warmup_ratio)))
        return LRSchedule(self.lr_scheduler_type, warmup, total)

    def _apply_lr_options(self, lr, epochs):
        """Rebuild the optimiser's param groups from encoder_param_groups and attach the phase's schedule; the state is
        keyed by parameter and survives.  Back at the defaults after a phase with options: one group, no schedule, the
        one-launch-per-run step again."""
        opt = self.optimizer
        template = {k: v for k, v in opt.param_groups[0].items() if k not in ("params", "names", "layer_id", "lr_scale")}
        if not self._lr_options_active():
            if self._lr_options_applied:
                opt.param_groups = [dict(template, params=list(self.model.parameters()), lr=lr,
                                         weight_decay=self._weight_decay)]
                opt.set_schedule(None)
                opt.multi_tensor = False
                self._lr_options_applied = False
            return
        if not self._lr_options_applied:
            self._weight_decay = opt.param_groups[0]["weight_decay"]
        groups = encoder_param_groups(self.model, lr, self._weight_decay, self.layer_decay, self.decay_bias_and_norm)
        opt.param_groups = [dict(template, **g) for g in groups]
        opt.multi_tensor = True
        opt.set_schedule(self._schedule_for(epochs))
        self._lr_options_applied = True

    def _apply_weight_averaging(self):
        """Attach what the weight-averaging options describe (once: the step count and the averages carry over the
        phases; again when an option changed), or detach it."""
        opt = self.optimizer
        if self.weight_averaging is None:
            if opt.averaging is not None:
                opt.set_averaging(None)
                opt.multi_tensor = self._lr_options_applied
            return
        start = int(self.averaging_start_epoch)
        if start < 0:
            raise ValueError(f"averaging_start_epoch {self.averaging_start_epoch!r} must be >= 0")
        k_acc = max(1, int(self.gradient_accumulation_steps))
        steps_per_epoch = -(-len(self.train_dataloader) // k_acc)
        want = WeightAveraging(self.weight_averaging, self.ema_decay, self.ema_warmup,
                               start * steps_per_epoch + 1 if start else 0, self.averaging_every)
        if opt.averaging != want:
            opt.set_averaging(want)
        opt.multi_tensor = True

    def _averaged(self):
        """The context _evaluate and save_pretrained run in: the averaged weights swapped in, when there are any."""
        return self.optimizer.averaged_parameters() if self.optimizer.averaging is not None else contextlib.nullcontext()

    def _lr_text(self):
        """", lr x" for the epoch line under a non-constant schedule (one read-back per epoch), else ""."""
        if self.lr_scheduler_type == "constant" or self.optimizer.last_lr is None:
            return ""
        return f", lr {float(self.optimizer.last_lr.item()):.3e}"

    def _enter_phase(self, lr, freeze, epochs=None):
        lr = self.initial_lr if lr is None else lr
        for group in self.optimizer.param_groups:
            group['lr'] = lr
        if self._lr_options_active() or self._lr_options_applied:
            self._apply_lr_options(lr, epochs)
        if self.weight_averaging is not None or self.optimizer.averaging is not None:
            self._apply_weight_averaging()
        self.optimizer.max_grad_norm = self.max_grad_norm
        trainable_head = {id(p) for p in self.model.classifier.parameters()}
        for p in self.model.parameters():
            p.requires_grad = (not freeze) or (id(p) in trainable_head)
        if self.grad_sync is not None:       # frozen phase: only the head's gradients cross the xGMI links
            self.grad_sync.set_active(self.model.head_grad_ranges() if freeze else None)
        self._apply_regularisers(freeze)
        self._begin_phase_cache(freeze)
        return lr

    # Frozen-phase feature cache.  With `freeze=True` the backbone and its inputs are constant and every dropout of the
    # reference checkpoints is 0.0 (Pre_trained_models/ast-finetuned-audioset/config.json: hidden_dropout_prob 0.0,
    # attention_probs_dropout_prob 0.0; ViTConfig defaults the same), so the classifier's input of a given sample is the
    # same in every frozen epoch (Transformer_Audio.py:44-56, Transformer_Vision.py:61-77 re-run the whole backbone 10
    # times per subject).  The first frozen epoch of a train() call runs the backbone once per sample and keeps those
    # [N, hidden] features in HBM; the following epochs run only the head's forward / CE / backward / AdamW and the head on
    # the cached test features.  Same kernels on the same values: in "fp32" precision outputs, head weights and optimiser
    # state are bit-equal to the uncached run; in "split" precision the patch planes' scale depends on which samples share
    # a batch, so the two runs agree to rounding (~1e-6) instead.  `cache_frozen_features = False` restores the literal
    # schedule.  A trainer-level saving: it never enters bench.py's step metric.
    #
    # A checkpoint whose config sets hidden_dropout_prob or attention_probs_dropout_prob has no constant features: the
    # reference calls model.train() every epoch (Transformer_Audio.py:63), so HF drops inside the frozen backbone too.  The
    # cache is then bypassed - the frozen phase runs the backbone forward every step, in training mode - and one line says so.
    cache_frozen_features = True

    def _begin_phase_cache(self, freeze):
        self._feat_cache = None
        cfg = self.model.cfg
        if freeze and self.cache_frozen_features and self.grad_sync is None and (cfg.hidden_dropout > 0.0
                                                                                 or cfg.attention_dropout > 0.0):
            print(f"frozen-phase feature cache bypassed: the model drops (hidden {cfg.hidden_dropout:g}, attention "
                  f"{cfg.attention_dropout:g}), its features differ from step to step")
            return
        if freeze and self.cache_frozen_features and self.grad_sync is None:
            hid = self.model.cfg.hidden
            self._feat_cache = {"train": torch.empty(len(self.train_dataloader.dataset), hid, device=self.device),
                                "test": torch.empty(len(self.test_dataloader.dataset), hid, device=self.device),
                                "have_train": False, "have_test": False}

    def _train_one_epoch(self, after_batch=None):
        """Returns (#correct on device, #seen).  One optimiser step per batch; nothing is read back per step.
        Multi-label: (#element hits, #elements); regression: (squared-error sum, #elements).

        gradient_accumulation_steps = k > 1: the loader's batches are taken in groups of k consecutive micro-batches and
        ONE optimiser step is made per group.  Micro-batch j is folded into the optimiser's accumulator with weight
        len(batch j) / (samples of the group), so the update of a group is that of one batch holding the group's
        samples - the ragged last group included (a last group of one micro-batch has weight 1).  The weights count
        SAMPLES, not valid labels: with ignore_index (-100) labels each micro-batch's cross-entropy is the mean over its
        own valid rows, and the group's gradient then differs from torch's mean over the valid rows of one big batch.
        grad_sync() runs after every micro-batch's backward, before the fold (the all-reduce is linear).  Metrics, the
        frozen-phase feature cache and `after_batch` stay per micro-batch."""
        k_acc = int(self.gradient_accumulation_steps)
        if k_acc < 1:
            raise ValueError(f"gradient_accumulation_steps {self.gradient_accumulation_steps!r}: expected an integer >= 1")
        if k_acc > 1:
            return self._train_one_epoch_accumulating(k_acc, after_batch)
        self.model.train()
        classifies = self._classifies()
        correct = torch.zeros((), device=self.device, dtype=torch.long if classifies else
                              torch.float32 if self.problem_type == "regression" else torch.int32)
        self._batch_loss = torch.zeros((), dtype=torch.float32, device=self.device)
        dl = self.train_dataloader
        seen, nb = 0, len(dl)
        fc = getattr(self, "_feat_cache", None)
        batches = dl.index_batches()
        plan = self._epoch_plan(batches)
        for k, idx in enumerate(batches, start=1):
            self.optimizer.zero_grad()
            logits, tb, primary = self._train_batch(dl, idx, fc, plan)
            loss = self.loss_fn(logits, tb)
            loss.backward()
            if self.grad_sync is not None:
                self.grad_sync()
            self.optimizer.step()
            if classifies:
                correct += (logits.argmax(dim=-1) == primary).sum()
                seen += tb.size(0)
            else:
                seen += self._count(logits.detach(), tb, correct, loss.detach())
            if after_batch is not None:
                after_batch(k, nb)
        if fc is not None:
            fc["have_train"] = True
        self.loss_fn.check()            # labels outside [0, classes) seen by any step of this epoch raise here
        return correct, seen

    def _train_one_epoch_accumulating(self, k_acc, after_batch=None):
        """_train_one_epoch with one optimiser step per group of k_acc micro-batches (its docstring)."""
        self.model.train()
        classifies = self._classifies()
        correct = torch.zeros((), device=self.device, dtype=torch.long if classifies else
                              torch.float32 if self.problem_type == "regression" else torch.int32)
        self._batch_loss = torch.zeros((), dtype=torch.float32, device=self.device)
        dl = self.train_dataloader
        seen, nb = 0, len(dl)
        fc = getattr(self, "_feat_cache", None)
        batches = list(dl.index_batches())
        plan = self._epoch_plan(batches)        # partners come from the micro-batch, never from the rest of the group
        k = 0
        for first in range(0, len(batches), k_acc):
            group = batches[first:first + k_acc]
            total = sum(len(idx) for idx in group)
            for j, idx in enumerate(group):
                k += 1
                self.optimizer.zero_grad()
                logits, tb, primary = self._train_batch(dl, idx, fc, plan)
                loss = self.loss_fn(logits, tb)
                loss.backward()
                if self.grad_sync is not None:
                    self.grad_sync()
                self.optimizer.accumulate(len(idx) / total, last=j == len(group) - 1)
                if classifies:
                    correct += (logits.argmax(dim=-1) == primary).sum()
                    seen += tb.size(0)
                else:
                    seen += self._count(logits.detach(), tb, correct, loss.detach())
                if after_batch is not None:
                    after_batch(k, nb)
            self.optimizer.step()
        if fc is not None:
            fc["have_train"] = True
        self.loss_fn.check()
        return correct, seen

    def _index(self, idx):
        return torch.as_tensor(idx, dtype=torch.long, device=self.device)

    def _evaluate(self):
        """Test pass: list of (logits numpy [b, classes], #correct, b) per batch.  Logits and per-batch hit counts stay on
        the device until the pass is over - ONE device-to-host copy per epoch (the reference synchronises twice per
        batch: Transformer_Audio.py:91-96, Transformer_Vision.py:111-116).  Multi-label: (logits, #element hits,
        #elements); regression: (logits, squared-error sum, #elements)."""
        classifies = self._classifies()
        self.model.eval()
        dl = self.test_dataloader
        n, nb = len(dl.dataset), len(dl)
        fc = getattr(self, "_feat_cache", None)
        all_logits = torch.empty(n, self.model.cfg.num_labels, device=self.device)
        hits = torch.zeros(nb, device=self.device, dtype=torch.long if classifies else
                           torch.float32 if self.problem_type == "regression" else torch.int32)
        self._batch_loss = torch.zeros((), dtype=torch.float32, device=self.device)
        spans, pos = [], 0
        with self._averaged(), torch.no_grad():
            for k, idx in enumerate(dl.index_batches()):
                if fc is not None and fc["have_test"]:
                    tb = dl.gather_labels(idx)
                    logits = self.model.head(fc["test"][pos:pos + len(idx)]).logits
                else:
                    xb, tb = dl.gather(idx)
                    logits = self.model(xb).logits
                    if fc is not None:
                        fc["test"][pos:pos + len(idx)] = self.model.last_features()
                all_logits[pos:pos + len(idx)] = logits
                if classifies:
                    hits[k] = (logits.argmax(dim=-1) == tb).sum()
                    spans.append((pos, len(idx)))
                else:
                    spans.append((pos, len(idx), self._count(logits, tb, hits[k:k + 1])))
                pos += len(idx)
        if fc is not None:
            fc["have_test"] = True
        host_logits, host_hits = all_logits.cpu().numpy(), hits.cpu().tolist()      # the epoch's only read-back
        if not classifies:
            return [(host_logits[a:a + b], h, n) for (a, b, n), h in zip(spans, host_hits)]
        return [(host_logits[a:a + b], int(h), b) for (a, b), h in zip(spans, host_hits)]

    def _keep_outputs(self, rows, is_last_epoch, freeze):
        if is_last_epoch and not freeze:
            self.outputs_test = np.concatenate([r[0] for r in rows], axis=0)
