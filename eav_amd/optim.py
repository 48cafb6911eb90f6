"""Fused Adam / AdamW over flat parameter storage.  The criteria (cross-entropy, BCE-with-logits, MSE) live in
``eav_amd/criteria.py``; their public names are re-exported here, where they used to be.

Host-side mirrors of what the reference trainers construct:
  * ``optim.Adam(model.parameters(), lr)``            CNN_torch/EEGNet_tor.py:82
  * ``optim.AdamW(model.parameters(), lr)``           Transformer_Audio.py:30, Transformer_Vision.py:36
    (weight_decay is torch's default 0.01 - the trainer's ctor argument is ignored)

The arithmetic runs in libeav_hip.so (``eav_adam_step``).
Parameters that live in one flat buffer (``flatten_parameters``) are updated
with one launch per run of tensors that share a step count - the frozen and
unfrozen fine-tuning phases give the head and the backbone different counts
(SURVEY Q11), and tensors whose ``grad`` is None are skipped like torch does.

Training-loop options (csrc/grad_clip.hip): ``FusedAdam(max_grad_norm=...)`` clips by the global L2 norm inside the
step, ``FusedAdam.accumulate()`` folds the gradients of several backward passes into an accumulator the next step
consumes, and ``clip_grad_norm_`` is torch's free function on the same kernels.  Nothing of it reads a value back.

Learning-rate options (csrc/adam_jobs.hip): ``FusedAdam(multi_tensor=True)`` updates every tensor of every param group -
each with its own ``lr`` / ``weight_decay`` and step count - in two launches over a device job table, and
``FusedAdam.set_schedule(LRSchedule(...))`` scales the rates by ``transformers.get_scheduler``'s factors, evaluated on the
device from a device-resident step count.  Off by default: the default step launches what it always did.

Weight averaging (csrc/adam_jobs.hip): ``FusedAdam.set_averaging(WeightAveraging("ema" | "swa", ...))`` keeps an
exponential or equal-weight average of every parameter, updated inside the multi-tensor step's own two launches from the
parameter the step has in registers; ``averaged_parameters()`` swaps the averages in for evaluation.
"""
from __future__ import annotations

import contextlib
from operator import itemgetter

import torch

from . import _lib
from .criteria import (BCEWithLogitsLoss, CrossEntropyLoss, HEAD_NARROW_CLASSES, MSELoss,  # noqa: F401 - the old import path
                       head_is_wide, unit_gradient)


def flatten_parameters(module: torch.nn.Module, order=None, pad_after=None):
    """Re-home every parameter of ``module`` as a view of one flat fp32 device
    buffer (and allocate a same-shaped flat gradient buffer).  Parameter objects
    are preserved, so optimisers created earlier stay valid.  Returns
    (flat_param, flat_grad, {name: (offset, numel)}).

    pad_after: {name: n} leaves n zero floats after that tensor in every flat buffer (e.g. to lay a [40,40] weight out
    as the first rows of a zero-padded [64,40] GEMM operand); the padding stays zero under FusedAdam."""
    params = [(n, p) for n, p in module.named_parameters()]
    if order is not None:  # explicit flat layout (e.g. q/k/v weights adjacent for one fused GEMM)
        named = dict(params)
        assert sorted(named) == sorted(order), "order must name every parameter exactly once"
        params = [(n, named[n]) for n in order]
    if not params:
        raise ValueError("module has no parameters")
    dev = params[0][1].device
    offsets, total = {}, 0
    for n, p in params:
        if p.dtype != torch.float32:
            raise TypeError(f"{n}: only fp32 parameters are supported")
        offsets[n] = (total, p.numel())
        total += (p.numel() + 3) // 4 * 4  # keep every tensor 16-byte aligned
        if pad_after and n in pad_after:
            assert pad_after[n] % 4 == 0
            total += pad_after[n]
            p._eav_pad = pad_after[n]
    flat = torch.zeros(total, dtype=torch.float32, device=dev)
    gflat = torch.zeros(total, dtype=torch.float32, device=dev)
    for n, p in params:
        off, num = offsets[n]
        view = flat[off:off + num].view(p.shape)
        view.copy_(p.data)
        p.data = view
        p._eav_flat = (flat, gflat, off)
    return flat, gflat, offsets


# A row: a run of fp32 elements that lies at the same place in several buffers, as a list of plain integers
#   [ptr, rel, numel, slack, key]
# ptr: its address in the first buffer; rel: tuple of the byte distances from there to the same run in the other buffers
# ((acc - g,), (0,) or (g - p, m - p, v - p)); slack: bytes - the next row may begin less than this after the end of this
# one and still join it; key: what joined rows must share (step count, lr, weight decay; None: nothing).
_PTR, _REL, _NUMEL, _SLACK, _KEY = range(5)


def _merge_rows(rows):
    """The one rule for "merge what is adjacent".  `rows` are taken in address order of `ptr` (a stable sort); a row joins
    its predecessor where it begins less than the predecessor's `slack` bytes after its end (never before it), lies at
    the same distances in the other buffers (equal `rel`) and the keys are equal.  The slack covers what lies between two
    tensors and holds zeros in every buffer - flat buffers: the 16-byte alignment padding plus declared zero padding
    (`_flat_slack`); loose tensors: slack 1, i.e. exactly adjacent.  The joined row spans both and takes the slack of the
    row that joined.  Rows are lists and are joined in place - this runs once per tensor in every optimiser step."""
    merged = []
    for r in sorted(rows, key=itemgetter(_PTR)):
        if merged:
            q = merged[-1]
            gap = r[_PTR] - (q[_PTR] + 4 * q[_NUMEL])
            if 0 <= gap < q[_SLACK] and r[_KEY] == q[_KEY] and r[_REL] == q[_REL]:
                q[_NUMEL] = (r[_PTR] - q[_PTR]) // 4 + r[_NUMEL]
                q[_SLACK] = r[_SLACK]
                continue
        merged.append(r)
    return merged


class _JobTables:
    """Device job tables ({pointer, element count} rows, include/eav_hip.h) and their fp64 partials, cached by the ranges
    they describe: a steady-state step finds its tables here and neither allocates nor copies anything to the device."""

    def __init__(self, limit=16):
        self._cache, self._limit = {}, limit

    def get(self, device, ranges):
        """ranges: tuple of (ptr, other_ptr, numel).  Returns (table of ptr, table of other_ptr, njobs, nchunks, partials)."""
        key = (device, ranges)
        hit = self._cache.get(key)
        if hit is None:
            nchunks = sum(int(_lib.plain("eav_grad_nchunks", r[2])) for r in ranges)
            if len(self._cache) >= self._limit:
                self._cache.clear()
            hit = (torch.tensor([[r[0], r[2]] for r in ranges], dtype=torch.int64).to(device),
                   torch.tensor([[r[1], r[2]] for r in ranges], dtype=torch.int64).to(device),
                   len(ranges), nchunks, torch.empty(max(nchunks, 1), dtype=torch.float64, device=device))
            self._cache[key] = hit
        return hit


def _flat_slack(p):
    return 16 + 4 * getattr(p, "_eav_pad", 0) if getattr(p, "_eav_flat", None) is not None else 1


class LRSchedule:
    """The learning-rate multiplier of ``transformers.get_scheduler(kind, ...)`` for ``kind`` in ``KINDS``: warmup from 0
    over ``num_warmup_steps`` optimiser steps, then constant, linear decay to 0 at ``num_training_steps``, or cosine decay
    (``num_cycles`` = 0.5: half a wave, down to 0 at ``num_training_steps``).  ``t`` counts the optimiser steps completed
    since the schedule was attached (``FusedAdam.set_schedule``), so the first step runs at ``factor(0)`` - 0 when there
    is a warmup, exactly as ``LambdaLR`` behaves.  ``factor`` is the host float64 version, for printing and for tests;
    the optimiser evaluates the same expressions on the device (csrc/adam_jobs.hip), from a device-resident ``t``."""

    KINDS = ("constant", "constant_with_warmup", "linear", "cosine")

    def __init__(self, kind, num_warmup_steps=0, num_training_steps=None, num_cycles=0.5):
        if kind not in self.KINDS:
            raise ValueError(f"LRSchedule: kind {kind!r}: expected one of {self.KINDS}")
        if int(num_warmup_steps) != num_warmup_steps or num_warmup_steps < 0:
            raise ValueError(f"LRSchedule: num_warmup_steps {num_warmup_steps!r} must be an integer >= 0")
        if kind in ("linear", "cosine"):
            if num_training_steps is None or int(num_training_steps) != num_training_steps or num_training_steps < 0:
                raise ValueError(f"LRSchedule: kind {kind!r} needs num_training_steps, an integer >= 0, "
                                 f"got {num_training_steps!r}")
        self.kind = kind
        self.num_warmup_steps = int(num_warmup_steps) if kind != "constant" else 0
        self.num_training_steps = 0 if num_training_steps is None else int(num_training_steps)
        self.num_cycles = float(num_cycles)

    @property
    def code(self):
        """The kind as include/eav_hip.h numbers it (EAV_SCHED_*)."""
        return self.KINDS.index(self.kind)

    def factor(self, t):
        import math
        t, W, T = int(t), self.num_warmup_steps, self.num_training_steps
        if self.kind == "constant":
            return 1.0
        if t < W:
            return float(t) / float(max(1, W))
        if self.kind == "constant_with_warmup":
            return 1.0
        if self.kind == "linear":
            return max(0.0, float(T - t) / float(max(1, T - W)))
        progress = float(t - W) / float(max(1, T - W))
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * self.num_cycles * 2.0 * progress)))

    def __repr__(self):
        return (f"LRSchedule({self.kind!r}, num_warmup_steps={self.num_warmup_steps}, "
                f"num_training_steps={self.num_training_steps}, num_cycles={self.num_cycles})")


_CONSTANT = LRSchedule("constant")


class WeightAveraging:
    """What ``FusedAdam.set_averaging`` attaches: an average of the weights kept beside them, updated by the optimiser
    step itself.  ``s`` counts the optimiser steps since it was attached, from 1; step ``s`` is an averaging step when
    ``s >= start_step`` and ``(s - start_step) % every == 0``.  The first averaging step copies the parameters
    (``torch.optim.swa_utils.AveragedModel.update_parameters``' first call); every later one does
    ``avg += c * (p - avg)`` with

      kind "ema":  c = 1 - decay (``get_ema_multi_avg_fn(decay)``); ``warmup=True`` uses min(decay, (1 + n) / (10 + n))
                   in place of decay (timm's ModelEmaV2 / tf.train.ExponentialMovingAverage warm-up),
      kind "swa":  c = 1 / (n + 1) (``get_swa_multi_avg_fn()``): the equal-weight mean of the averaged iterates,

    n = ``n_averaged``, the averaging steps so far.  ``mode_and_coefficient`` is the host float64 version, for tests and
    printing; the optimiser evaluates the same expressions on the device from device-resident ``s`` and ``n``.
    Parameters only: buffers (BatchNorm running statistics) are not averaged."""

    KINDS = _lib.AVG_KINDS

    def __init__(self, kind="ema", decay=0.999, warmup=False, start_step=0, every=1):
        if kind not in self.KINDS:
            raise ValueError(f"WeightAveraging: kind {kind!r}: expected one of {self.KINDS}")
        if not 0.0 <= float(decay) <= 1.0:
            raise ValueError(f"WeightAveraging: decay {decay!r} is outside [0, 1]")
        if int(start_step) != start_step or start_step < 0:
            raise ValueError(f"WeightAveraging: start_step {start_step!r} must be an integer >= 0")
        if int(every) != every or every < 1:
            raise ValueError(f"WeightAveraging: every {every!r} must be an integer >= 1")
        self.kind, self.decay, self.warmup = kind, float(decay), bool(warmup)
        self.start_step, self.every = int(start_step), int(every)

    @property
    def code(self):
        """The kind as include/eav_hip.h numbers it (EAV_AVG_EMA / EAV_AVG_SWA)."""
        return self.KINDS.index(self.kind)

    def as_dict(self):
        return dict(kind=self.kind, decay=self.decay, warmup=self.warmup, start_step=self.start_step, every=self.every)

    def mode_and_coefficient(self, s, n):
        """("skip" | "copy" | "lerp", c as a float64) of step ``s`` (from 1) when ``n`` steps have been averaged."""
        if s < self.start_step or (s - self.start_step) % self.every:
            return "skip", 0.0
        if n == 0:
            return "copy", 1.0
        if self.kind == "swa":
            return "lerp", 1.0 / (float(n) + 1.0)
        d = min(self.decay, (1.0 + float(n)) / (10.0 + float(n))) if self.warmup else self.decay
        return "lerp", 1.0 - d

    def __eq__(self, other):
        return isinstance(other, WeightAveraging) and self.as_dict() == other.as_dict()

    __hash__ = None

    def __repr__(self):
        return (f"WeightAveraging({self.kind!r}, decay={self.decay}, warmup={self.warmup}, start_step={self.start_step}, "
                f"every={self.every})")


class _AdamJobTable:
    """One cached table of eav_adam_step_jobs (rows: include/eav_hip.h) with the device step counts its rows read."""

    def __init__(self, device, jobs, shared_step_ptr):
        """jobs: rows over (p, g, m, v) - and the average, under FusedAdam.set_averaging - with key (step, lr, weight decay)."""
        words = _lib.JOB_WORDS
        n = len(jobs)
        self.njobs = n
        self.nchunks = sum(int(_lib.plain("eav_adam_jobs_nchunks", r[_NUMEL])) for r in jobs)
        self.per_tensor = shared_step_ptr is None
        # the counts hold the steps COMPLETED: eav_adam_jobs_begin advances them before it reads them
        self.steps = [step - 1 for _, _, _, _, (step, _, _) in jobs]       # host mirror: the step each job ran last
        self.counts = torch.tensor(self.steps, dtype=torch.int64).to(device) if self.per_tensor else None
        rows = torch.zeros(n, words, dtype=torch.int64)
        rows[:, :5] = torch.tensor([[p, p + rel[0], p + rel[1], p + rel[2], numel] for p, rel, numel, _, _ in jobs],
                                   dtype=torch.int64)
        # the averages' addresses, a parallel array (eav_adam_step_jobs_avg); None without averaging
        self.avgs = (torch.tensor([p + rel[3] for p, rel, _, _, _ in jobs], dtype=torch.int64).to(device)
                     if len(jobs[0][_REL]) == 4 else None)
        rows[:, 5] = torch.tensor([lr for _, _, _, _, (_, lr, _) in jobs], dtype=torch.float64).view(torch.int64)
        if self.per_tensor:
            rows[:, 6] = self.counts.data_ptr() + 8 * torch.arange(n, dtype=torch.int64)
        else:
            rows[:, 6] = shared_step_ptr
        rows[:, 7] = (torch.tensor([wd for _, _, _, _, (_, _, wd) in jobs], dtype=torch.float32).view(torch.int32)
                      .to(torch.int64) & 0xffffffff)
        self.rows = rows.to(device)

    def sync_counts(self, steps):
        """`steps`: the step each job is about to run.  Re-seeds the device counts when they are not one behind (another
        table advanced these tensors in between, or the state was loaded)."""
        if self.per_tensor and [s - 1 for s in steps] != self.steps:
            self.counts.copy_(torch.tensor([s - 1 for s in steps], dtype=torch.int64))
        self.steps = list(steps)


class FusedAdam(torch.optim.Optimizer):
    """Adam (``decoupled=False``) / AdamW (``decoupled=True``) with torch's
    hyper-parameter names; one ``eav_adam_step`` launch per contiguous run.

    ``max_grad_norm`` (attribute, may be changed between steps; None: off) clips by the global L2 norm like
    ``torch.nn.utils.clip_grad_norm_(params, max_grad_norm)`` before the update: step() forms the norm over exactly the
    gradients it is about to consume - parameters whose ``grad`` is None are left out - in two extra launches however
    many tensors there are (``eav_grad_sumsq``, ``eav_grad_clip_finish``), and the update launches become
    ``eav_adam_step_scaled`` with the device-resident coefficient min(1, max_grad_norm / (norm + 1e-6)).  ``p.grad``
    ITSELF IS LEFT UNSCALED (torch's function scales it in place; the free function ``clip_grad_norm_`` below does that).
    ``last_grad_norm`` is the 0-dim device tensor holding the norm before clipping, overwritten by every such step and
    never read back by the library; ``float("inf")`` measures the norm and clips nothing.  Nothing needs a host value,
    so a capturable optimiser's step() is captured with its clipping.

    ``accumulate(weight)`` folds the current gradients into an accumulator (the models' backward OVERWRITES the flat
    gradient buffer, so torch's idiom of several backward() calls before one step() cannot work here); the next step()
    consumes the accumulator instead of ``p.grad``.

    ``multi_tensor=True`` (keyword-only, like ``max_grad_norm`` now) updates every tensor in TWO launches whatever the
    param groups look like (csrc/adam_jobs.hip): step() builds one job per parameter tensor that has a gradient -
    adjacent tensors with equal ``lr``, ``weight_decay`` and step count merged as on the default path, ACROSS groups -
    and issues ``eav_adam_jobs_begin`` (step counts, schedule factor, each job's lr and bias corrections, all on the
    device) and ``eav_adam_step_jobs``.  Per-group ``lr`` and ``weight_decay`` are honoured; ``betas``, ``eps`` and
    ``decoupled`` must be equal across the groups (EavError otherwise).  The per-tensor step counts live in a device
    int64 array seeded from ``state[p]["step"]`` whenever a table is built - head and backbone keep their own counts
    through the frozen / unfrozen phases - and the host mirror is still advanced, so ``state_dict()``
    keeps torch's shape; with ``capturable=True`` every job reads the one device count.  The table is cached by what it
    describes - pointers, sizes AND each job's ``lr`` and ``weight_decay``: changing ``group["lr"]`` or
    ``group["weight_decay"]`` between steps is picked up because it is part of the cache key (a new table is built, the
    old one stays cached for when the values return); a steady-state step allocates and copies nothing.
    ``max_grad_norm`` and ``accumulate()`` work as on the default path, and the element update is the same function
    (``adam_update``, csrc/eav_common.h): the same bits as ``eav_adam_step`` with a device step count gives.

    ``set_schedule(LRSchedule(...))`` multiplies every group's ``lr`` by a factor evaluated ON THE DEVICE from a
    device-resident count of the steps completed since the call; ``group["lr"]`` stays the base rate and nothing mutates
    it per step, so a captured step() follows the schedule on every replay.  It needs - and turns on - ``multi_tensor``.
    ``last_lr`` is the 0-dim device tensor holding group 0's rate in the last step, ``(float)(lr * factor)``, never read
    back by the library.  Tables and the schedule record are created by the first step:
    run one step eagerly before capturing, and capture again after ``set_schedule``.

    ``set_averaging(WeightAveraging(...))`` keeps an EMA or SWA average of EVERY parameter of the optimiser
    (``state[p]["avg"]``, present only while averaging is on; a copy of the parameter when attached; views of one flat
    buffer laid out like the moments for a flat model, so jobs merge as before).  It needs - and turns on -
    ``multi_tensor``; the step stays two launches, ``eav_adam_jobs_begin_avg`` and ``eav_adam_step_jobs_avg``: the count
    of steps, ``n_averaged`` and the coefficient live in a device record, the average is formed from the parameter the
    step holds in registers, and ``p``, ``exp_avg`` and ``exp_avg_sq`` get the bits they get without averaging.  It works
    with ``max_grad_norm``, ``accumulate()``, a schedule and ``capturable=True`` - a captured step averages on every
    replay; as for ``set_schedule``, run one step eagerly before capturing and capture again after ``set_averaging``.  A
    tensor the step skips (``grad`` None, the frozen phase) keeps its average: it equals the parameter until the tensor
    first trains, as ``AveragedModel`` over the whole model averages a constant parameter to itself.  (A tensor that
    trained before ``start_step`` and has no gradient in the first averaging step keeps its copy from attach time.)
    Buffers are not averaged.  ``n_averaged`` is the 0-dim device int64 tensor of the record, never read back by the
    library.  ``with optimizer.averaged_parameters():`` swaps the averages into the parameters (one ``eav_swap_jobs``
    launch each way, the swapped ranges recorded like a step's, so an Encoder refreshes its operand planes); it refuses
    to nest and refuses a step() inside.  ``state_dict()`` gains an ``"averaging"`` entry (the options, ``s`` and ``n`` -
    read back there and only there) and ``load_state_dict`` restores it with the averages; with averaging off both have
    the shape they always had."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False,
                 capturable=False, *, multi_tensor=False, max_grad_norm=None):
        """capturable=True keeps ONE step count in device memory (incremented by a kernel), so that step()
        can be captured in a hipGraph and replayed; it requires every parameter to receive a gradient on
        every step (true for EEGNet; the two-phase AST/ViT fine-tune uses the default host-side counts)."""
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled=decoupled)
        super().__init__(params, defaults)
        self._flat_state = {}
        self.capturable = capturable
        self.multi_tensor = bool(multi_tensor)
        self.schedule = None
        self.last_lr = None
        self._sched = None              # device schedule record (include/eav_hip.h)
        self._adam_tables = {}          # _AdamJobTable by (device, jobs)
        self.averaging = None           # WeightAveraging (set_averaging)
        self._avg_rec = None            # device averaging record (include/eav_hip.h)
        self._avg_flat = {}             # flat average buffers by the flat parameter buffer's address
        self._swap_tables = {}          # (rows, avgs, njobs, nchunks, ranges, flats) of averaged_parameters, by its ranges
        self._swapped = False           # inside averaged_parameters()
        self._dev_step = None
        # capturable: set by a caller that increments the device step count itself at the start of the step, in a launch
        # it issues anyway (GraphStep: eav_step_begin) - step() then skips its own eav_counter_inc for that one call
        self.step_counted = False
        self.max_grad_norm = max_grad_norm
        self.last_grad_norm = None
        self._tables = _JobTables()
        self._norm_out = None           # device [norm, coefficient]
        self._weights = {}              # fold weights as device scalars, by value
        self._acc_flat, self._acc_loose = {}, {}
        self._acc_key, self._acc_folds, self._acc_tables, self._acc_partials = None, 0, None, False

    def _launch(self, p_ptr, g_ptr, m_ptr, v_ptr, n, group, step, gscale=None):
        b1, b2 = group["betas"]
        args = (p_ptr, g_ptr, m_ptr, v_ptr, n, float(group["lr"]), float(b1), float(b2),
                float(group["eps"]), float(group["weight_decay"]), int(step), int(bool(group["decoupled"])),
                None if self._dev_step is None else self._dev_step.data_ptr())
        if gscale is None:
            _lib.call("eav_adam_step", *args, _lib.stream_ptr())
        else:
            _lib.call("eav_adam_step_scaled", *args, gscale, _lib.stream_ptr())

    # ---- gradient accumulation ------------------------------------------------------------------------------------
    def _checked_grad(self, p):
        """p.grad as step() and accumulate() consume it: on the device, contiguous, and - for a parameter of a flat model -
        the model's own view of its flat gradient buffer."""
        g = p.grad
        if not p.is_cuda:
            raise _lib.EavError("FusedAdam needs parameters on a ROCm device (no CPU fallback)")
        if not g.is_contiguous():
            g = g.contiguous()
        fl = getattr(p, "_eav_flat", None)
        if fl is not None and g.data_ptr() != fl[1].data_ptr() + 4 * fl[2]:
            # the models return views of their flat gradient buffer, which each backward OVERWRITES; autograd
            # adopts the view only when p.grad was None - anything else means torch accumulated into a copy
            # (zero_grad(set_to_none=False), or two backward() calls before one step)
            raise _lib.EavError("FusedAdam: p.grad is not the model's flat gradient buffer - use "
                                "optimizer.zero_grad() (set_to_none=True) and one backward() per step; gradient "
                                "accumulation across backward() calls is not supported (call optimizer.accumulate() "
                                "after each backward() instead)")
        return g

    def accumulated_grad(self, p):
        """p's view of the accumulator (None before the first accumulate() that saw p with a gradient)."""
        fl = getattr(p, "_eav_flat", None)
        if fl is not None:
            acc = self._acc_flat.get(fl[1].data_ptr())
            return None if acc is None else acc[fl[2]:fl[2] + p.numel()].view(p.shape)
        return self._acc_loose.get(p)

    def _weight_scalar(self, weight, device):
        key = (float(weight), device)
        if key not in self._weights:
            if len(self._weights) >= 64:
                self._weights.clear()
            self._weights[key] = torch.tensor(float(weight), dtype=torch.float32).to(device)
        return self._weights[key]

    @torch.no_grad()
    def accumulate(self, weight=1.0, last=False):
        """acc = weight * grad (first fold since the last step(): the accumulator's old contents are not read) or
        acc += weight * grad, over every parameter that has a gradient, in one ``eav_grad_fold`` launch.  The next step()
        updates from the accumulator and empties it.  With weights len(micro-batch) / len(group) the update is that of
        one batch holding the group's samples.  last=True on the final fold of a group lets that launch produce the
        sum-of-squares partials ``max_grad_norm`` needs; without it step() runs ``eav_grad_sumsq`` over the accumulator
        (same bits).  The set of parameters with a gradient must not change inside a group."""
        if self.capturable:
            raise _lib.EavError("FusedAdam(capturable=True).accumulate(): a captured step holds one whole optimiser step - "
                                "gradient accumulation inside a graph is not supported; build the optimiser with "
                                "capturable=False to accumulate")
        ps = [p for group in self.param_groups for p in group["params"] if p.grad is not None]
        if not ps:
            raise _lib.EavError("FusedAdam.accumulate(): no parameter has a gradient")
        key = tuple(id(p) for p in ps)
        if self._acc_folds and key != self._acc_key:
            raise _lib.EavError("FusedAdam.accumulate(): the parameters with a gradient differ from those already in the "
                                "accumulator (requires_grad changed inside an accumulation group?) - step() first")
        ranges = []
        for p in ps:
            g = self._checked_grad(p)
            fl = getattr(p, "_eav_flat", None)
            if fl is not None:
                if fl[1].data_ptr() not in self._acc_flat:
                    self._acc_flat[fl[1].data_ptr()] = torch.zeros_like(fl[1])
            elif p not in self._acc_loose:
                self._acc_loose[p] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            at = g.data_ptr()
            ranges.append([at, (self.accumulated_grad(p).data_ptr() - at,), p.numel(), _flat_slack(p), None])
        dev = ps[0].device
        tables = self._tables.get(dev, tuple((at, at + acc, numel) for at, (acc,), numel, _, _ in _merge_rows(ranges)))
        jobs_g, jobs_a, njobs, nchunks, partials = tables
        want = bool(last) and self.max_grad_norm is not None
        _lib.call("eav_grad_fold", jobs_g.data_ptr(), jobs_a.data_ptr(), njobs, nchunks,
                  self._weight_scalar(weight, dev).data_ptr(), int(self._acc_folds == 0),
                  partials.data_ptr() if want else None, _lib.stream_ptr())
        self._acc_key, self._acc_tables, self._acc_partials = key, tables, want
        self._acc_folds += 1

    def _clip(self, device, tables, have_partials):
        """The norm of the ranges of `tables` and the clipping coefficient, on the device; returns the coefficient's pointer."""
        _, jobs, njobs, nchunks, partials = tables
        if self._norm_out is None or self._norm_out.device != device:
            self._norm_out = torch.zeros(2, dtype=torch.float32, device=device)
            self.last_grad_norm = self._norm_out[0]
        if not have_partials:
            _lib.call("eav_grad_sumsq", jobs.data_ptr(), njobs, nchunks, partials.data_ptr(), _lib.stream_ptr())
        _lib.call("eav_grad_clip_finish", partials.data_ptr(), nchunks, float(self.max_grad_norm),
                  self._norm_out.data_ptr(), _lib.stream_ptr())
        return self._norm_out.data_ptr() + 4

    def device_step_counter(self):
        """The device-resident step count of a capturable optimiser (created on first use)."""
        if not self.capturable:
            return None
        if self._dev_step is None:
            dev = next(p for g in self.param_groups for p in g["params"]).device
            self._dev_step = torch.zeros((), dtype=torch.int64, device=dev)
        return self._dev_step

    def set_schedule(self, schedule):
        """Attach an LRSchedule (None: detach - the base rates apply again) and restart its step count at 0.  Turns
        ``multi_tensor`` on; a captured step() must be captured again afterwards."""
        if schedule is not None and not isinstance(schedule, LRSchedule):
            raise TypeError(f"FusedAdam.set_schedule: expected an LRSchedule or None, got {type(schedule).__name__}")
        self.schedule = schedule
        if schedule is not None:
            self.multi_tensor = True
        if self._sched is not None:
            self._sched[0].zero_()

    # ---- weight averaging ------------------------------------------------------------------------------------------
    def set_averaging(self, averaging):
        """Attach a WeightAveraging (None: detach and drop the averages): every parameter gets ``state[p]["avg"]``, a copy
        of it, and the step count ``s`` and ``n_averaged`` restart at 0.  Turns ``multi_tensor`` on; a captured step()
        must be captured again afterwards."""
        if averaging is not None and not isinstance(averaging, WeightAveraging):
            raise TypeError(f"FusedAdam.set_averaging: expected a WeightAveraging or None, got {type(averaging).__name__}")
        if self._swapped:
            raise _lib.EavError("FusedAdam.set_averaging() inside averaged_parameters(): leave the block first")
        params = [p for group in self.param_groups for p in group["params"]]
        if averaging is not None and not all(p.is_cuda for p in params):
            raise _lib.EavError("FusedAdam.set_averaging needs parameters on a ROCm device (no CPU fallback)")
        for p in params:
            if p in self.state:
                self.state[p].pop("avg", None)
        self.averaging, self._avg_rec, self._avg_flat, self._swap_tables = averaging, None, {}, {}
        if averaging is None:
            return
        self.multi_tensor = True
        self._avg_rec = torch.zeros(_lib.AVG_WORDS, dtype=torch.int64, device=params[0].device)
        with torch.no_grad():
            for p in params:
                fl = getattr(p, "_eav_flat", None)
                if fl is not None and fl[0].data_ptr() + 4 * fl[2] == p.data_ptr():
                    buf = self._avg_flat.get(fl[0].data_ptr())
                    if buf is None:
                        buf = self._avg_flat[fl[0].data_ptr()] = fl[0].clone()
                    self.state[p]["avg"] = buf[fl[2]:fl[2] + p.numel()].view(p.shape)
                else:
                    self.state[p]["avg"] = p.detach().clone(memory_format=torch.contiguous_format)

    @property
    def n_averaged(self):
        """The averaging steps so far: a 0-dim device int64 tensor (None while averaging is off)."""
        return None if self._avg_rec is None else self._avg_rec[1]

    def _swap(self):
        """p <-> avg over every parameter in one eav_swap_jobs launch; the ranges are recorded as a step records them."""
        rows, touched = [], {}
        for group in self.param_groups:
            for p in group["params"]:
                fl = getattr(p, "_eav_flat", None)
                if fl is not None:
                    touched[fl[0].data_ptr()] = fl[0]
                at = p.data_ptr()
                rows.append([at, (self.state[p]["avg"].data_ptr() - at,), p.numel(), _flat_slack(p), None])
        jobs = _merge_rows(rows)
        key = tuple((at, a, numel) for at, (a,), numel, _, _ in jobs)
        table = self._swap_tables.get(key)
        if table is None:
            self._swap_tables.clear()
            dev = self._avg_rec.device
            t = torch.zeros(len(jobs), _lib.JOB_WORDS, dtype=torch.int64)
            t[:, 0] = torch.tensor([at for at, _, _ in key], dtype=torch.int64)
            t[:, 4] = torch.tensor([numel for _, _, numel in key], dtype=torch.int64)
            table = self._swap_tables[key] = (
                t.to(dev), torch.tensor([at + a for at, a, _ in key], dtype=torch.int64).to(dev), len(jobs),
                sum(int(_lib.plain("eav_adam_jobs_nchunks", numel)) for _, _, numel in key))
        _lib.call("eav_swap_jobs", table[0].data_ptr(), table[1].data_ptr(), table[2], table[3], _lib.stream_ptr())
        self._record_dirty(touched, jobs)

    @contextlib.contextmanager
    def averaged_parameters(self):
        """Inside the block the parameters hold the averages (and ``state[p]["avg"]`` the last iterate); on exit they are
        swapped back, bit for bit.  For evaluating or saving the averaged model."""
        if self.averaging is None:
            raise _lib.EavError("FusedAdam.averaged_parameters(): averaging is off - call set_averaging first")
        if self._swapped:
            raise _lib.EavError("FusedAdam.averaged_parameters() does not nest: the parameters already hold the averages")
        self._swap()
        self._swapped = True
        try:
            yield self
        finally:
            self._swapped = False
            self._swap()

    def state_dict(self):
        sd = super().state_dict()
        if self.averaging is not None:
            rec = self._avg_rec.cpu()
            sd["averaging"] = dict(self.averaging.as_dict(), s=int(rec[0]), n=int(rec[1]))
        return sd

    def load_state_dict(self, state_dict):
        cfg = state_dict.get("averaging")
        super().load_state_dict({k: v for k, v in state_dict.items() if k != "averaging"})
        params = [p for group in self.param_groups for p in group["params"]]
        loaded = {p: self.state[p].pop("avg") for p in params if p in self.state and "avg" in self.state[p]}
        if cfg is None:
            self.set_averaging(None)
            return
        cfg = dict(cfg)
        s, n = cfg.pop("s"), cfg.pop("n")
        self.set_averaging(WeightAveraging(**cfg))
        with torch.no_grad():
            for p, avg in loaded.items():
                self.state[p]["avg"].copy_(avg.view(p.shape))
            self._avg_rec[:2].copy_(torch.tensor([s, n], dtype=torch.int64))

    # ---- what the two step paths share ----------------------------------------------------------------------------
    def _gather(self):
        """The walk over the parameters that both paths begin with.  Each tensor is updated from its view of the
        accumulator when accumulate() was called since the last step, else from ``p.grad`` as _checked_grad passes it;
        a tensor without a gradient is skipped like torch does (a capturable optimiser refuses it).  State is created on
        first sight and the host step count advanced.  Returns ([(group, rows)] with one row (_merge_rows) over
        (p, g, m, v) per tensor, keyed by its host step count; the flat parameter buffers these tensors live in, by
        address; the device of the gradients - None when there is nothing to update)."""
        folded = set(self._acc_key) if self._acc_folds else None      # accumulate() was called: consume the accumulator
        plan, touched, dev, flat = [], {}, None, None
        averaging = self.averaging is not None
        for group in self.param_groups:
            rows = []
            for p in group["params"]:
                if folded is not None:
                    if id(p) not in folded:
                        continue
                    g = self.accumulated_grad(p)
                elif p.grad is None:
                    if self.capturable:
                        raise _lib.EavError("FusedAdam(capturable=True): every parameter must have a gradient")
                    continue
                else:
                    g = self._checked_grad(p)
                st = self.state[p]
                fl = getattr(p, "_eav_flat", None)
                if fl is not None and fl[0] is not flat:        # (neighbours share their buffer: one entry, one look)
                    flat = fl[0]
                    touched[flat.data_ptr()] = flat
                if "step" not in st:        # (under set_averaging a fresh state already holds "avg")
                    self._init_state(p, st)
                st["step"] += 1
                if dev is None:
                    dev = g.device
                # adjacent in all four buffers up to the 16-byte alignment padding plus declared zero padding, whose
                # gradient and moments are zero, so the update leaves it zero
                at = p.data_ptr()
                rel = (g.data_ptr() - at, st["exp_avg"].data_ptr() - at, st["exp_avg_sq"].data_ptr() - at)
                if averaging:               # a fifth buffer that joined rows must be adjacent in
                    if "avg" not in st:
                        raise _lib.EavError("FusedAdam: a parameter without an average (added after set_averaging?) - "
                                            "call set_averaging again")
                    rel += (st["avg"].data_ptr() - at,)
                rows.append([at, rel, p.numel(), 16 + 4 * getattr(p, "_eav_pad", 0), st["step"]])
            plan.append((group, rows))
        return plan, touched, dev

    def _acc_reset(self):
        """The accumulator is consumed (or there was nothing to consume): the next accumulate() starts a new group."""
        self._acc_folds, self._acc_partials = 0, False

    def _grad_scale(self, dev, runs):
        """The clipping coefficient's device pointer for a step over `runs` (None: no clipping), from the accumulator's own
        table when the step consumes it - the partials of a last=True fold belong to that table - else from a table over
        the gradient ranges of `runs`, in their order.  Empties the accumulator either way."""
        gscale = None
        if self.max_grad_norm is not None and runs:
            if self._acc_folds:
                gscale = self._clip(dev, self._acc_tables, self._acc_partials)
            else:
                ranges = tuple((at + rel[0], at + rel[0], numel) for at, rel, numel, _, _ in runs)
                gscale = self._clip(dev, self._tables.get(dev, ranges), False)
        self._acc_reset()
        return gscale

    @staticmethod
    def _record_dirty(touched, runs):
        """Tell whoever caches derived copies of these parameters (transformer.Encoder's fp16 operand planes) which byte
        ranges of the flat buffers just changed.  Only flat buffers whose owner registered interest - `_eav_track_dirty` -
        are tracked, and a list collapses to its hull once it passes 64 entries: an eager loop that nobody drains must
        not grow it."""
        tracked = [(fl, fl.data_ptr(), fl.data_ptr() + 4 * fl.numel()) for fl in touched.values()
                   if getattr(fl, "_eav_track_dirty", False)]
        for at, _, numel, _, _ in runs if tracked else ():
            for fl, lo, hi in tracked:
                if lo <= at < hi:
                    d = getattr(fl, "_eav_dirty", [])
                    d.append((at, at + 4 * numel))
                    if len(d) > 64:
                        d = [(min(a for a, _ in d), max(b for _, b in d))]
                    fl._eav_dirty = d

    def _step_jobs(self):
        """step() of ``multi_tensor=True`` (class docstring): eav_adam_jobs_begin + eav_adam_step_jobs over one table."""
        # checked across the groups BEFORE any state is touched: a refused step leaves the step counts where they were
        first = self.param_groups[0]
        shared = (tuple(float(b) for b in first["betas"]), float(first["eps"]), bool(first["decoupled"]))
        for group in self.param_groups:
            if (tuple(float(b) for b in group["betas"]), float(group["eps"]), bool(group["decoupled"])) != shared:
                raise _lib.EavError("FusedAdam(multi_tensor=True): betas, eps and decoupled must be equal across the param "
                                    "groups (lr and weight_decay may differ)")
        plan, touched, dev = self._gather()
        # a job's tensors share lr, weight decay and step count, whichever group they are in - the count being 0 for a
        # capturable optimiser, whose jobs all read the one device count (the default path keys on the host count then
        # too) - and are merged ACROSS the groups, in one address order: a job is a table row, their order costs no launch
        capturable, runs = self.capturable, []
        for group, rows in plan:
            lr, wd = float(group["lr"]), float(group["weight_decay"])
            for r in rows:
                r[_KEY] = (0 if capturable else r[_KEY], lr, wd)
            runs += rows
        jobs = _merge_rows(runs)
        if not jobs:        # no gradient anywhere: nothing is launched, the accumulator flags are emptied all the same
            self._acc_reset()
            return
        if self._sched is None or self._sched.device != dev:
            self._sched = torch.zeros(_lib.SCHED_WORDS, dtype=torch.int64, device=dev)
            self.last_lr = self._sched.view(torch.float32)[4]
        # the step counts change every step: they are seeded into the table's device counts, not part of its key
        key = (dev, capturable, tuple((at, rel, numel, lr, wd) for at, rel, numel, _, (_, lr, wd) in jobs))
        table = self._adam_tables.get(key)
        if table is None:
            if len(self._adam_tables) >= 16:
                self._adam_tables.clear()
            table = self._adam_tables[key] = _AdamJobTable(dev, jobs, self._dev_step.data_ptr() if capturable else None)
        table.sync_counts([r[_KEY][0] for r in jobs])
        gscale = self._grad_scale(dev, jobs)
        sch = self.schedule if self.schedule is not None else _CONSTANT
        b1, b2 = shared[0]
        st = _lib.stream_ptr()
        begin = (table.rows.data_ptr(), table.njobs, _lib.ptr(table.counts), table.njobs if table.per_tensor else 0,
                 self._sched.data_ptr(), sch.code, sch.num_warmup_steps, sch.num_training_steps, sch.num_cycles,
                 float(first["lr"]), b1, b2)
        avg = self.averaging
        if avg is None:
            _lib.call("eav_adam_jobs_begin", *begin, st)
            _lib.call("eav_adam_step_jobs", table.rows.data_ptr(), table.njobs, table.nchunks, b1, b2, shared[1],
                      int(shared[2]), gscale, st)
        else:
            rec = self._avg_rec.data_ptr()
            _lib.call("eav_adam_jobs_begin_avg", *begin, rec, avg.code, avg.decay, int(avg.warmup), avg.start_step,
                      avg.every, st)
            _lib.call("eav_adam_step_jobs_avg", table.rows.data_ptr(), table.avgs.data_ptr(), table.njobs, table.nchunks,
                      b1, b2, shared[1], int(shared[2]), gscale, rec, st)
        self._record_dirty(touched, jobs)

    def _init_state(self, p, st):
        """Step count 0 and zero moments; the moments of a flat model's parameters are views of two flat buffers laid out
        like the parameters, so that adjacent tensors stay adjacent in all four."""
        st["step"] = 0
        flat = getattr(p, "_eav_flat", None)
        if flat is not None and flat[0].data_ptr() + 4 * flat[2] == p.data_ptr():
            shared = self._flat_state.setdefault(flat[0].data_ptr(), {})
            if not shared:
                shared["m"] = torch.zeros_like(flat[0])
                shared["v"] = torch.zeros_like(flat[0])
            st["exp_avg"] = shared["m"][flat[2]:flat[2] + p.numel()].view(p.shape)
            st["exp_avg_sq"] = shared["v"][flat[2]:flat[2] + p.numel()].view(p.shape)
        else:
            st["exp_avg"] = torch.zeros_like(p)
            st["exp_avg_sq"] = torch.zeros_like(p)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        if self._swapped:
            raise _lib.EavError("FusedAdam.step() inside averaged_parameters(): the parameters hold the averages")
        if self.averaging is not None and not self.multi_tensor:
            raise _lib.EavError("FusedAdam: weight averaging runs inside the multi-tensor step - multi_tensor was turned "
                                "off after set_averaging")
        if self.capturable:
            count = self.device_step_counter()
            if self.step_counted:
                self.step_counted = False
            else:
                _lib.call("eav_counter_inc", count.data_ptr(), _lib.stream_ptr())
        if self.multi_tensor:
            self._step_jobs()
            return loss
        # one launch per run of adjacent tensors that share a step count - the HOST count, also when capturable (all equal
        # then).  Merged WITHIN a group only and launched group by group, by address inside a group: the hyper-parameters
        # are launch arguments.  The grad-norm ranges follow the same order, which is the order the fp64 partials are
        # added in and so decides the bits of the norm.
        plan, touched, dev = self._gather()
        plan = [(group, _merge_rows(rows)) for group, rows in plan]
        runs = [r for _, rows in plan for r in rows]
        gscale = self._grad_scale(dev, runs)        # (no gradient anywhere: runs is empty and nothing is launched)
        for group, rows in plan:
            for at, (g, m, v), numel, _, step in rows:
                self._launch(at, at + g, at + m, at + v, numel, group, step, gscale)
        self._record_dirty(touched, runs)
        return loss


_CLIP_TABLES = _JobTables()


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False):
    """``torch.nn.utils.clip_grad_norm_`` on the device: scales every ``p.grad`` in place by
    min(1, max_norm / (norm + 1e-6)) and returns the global L2 norm before clipping as a 0-dim device tensor - three
    launches (``eav_grad_sumsq``, ``eav_grad_clip_finish``, ``eav_scale_ranges``), nothing read back.  L2 only; a
    non-finite norm is handled like torch's default (NaN scales by NaN, infinity by 0)."""
    if float(norm_type) != 2.0:
        raise NotImplementedError(f"clip_grad_norm_: norm_type {norm_type!r} - only the L2 norm is implemented")
    if error_if_nonfinite:
        raise NotImplementedError("clip_grad_norm_: error_if_nonfinite=True needs the norm on the host; read the "
                                  "returned tensor instead")
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    ps = [p for p in parameters if p.grad is not None]
    if not ps:
        raise _lib.EavError("clip_grad_norm_: no parameter has a gradient")
    ranges = []
    for p in ps:
        g = p.grad
        if not g.is_cuda or g.dtype != torch.float32 or not g.is_contiguous() or g.device != ps[0].grad.device:
            raise _lib.EavError("clip_grad_norm_ needs contiguous fp32 gradients on one ROCm device (no CPU fallback)")
        if g.numel():
            ranges.append([g.data_ptr(), (0,), g.numel(), _flat_slack(p), None])
    dev = ps[0].grad.device
    _, jobs, njobs, nchunks, partials = _CLIP_TABLES.get(dev, tuple((at, at, numel) for at, _, numel, _, _ in _merge_rows(ranges)))
    out = torch.empty(2, dtype=torch.float32, device=dev)
    st = _lib.stream_ptr()
    _lib.call("eav_grad_sumsq", jobs.data_ptr(), njobs, nchunks, partials.data_ptr(), st)
    _lib.call("eav_grad_clip_finish", partials.data_ptr(), nchunks, float(max_norm), out.data_ptr(), st)
    _lib.call("eav_scale_ranges", jobs.data_ptr(), njobs, nchunks, out.data_ptr() + 4, st)
    return out[0]
