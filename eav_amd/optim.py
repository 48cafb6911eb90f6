"""Fused Adam / AdamW over flat parameter storage + the criteria (cross-entropy, BCE-with-logits, MSE).

Host-side mirrors of what the reference trainers construct:
  * ``optim.Adam(model.parameters(), lr)``            CNN_torch/EEGNet_tor.py:82
  * ``optim.AdamW(model.parameters(), lr)``           Transformer_Audio.py:30, Transformer_Vision.py:36
    (weight_decay is torch's default 0.01 - the trainer's ctor argument is ignored)
  * ``nn.CrossEntropyLoss()``                          EEGNet_tor.py:81, Transformer_Audio.py:31

  * ``nn.BCEWithLogitsLoss()`` / ``nn.MSELoss()``      the other two losses HF's classification models pick by
    ``config.problem_type`` (transformers/loss/loss_utils.py, ForSequenceClassificationLoss)

The arithmetic runs in libeav_hip.so (``eav_adam_step`` / ``eav_ce_fwd_bwd`` / ``eav_bce_logits_fwd_bwd`` / ``eav_mse_fwd_bwd``;
``eav_ce_general_fwd_bwd`` for ``CrossEntropyLoss(weight=..., label_smoothing=...)`` and class-probability targets).
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
"""
from __future__ import annotations

import os

import torch

from . import _lib


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


def _merge_ranges(ranges):
    """ranges: lists [ptr, other_ptr, numel, slack_bytes] - merged, in address order, where the next range begins less than
    `slack_bytes` after the end of the previous one at BOTH pointers (flat buffers: the 16-byte alignment padding plus
    declared zero padding, whose gradient is zero; loose tensors: slack 1, i.e. exactly adjacent)."""
    merged = []
    for r in sorted(ranges, key=lambda r: r[0]):
        if merged:
            q = merged[-1]
            gap = r[0] - (q[0] + 4 * q[2])
            if 0 <= gap < q[3] and r[1] - q[1] == r[0] - q[0]:
                q[2] = (r[0] - q[0]) // 4 + r[2]
                q[3] = r[3]
                continue
        merged.append(list(r))
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


class _AdamJobTable:
    """One cached table of eav_adam_step_jobs (rows: include/eav_hip.h) with the device step counts its rows read."""

    def __init__(self, device, jobs, shared_step_ptr):
        words = _lib.JOB_WORDS
        n = len(jobs)
        self.njobs = n
        self.nchunks = sum(int(_lib.plain("eav_adam_jobs_nchunks", r[4])) for r in jobs)
        self.per_tensor = shared_step_ptr is None
        # the counts hold the steps COMPLETED: eav_adam_jobs_begin advances them before it reads them
        self.counts = torch.tensor([r[5] - 1 for r in jobs], dtype=torch.int64).to(device) if self.per_tensor else None
        self.steps = [r[5] - 1 for r in jobs]           # host mirror: the step each job ran last
        rows = torch.zeros(n, words, dtype=torch.int64)
        rows[:, :5] = torch.tensor([r[:5] for r in jobs], dtype=torch.int64)
        rows[:, 5] = torch.tensor([r[6] for r in jobs], dtype=torch.float64).view(torch.int64)
        if self.per_tensor:
            rows[:, 6] = self.counts.data_ptr() + 8 * torch.arange(n, dtype=torch.int64)
        else:
            rows[:, 6] = shared_step_ptr
        rows[:, 7] = torch.tensor([r[7] for r in jobs], dtype=torch.float32).view(torch.int32).to(torch.int64) & 0xffffffff
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
    run one step eagerly before capturing, and capture again after ``set_schedule``."""

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
            ranges.append([g.data_ptr(), self.accumulated_grad(p).data_ptr(), p.numel(), _flat_slack(p)])
        dev = ps[0].device
        tables = self._tables.get(dev, tuple((r[0], r[1], r[2]) for r in _merge_ranges(ranges)))
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

    def _step_jobs(self):
        """step() of ``multi_tensor=True`` (class docstring): eav_adam_jobs_begin + eav_adam_step_jobs over one table."""
        first = self.param_groups[0]
        shared = (tuple(float(b) for b in first["betas"]), float(first["eps"]), bool(first["decoupled"]))
        folded = set(self._acc_key) if self._acc_folds else None      # accumulate() was called: consume the accumulator
        runs, touched = [], {}
        for group in self.param_groups:
            if (tuple(float(b) for b in group["betas"]), float(group["eps"]), bool(group["decoupled"])) != shared:
                raise _lib.EavError("FusedAdam(multi_tensor=True): betas, eps and decoupled must be equal across the param "
                                    "groups (lr and weight_decay may differ)")
        for group in self.param_groups:
            lr, wd = float(group["lr"]), float(group["weight_decay"])
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
                if getattr(p, "_eav_flat", None) is not None:
                    touched[p._eav_flat[0].data_ptr()] = p._eav_flat[0]
                if not st:
                    self._init_state(p, st)
                st["step"] += 1
                # [p, g, m, v, numel, step, lr, wd, declared padding in bytes]
                runs.append([p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                             p.numel(), 0 if self.capturable else st["step"], lr, wd, 4 * getattr(p, "_eav_pad", 0)])
        if not runs:
            self._acc_folds, self._acc_partials = 0, False
            return
        # merge what is adjacent in all four buffers (up to the 16-byte alignment padding plus declared zero padding,
        # whose gradient and moments are zero) and shares lr, weight decay and step count - whichever group it is in
        runs.sort(key=lambda r: r[0])
        jobs = []
        for r in runs:
            if jobs:
                q = jobs[-1]
                gap = r[0] - (q[0] + 4 * q[4])
                if (0 <= gap < 16 + q[8] and r[5:8] == q[5:8] and r[1] - q[1] == r[0] - q[0]
                        and r[2] - q[2] == r[0] - q[0] and r[3] - q[3] == r[0] - q[0]):
                    q[4] = (r[0] - q[0]) // 4 + r[4]
                    q[8] = r[8]
                    continue
            jobs.append(r)
        dev = next(iter(p for group in self.param_groups for p in group["params"])).device
        if self._sched is None or self._sched.device != dev:
            self._sched = torch.zeros(_lib.SCHED_WORDS, dtype=torch.int64, device=dev)
            self.last_lr = self._sched.view(torch.float32)[4]
        # the step counts change every step: they are seeded into the table's device counts, not part of its key
        key = (dev, self.capturable, tuple((r[0], r[1], r[2], r[3], r[4], r[6], r[7]) for r in jobs))
        table = self._adam_tables.get(key)
        if table is None:
            if len(self._adam_tables) >= 16:
                self._adam_tables.clear()
            table = self._adam_tables[key] = _AdamJobTable(dev, jobs, self._dev_step.data_ptr() if self.capturable else None)
        table.sync_counts([r[5] for r in jobs])
        gscale = None
        if self.max_grad_norm is not None:
            if folded is not None:      # the accumulator's own table: the partials of a last=True fold belong to it
                gscale = self._clip(dev, self._acc_tables, self._acc_partials)
            else:
                gscale = self._clip(dev, self._tables.get(dev, tuple((r[1], r[1], r[4]) for r in jobs)), False)
        self._acc_folds, self._acc_partials = 0, False
        sch = self.schedule if self.schedule is not None else _CONSTANT
        b1, b2 = shared[0]
        st = _lib.stream_ptr()
        _lib.call("eav_adam_jobs_begin", table.rows.data_ptr(), table.njobs, _lib.ptr(table.counts),
                  table.njobs if table.per_tensor else 0, self._sched.data_ptr(), sch.code, sch.num_warmup_steps,
                  sch.num_training_steps, sch.num_cycles, float(first["lr"]), b1, b2, st)
        _lib.call("eav_adam_step_jobs", table.rows.data_ptr(), table.njobs, table.nchunks, b1, b2, shared[1],
                  int(shared[2]), gscale, st)
        # the byte ranges that just changed, for whoever caches derived copies of these parameters (step()'s comment)
        for fl in touched.values():
            if not getattr(fl, "_eav_track_dirty", False):
                continue
            lo = fl.data_ptr()
            d = getattr(fl, "_eav_dirty", [])
            d.extend((r[0], r[0] + 4 * r[4]) for r in jobs if lo <= r[0] < lo + 4 * fl.numel())
            if len(d) > 64:
                d = [(min(a for a, _ in d), max(b for _, b in d))]
            fl._eav_dirty = d

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
        if self.capturable:
            if self._dev_step is None:
                dev = next(p for g in self.param_groups for p in g["params"]).device
                self._dev_step = torch.zeros((), dtype=torch.int64, device=dev)
            if self.step_counted:
                self.step_counted = False
            else:
                _lib.call("eav_counter_inc", self._dev_step.data_ptr(), _lib.stream_ptr())
        if self.multi_tensor:
            self._step_jobs()
            return loss
        folded = set(self._acc_key) if self._acc_folds else None      # accumulate() was called: consume the accumulator
        plan = []
        for group in self.param_groups:
            runs = []  # (p_ptr, g_ptr, m_ptr, v_ptr, numel, step) candidates for merging
            touched = {}
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
                if getattr(p, "_eav_flat", None) is not None:
                    touched[p._eav_flat[0].data_ptr()] = p._eav_flat[0]
                if not st:
                    self._init_state(p, st)
                st["step"] += 1
                runs.append([p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                             p.numel(), st["step"], g, 4 * getattr(p, "_eav_pad", 0)])
            # merge runs that are adjacent (up to 16-B alignment padding, plus declared zero padding - whose
            # gradient and moments are zero, so the update leaves it zero) in all four buffers
            runs.sort(key=lambda r: r[0])
            merged = []
            for r in runs:
                if merged:
                    q = merged[-1]
                    gap = r[0] - (q[0] + 4 * q[4])
                    if (0 <= gap < 16 + q[7] and r[5] == q[5] and r[1] - q[1] == r[0] - q[0]
                            and r[2] - q[2] == r[0] - q[0] and r[3] - q[3] == r[0] - q[0]):
                        q[4] = (r[0] - q[0]) // 4 + r[4]
                        q[7] = r[7]
                        continue
                merged.append(r)
            plan.append((group, merged, touched))
        gscale = None
        if self.max_grad_norm is not None and any(merged for _, merged, _ in plan):
            dev = next(r[6].device for _, merged, _ in plan for r in merged)
            if folded is not None:      # the accumulator's own table: the partials of a last=True fold belong to it
                gscale = self._clip(dev, self._acc_tables, self._acc_partials)
            else:
                ranges = tuple((r[1], r[1], r[4]) for _, merged, _ in plan for r in merged)
                gscale = self._clip(dev, self._tables.get(dev, ranges), False)
        self._acc_folds, self._acc_partials = 0, False
        for group, merged, touched in plan:
            for r in merged:
                self._launch(r[0], r[1], r[2], r[3], r[4], group, r[5], gscale)
                # tell whoever caches derived copies of these parameters (transformer.Encoder's fp16 operand
                # planes) which byte ranges of the flat buffer just changed
                # (only flat buffers whose owner registered interest - `_eav_track_dirty` - are tracked, and the list
                # collapses to its hull beyond a few entries: an eager loop that nobody drains must not grow it)
                for fl in touched.values():
                    lo = fl.data_ptr()
                    if getattr(fl, "_eav_track_dirty", False) and lo <= r[0] < lo + 4 * fl.numel():
                        d = getattr(fl, "_eav_dirty", [])
                        d.append((r[0], r[0] + 4 * r[4]))
                        if len(d) > 64:
                            d = [(min(a for a, _ in d), max(b for _, b in d))]
                        fl._eav_dirty = d
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
            ranges.append([g.data_ptr(), g.data_ptr(), g.numel(), _flat_slack(p)])
    dev = ps[0].grad.device
    _, jobs, njobs, nchunks, partials = _CLIP_TABLES.get(dev, tuple((r[0], r[1], r[2]) for r in _merge_ranges(ranges)))
    out = torch.empty(2, dtype=torch.float32, device=dev)
    st = _lib.stream_ptr()
    _lib.call("eav_grad_sumsq", jobs.data_ptr(), njobs, nchunks, partials.data_ptr(), st)
    _lib.call("eav_grad_clip_finish", partials.data_ptr(), nchunks, float(max_norm), out.data_ptr(), st)
    _lib.call("eav_scale_ranges", jobs.data_ptr(), njobs, nchunks, out.data_ptr() + 4, st)
    return out[0]


class _CEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, targets, flag, scratch=None, general=None):
        B, NC = scores.shape
        loss = torch.empty((), dtype=torch.float32, device=scores.device)
        need_grad = ctx.needs_input_grad[0]
        dsc = torch.empty_like(scores) if need_grad else None      # no gradient buffer under no_grad (validate())
        _ce_launch(scratch, scores, targets, loss, dsc, None, flag, general)
        ctx.dsc = dsc
        return loss

    @staticmethod
    def backward(ctx, gout):
        return _seeded(ctx.dsc, gout), None, None, None, None


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


_UNIT = {}


def unit_gradient(device):
    """A device-resident constant 1.0 to seed ``loss.backward(gradient=unit_gradient(dev))`` with: autograd then needs no
    fill kernel for the implicit ones_like(loss), and the CE backward recognises it and skips its scaling launch."""
    device = torch.device(device)
    if device not in _UNIT:
        t = torch.ones((), dtype=torch.float32, device=device)
        _UNIT[device] = (t, t.data_ptr())
    return _UNIT[device][0]


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
        self._scratch = {}
        self._general_scratch = {}
        self.head_algo = os.environ.get("EAV_HEAD_ALGO", "auto")

    weight = property(lambda self: self._weight, doc="per-class weights (fp32 tensor) or None; fixed at construction")
    label_smoothing = property(lambda self: self._smoothing, doc="the smoothing factor; fixed at construction")

    def _wide(self, classes):
        return head_is_wide(self.head_algo, classes, "the scores have")

    def _scratch_for(self, scores):
        """The wide kernel's row terms for this batch size (None: the narrow kernel runs)."""
        B, NC = scores.shape
        if not self._wide(NC):
            return None
        key = (B, scores.device)
        if key not in self._scratch:
            self._scratch[key] = torch.empty(_lib.plain("eav_ce_wide_ws_floats", B), dtype=torch.float32, device=scores.device)
        return self._scratch[key]

    def _route(self, scores, targets):
        """(scratch, general) of _ce_launch: the default criterion on class indices keeps its two kernels, everything else
        takes the general one with the weights on the scores' device."""
        if targets.dim() == 1 and self._weight is None and self._smoothing == 0.0:
            return self._scratch_for(scores), None
        B, NC = scores.shape
        if self._weight is not None:
            if self._weight.numel() != NC:
                raise ValueError(f"CrossEntropyLoss: {self._weight.numel()} class weights for {NC} classes")
            if self._weight.device != scores.device:
                self._weight = self._weight.to(scores.device)
        key = (B, scores.device)
        if key not in self._general_scratch:
            self._general_scratch[key] = torch.empty(_lib.plain("eav_ce_general_ws_floats", B), dtype=torch.float32,
                                                     device=scores.device)
        return self._general_scratch[key], (self._weight, self._smoothing)

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
        if not scores.is_cuda or scores.dim() != 2 or scores.dtype != torch.float32 or not scores.is_contiguous():
            raise _lib.EavError("CrossEntropyLoss.accumulate: scores must be a contiguous fp32 [batch, classes] device tensor")
        # every operand goes to the kernel as a raw pointer: a host tensor would be dereferenced on the GPU
        soft = isinstance(targets, torch.Tensor) and targets.dim() == 2
        if soft and not targets.is_floating_point():
            raise TypeError(f"CrossEntropyLoss.accumulate: [batch, classes] targets are class probabilities, got {targets.dtype}")
        if not isinstance(targets, torch.Tensor) or targets.device != scores.device \
                or (tuple(targets.shape) != tuple(scores.shape) if soft else
                    targets.dim() != 1 or targets.numel() != scores.shape[0]):
            raise _lib.EavError(f"CrossEntropyLoss.accumulate: targets must be {scores.shape[0]} labels on {scores.device} "
                                "(no CPU fallback: move the loader's tensors to the device)")
        if not isinstance(loss_out, torch.Tensor) or loss_out.device != scores.device or loss_out.dtype != torch.float32 \
                or loss_out.numel() < 1:
            raise _lib.EavError(f"CrossEntropyLoss.accumulate: loss_out must be an fp32 tensor on {scores.device}")
        if not isinstance(ncorrect, torch.Tensor) or ncorrect.device != scores.device or ncorrect.dtype != torch.int32 \
                or ncorrect.numel() < 1:
            raise _lib.EavError(f"CrossEntropyLoss.accumulate: ncorrect must be an int32 tensor on {scores.device}")
        targets = self._targets(scores, targets, "CrossEntropyLoss.accumulate")
        if self._flag is None or self._flag.device != scores.device:
            self._flag = torch.zeros((), dtype=torch.int32, device=scores.device)
        scratch, general = self._route(scores, targets)
        _ce_launch(scratch, scores, targets, loss_out, None, ncorrect, self._flag, general)

    def __call__(self, scores, targets):
        if isinstance(targets, torch.Tensor) and targets.dim() == 2 and not targets.is_floating_point():
            raise TypeError(f"CrossEntropyLoss: [batch, classes] targets are class probabilities, got {targets.dtype}")
        if not isinstance(scores, torch.Tensor) or not scores.is_cuda or not targets.is_cuda:
            raise _lib.EavError("CrossEntropyLoss needs device tensors (no CPU fallback)")
        if scores.dim() != 2 or scores.dtype != torch.float32 or not scores.is_contiguous():
            raise _lib.EavError(f"CrossEntropyLoss: scores must be a contiguous fp32 [batch, classes] tensor, got "
                                f"{tuple(scores.shape)} {scores.dtype}")
        targets = self._targets(scores, targets, "CrossEntropyLoss")
        if self._flag is None or self._flag.device != scores.device:
            self._flag = torch.zeros((), dtype=torch.int32, device=scores.device)
        scratch, general = self._route(scores, targets)
        return _CEFn.apply(scores, targets, self._flag, scratch, general)


class _ElementLossFn(torch.autograd.Function):
    """_CEFn's shape for the element-wise criteria: the forward launch produces the loss and d loss / d scores together."""

    @staticmethod
    def forward(ctx, scores, targets, crit):
        loss = torch.empty((), dtype=torch.float32, device=scores.device)
        dsc = torch.empty_like(scores) if ctx.needs_input_grad[0] else None      # no gradient buffer under no_grad
        crit._launch(scores, targets, loss, dsc, None)
        ctx.dsc = dsc
        return loss

    @staticmethod
    def backward(ctx, gout):
        return _seeded(ctx.dsc, gout), None, None


class _ElementLoss:
    """What BCEWithLogitsLoss and MSELoss share: the mean over all batch x classes elements and its gradient from one
    launch of csrc/head_loss.hip (one wave per row, row sums added in row order - no atomics, two runs give the same bits).

    Targets are fp32 [batch, classes] on the scores' device ([batch] accepted for one class; integer targets are
    converted to fp32) and are not validated - torch accepts any float - so `check()` has nothing to report and is a
    no-op that trainers may call blindly.  The kernels' per-row scratch is kept on the criterion, one buffer per
    (batch, device): nothing is allocated for it in the launch path, and nothing synchronises with the host."""

    _NAME = _ENTRY = None

    def __init__(self):
        self._scratch = {}

    def check(self):
        pass

    def _scratch_for(self, scores):
        key = (scores.shape[0], scores.device)
        if key not in self._scratch:
            self._scratch[key] = torch.empty(_lib.plain("eav_head_loss_ws_floats", scores.shape[0]), dtype=torch.float32,
                                             device=scores.device)
        return self._scratch[key]

    def _operands(self, scores, targets, who):
        if not isinstance(scores, torch.Tensor) or not scores.is_cuda or not isinstance(targets, torch.Tensor) \
                or not targets.is_cuda:
            raise _lib.EavError(f"{who} needs device tensors (no CPU fallback)")
        if scores.dim() != 2 or scores.dtype != torch.float32 or not scores.is_contiguous():
            raise _lib.EavError(f"{who}: scores must be a contiguous fp32 [batch, classes] tensor, got "
                                f"{tuple(scores.shape)} {scores.dtype}")
        B, NC = scores.shape
        # every operand goes to the kernel as a raw pointer: a tensor elsewhere would be dereferenced on this GPU
        if targets.device != scores.device:
            raise _lib.EavError(f"{who}: targets are on {targets.device}, the scores on {scores.device}")
        if tuple(targets.shape) != (B, NC) and not (NC == 1 and tuple(targets.shape) == (B,)):
            raise _lib.EavError(f"{who}: targets {tuple(targets.shape)} for scores {(B, NC)}")
        if targets.dtype != torch.float32:
            targets = targets.float()
        return targets.reshape(B, NC).contiguous()

    def _out_check(self, t, dtype, what, scores, who):
        if not isinstance(t, torch.Tensor) or t.device != scores.device or t.dtype != dtype or t.numel() < 1:
            raise _lib.EavError(f"{who}: {what} must be a {str(dtype).replace('torch.', '')} tensor on {scores.device}")

    def __call__(self, scores, targets):
        targets = self._operands(scores, targets, self._NAME)
        return _ElementLossFn.apply(scores, targets, self)


class BCEWithLogitsLoss(_ElementLoss):
    """``nn.BCEWithLogitsLoss()`` (mean over batch x classes; no pos_weight): HF's loss for
    problem_type "multi_label_classification".  Term max(x, 0) - x t + log1p(exp(-|x|)), torch's form, finite for any
    finite logit; gradient (sigmoid(x) - t) / (batch x classes).  See _ElementLoss for targets, scratch and check()."""

    _NAME = "BCEWithLogitsLoss"

    def _launch(self, scores, targets, loss, dsc, nhits):
        B, NC = scores.shape
        _lib.call("eav_bce_logits_fwd_bwd", scores.data_ptr(), targets.data_ptr(), _lib.ptr(loss), _lib.ptr(dsc),
                  _lib.ptr(nhits), self._scratch_for(scores).data_ptr(), B, NC, _lib.stream_ptr())

    def accumulate(self, scores, targets, loss_out, nhits):
        """Evaluation form (no gradient, nothing read back): the batch's mean loss into the 0-dim device tensor
        `loss_out`, and the number of elements with (score > 0) == (target > 0.5) - the multi-label counterpart of
        CrossEntropyLoss's argmax hits - added to the device int32 `nhits`."""
        who = "BCEWithLogitsLoss.accumulate"
        targets = self._operands(scores, targets, who)
        self._out_check(loss_out, torch.float32, "loss_out", scores, who)
        self._out_check(nhits, torch.int32, "nhits", scores, who)
        self._launch(scores, targets, loss_out, None, nhits)


class MSELoss(_ElementLoss):
    """``nn.MSELoss()`` (mean over batch x classes): HF's loss for problem_type "regression".  Term (x - t)^2, gradient
    2 (x - t) / (batch x classes).  See _ElementLoss for targets, scratch and check()."""

    _NAME = "MSELoss"

    def _launch(self, scores, targets, loss, dsc, nhits):
        B, NC = scores.shape
        _lib.call("eav_mse_fwd_bwd", scores.data_ptr(), targets.data_ptr(), _lib.ptr(loss), _lib.ptr(dsc),
                  self._scratch_for(scores).data_ptr(), B, NC, _lib.stream_ptr())

    def accumulate(self, scores, targets, loss_out):
        """Evaluation form (no gradient, nothing read back): the batch's mean loss into the 0-dim device tensor `loss_out`."""
        who = "MSELoss.accumulate"
        targets = self._operands(scores, targets, who)
        self._out_check(loss_out, torch.float32, "loss_out", scores, who)
        self._launch(scores, targets, loss_out, None, None)
