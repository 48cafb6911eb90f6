"""Reference arithmetic of the weight-averaging tests (csrc/adam_jobs.hip: eav_adam_jobs_begin_avg, eav_adam_step_jobs_avg;
optim.WeightAveraging, FusedAdam.set_averaging).  numpy only.

  * float64: `mode_and_coefficient`, the gating and the coefficient of every step (s counts the optimiser steps from 1, n
    the averaging steps so far), and `Averager`, the update itself over a list of tensors.  tests/test_weight_avg_cpu.py
    pins both to torch.optim.swa_utils.AveragedModel in float64.
  * float32: `lerp_f32`, the kernel's element arithmetic - d = p_new - avg rounded to fp32, then one fused multiply-add
    fmaf(c, d, avg), emulated through float64 (the product of two fp32 numbers is exact in double).

The bound of one lerp against exact arithmetic on identical fp32 inputs (the coefficient included: the reference takes c
as the fp32 value the kernel reads, `coefficient_f32`).  With Mx = max(|p_new|, |avg|):
    d = fl(p_new - avg) rounds once: relative error 2^-24, and |p_new - avg| <= 2 Mx, so |d - (p_new - avg)| <= 2 * 2^-24 Mx,
    which the factor c <= 1 does not enlarge;  the fma rounds once, and its result lies between avg and p_new up to that
    error: <= 2^-24 Mx more.  One update: <= 3 * 2^-24 Mx.
An error already in avg is carried with the factor (1 - c) <= 1, so after k updates the error is at most 3 k 2^-24 Mx.
`Tracked` adds the bound up update by update, 3 * 2^-24 Mx_k with Mx_k = max(|p_k|, |avg_ref| + the bound so far) - the
reference's own average plus what the kernel's may differ from it by - which never exceeds 3 k 2^-24 max_k Mx_k.  A copy
(mode "copy") is exact and starts the sum again at 0.  No fitted tolerance anywhere."""
import numpy as np

U = 2.0 ** -24          # half an ulp of 1.0 in fp32: the relative error of one rounding
KINDS = ("ema", "swa")
MODES = ("skip", "copy", "lerp")


def mode_and_coefficient(kind, s, n, decay=0.999, warmup=False, start_step=0, every=1):
    """(mode, c) of optimiser step s (from 1) when n steps have been averaged; c a float64."""
    assert kind in KINDS, kind
    if s < start_step or (s - start_step) % every != 0:
        return "skip", 0.0
    if n == 0:
        return "copy", 1.0
    if kind == "swa":
        return "lerp", 1.0 / (float(n) + 1.0)
    d = float(decay)
    if warmup:
        d = min(d, (1.0 + float(n)) / (10.0 + float(n)))
    return "lerp", 1.0 - d


def coefficient_f32(c):
    """The coefficient as the device record holds it: the float64 expression rounded once."""
    return np.float32(np.float64(c))


def sequence(kind, steps, **kw):
    """[(s, n after the step, mode, c)] for s = 1 .. steps."""
    out, n = [], 0
    for s in range(1, steps + 1):
        mode, c = mode_and_coefficient(kind, s, n, **kw)
        n += mode != "skip"
        out.append((s, n, mode, c))
    return out


class Averager:
    """float64 averages of a list of tensors.  update(params, present): one optimiser step; present[i] False: tensor i
    was not part of the step (no gradient) and keeps its average.  c32=True takes the coefficient as its fp32 value."""

    def __init__(self, params, kind, c32=False, **kw):
        self.avg = [np.asarray(p, dtype=np.float64).copy() for p in params]
        self.kind, self.kw, self.c32 = kind, kw, c32
        self.s = self.n = 0
        self.mode = None

    def update(self, params, present=None):
        self.s += 1
        mode, c = mode_and_coefficient(self.kind, self.s, self.n, **self.kw)
        self.mode = mode
        if self.c32:
            c = float(coefficient_f32(c))
        for i, p in enumerate(params):
            if mode == "skip" or (present is not None and not present[i]):
                continue
            p = np.asarray(p, dtype=np.float64)
            self.avg[i] = p.copy() if mode == "copy" else self.avg[i] + c * (p - self.avg[i])
        self.n += mode != "skip"
        return mode, c


def lerp_f32(avg, p, c):
    """fmaf(c, p - avg, avg) operation by operation in numpy float32; c an fp32 value."""
    avg, p = np.asarray(avg, dtype=np.float32), np.asarray(p, dtype=np.float32)
    d = p - avg
    assert d.dtype == np.float32
    return (np.float64(np.float32(c)) * d.astype(np.float64) + avg.astype(np.float64)).astype(np.float32)


class Tracked:
    """One tensor: the float64 average fed with the fp32 parameters the kernel produced, and the bound added up update
    by update (module docstring)."""

    def __init__(self, p0):
        self.avg = np.asarray(p0, dtype=np.float64).copy()
        self.tol = np.zeros_like(self.avg)
        self.updates = 0

    def update(self, mode, c, p):
        """c: the fp32 coefficient of the step (as a float)."""
        p = np.asarray(p, dtype=np.float64)
        if mode == "copy":
            self.avg, self.tol, self.updates = p.copy(), np.zeros_like(p), 0
        elif mode == "lerp":
            mx = np.maximum(np.abs(p), np.abs(self.avg) + self.tol)
            self.avg = self.avg + float(c) * (p - self.avg)
            self.tol = self.tol + 3.0 * U * mx
            self.updates += 1

    def check(self, got, what):
        err = np.abs(np.asarray(got, dtype=np.float64).reshape(self.avg.shape) - self.avg)
        worst = float(np.max(err / np.maximum(self.tol, 1e-300))) if self.updates else float(err.max())
        print(f"{what}: {self.updates} updates, worst error / bound {worst:.3f} (max error {float(err.max()):.3e})")
        assert np.all(err <= self.tol), (what, worst)
        return worst
