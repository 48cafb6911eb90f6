"""Reference arithmetic of the multi-tensor Adam tests (csrc/adam_jobs.hip, optim.FusedAdam(multi_tensor=True), LRSchedule).

Two parts, numpy only:
  * float64: the four schedule factors of transformers.get_scheduler, and an Adam / AdamW stepper with per-tensor lr,
    weight decay and step count (the update itself is tests/grad_clip_ref.adam_step).  tests/test_adam_jobs_cpu.py pins
    both to transformers / torch.optim on the CPU.
  * float32: `adam_step_f32`, a restatement of the kernel's expression order (adam_update, csrc/eav_common.h) in numpy
    float32 with its three fused multiply-adds emulated through float64, and the error bounds of the GPU tests.

Bounds of ONE step from identical fp32 inputs (hyper-parameters included: the reference takes betas, eps, weight decay
and the rate as the fp32 values the kernel receives - float32(0.999) is 1.3e-5 away from 0.999 relative to 1 - 0.999).
With EPS = 2^-23, G = |g c| + |wd p0| (Adam with weight decay; |g c| otherwise; c the clipping coefficient or 1),
S_m = |b1 m0| + (1 - b1) G, S_v = |b2 v0| + (1 - b2) G^2:
    |m - m_ref| <= 4 EPS S_m          two products and a sum, each rounded (1.5 EPS S_m), and the gradient's own rounding
    |v - v_ref| <= 4 EPS S_v          under a scale or a coupled decay (<= 1 EPS G on g, 2 EPS G^2 on g^2): < 4 EPS
    |p - p_ref| <= 1.25 EPS |p_ref| + 16 EPS D,   D = |lr wd p0| + (lr / bc1) (S_m / denom_ref)
These are the bounds |m - m_ref| <= 4 EPS (|b1 m0| + |(1 - b1) g|) and |p - p_ref| <= EPS |p_ref| + 16 EPS |delta_ref| with
two things made exact.  Cancellation: G is |g_eff| and D is the reference's total change of p, |delta_ref|, wherever the
terms of g_eff = g c + wd p0 and of m do not cancel; where they cancel, the ABSOLUTE error of the sum - EPS G, 4 EPS S_m -
is what reaches m, v and p, not one relative to the small result (test_adam_jobs_cpu.py runs the float32 restatement on
such inputs: with |g_eff| for G its m misses the bound by a factor of 8, with G and D it holds).  1.25 EPS |p_ref|:
the decayed p and the final fma are rounded to fp32, half an ulp each - up to EPS |p| together just above a power of
two - and AdamW's factor 1 - lr wd is itself one rounded fma just below 1: 2^-25 relative, EPS / 4.  16 EPS D: the
step term collects m (<= 4 EPS relative to S_m), sqrt(v) (<= 2.5 EPS), bc2s, the quotient, eps's sum, m / denom, bc1
and lr / bc1 (<= 0.5 EPS each but bc2s, a rounded square root of a rounded difference: 1 EPS) - under 11 EPS.
Over k steps the bounds are added up step by step (`Trajectory`): errors of m and v decay by b1 and b2 per step, so the
sums bound them; the step term of step s sees the relative errors of m and v accumulated over s steps, so its share is
taken s times."""
import math

import numpy as np

from tests import grad_clip_ref as R

EPS = 2.0 ** -23
KINDS = ("constant", "constant_with_warmup", "linear", "cosine")


def f32(x):
    return np.asarray(x, dtype=np.float32)


def schedule_factor(kind, t, warmup=0, total=0, num_cycles=0.5):
    """The multiplier of transformers.get_scheduler(kind, ...)'s lambda at step t, float64."""
    if kind == "constant":
        return 1.0
    if t < warmup:
        return float(t) / float(max(1, warmup))
    if kind == "constant_with_warmup":
        return 1.0
    if kind == "linear":
        return max(0.0, float(total - t) / float(max(1, total - warmup)))
    assert kind == "cosine", kind
    progress = float(t - warmup) / float(max(1, total - warmup))
    return max(0.0, 0.5 * (1.0 + math.cos(math.pi * float(num_cycles) * 2.0 * progress)))


def lr_f32(base_lr, factor):
    """The rate eav_adam_jobs_begin stores: the product formed in double, rounded once to fp32."""
    return np.float32(np.float64(base_lr) * np.float64(factor))


def bias_corrections_f32(b1, b2, step):
    """(bc1, bc2s) as the kernels form them: powers in float64 from the fp32 betas, rounded once to fp32."""
    b1, b2 = np.float64(np.float32(b1)), np.float64(np.float32(b2))
    return np.float32(1.0 - b1 ** float(step)), np.float32(np.sqrt(1.0 - b2 ** float(step)))


class Stepper:
    """float64 Adam / AdamW over a list of tensors with per-tensor lr, weight decay and step count.  step(grads, lrs):
    a gradient of None skips the tensor (its count does not move), like torch."""

    def __init__(self, params, weight_decays, decoupled, betas=(0.9, 0.999), eps=1e-8):
        self.p = [R.f64(p).copy() for p in params]
        self.m = [np.zeros_like(p) for p in self.p]
        self.v = [np.zeros_like(p) for p in self.p]
        self.steps = [0] * len(self.p)
        self.wd, self.decoupled, self.betas, self.eps = list(weight_decays), decoupled, betas, eps

    def step(self, grads, lrs):
        for i, g in enumerate(grads):
            if g is None:
                continue
            self.steps[i] += 1
            self.p[i], self.m[i], self.v[i] = R.adam_step(self.p[i], g, self.m[i], self.v[i], self.steps[i], lrs[i],
                                                          self.betas[0], self.betas[1], self.eps, self.wd[i], self.decoupled)


def _fma(a, b, c):
    """float32 fma through float64: the product of two fp32 numbers is exact in double."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def adam_step_f32(p, g, m, v, lr, wd, bc1, bc2s, b1, b2, eps, decoupled, gscale=None):
    """adam_update (csrc/eav_common.h) operation by operation in numpy float32; every argument an fp32 value."""
    p, g, m, v = f32(p).copy(), f32(g).copy(), f32(m), f32(v)
    lr, wd, bc1, bc2s, b1, b2, eps = (np.float32(x) for x in (lr, wd, bc1, bc2s, b1, b2, eps))
    one = np.float32(1.0)
    if gscale is not None:
        g = g * np.float32(gscale)
    if wd != 0:
        if decoupled:
            p = p * _fma(f32(-lr), f32(wd), f32(one))
        else:
            g = _fma(np.full_like(p, wd), p, g)
    m = b1 * m + (one - b1) * g
    v = b2 * v + (one - b2) * g * g
    denom = np.sqrt(v) / bc2s + eps
    assert m.dtype == v.dtype == denom.dtype == np.float32
    return _fma(np.full_like(p, -(lr / bc1)), m / denom, p), m, v


def step_bounds(p0, g, m0, v0, lr, wd, step, b1, b2, eps, decoupled, gscale=None, bc=None):
    """One reference step in float64 from fp32 inputs.  Returns (p_ref, m_ref, v_ref, tol_p, tol_m, tol_v, D), the
    tolerances as the module docstring derives them.  bc: (bc1, bc2s) to use instead of those of `step`."""
    p0, g, m0, v0 = R.f64(p0), R.f64(g), R.f64(m0), R.f64(v0)
    lr, wd, b1, b2, eps = (float(np.float32(x)) for x in (lr, wd, b1, b2, eps))
    if gscale is not None:
        g = g * float(np.float32(gscale))
    pd, ga = p0, np.abs(g)
    if wd != 0.0:
        if decoupled:
            pd = p0 * (1.0 - lr * wd)
        else:
            ga = ga + np.abs(wd * p0)
            g = g + wd * p0
    m = b1 * m0 + (1.0 - b1) * g
    v = b2 * v0 + (1.0 - b2) * g * g
    bc1, bc2s = (1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)) if bc is None else (float(bc[0]), float(bc[1]))
    denom = np.sqrt(v) / bc2s + eps
    p = pd - (lr / bc1) * (m / denom)
    s_m = np.abs(b1 * m0) + (1.0 - b1) * ga
    s_v = np.abs(b2 * v0) + (1.0 - b2) * ga * ga
    d = np.abs(pd - p0) + (lr / bc1) * (s_m / denom)
    return p, m, v, 1.25 * EPS * np.abs(p) + 16 * EPS * d, 4 * EPS * s_m, 4 * EPS * s_v, d


class Trajectory:
    """float64 reference over several steps with the compounded tolerances (module docstring): one instance per tensor."""

    def __init__(self, p0, wd, decoupled, betas=(0.9, 0.999), eps=1e-8):
        self.p = R.f64(p0).copy()
        self.m, self.v = np.zeros_like(self.p), np.zeros_like(self.p)
        self.tol_p, self.tol_m, self.tol_v = (np.zeros_like(self.p) for _ in range(3))
        self.steps, self.wd, self.decoupled, self.betas, self.eps = 0, wd, decoupled, betas, eps

    def step(self, g, lr, gscale=None):
        self.steps += 1
        self.p, self.m, self.v, _, tm, tv, d = step_bounds(self.p, g, self.m, self.v, lr, self.wd, self.steps,
                                                           self.betas[0], self.betas[1], self.eps, self.decoupled, gscale)
        self.tol_p += 1.25 * EPS * np.abs(self.p) + 16 * EPS * self.steps * d
        self.tol_m += tm
        self.tol_v += tv

    def check(self, p, m, v, what):
        for name, got, ref, tol in (("p", p, self.p, self.tol_p), ("m", m, self.m, self.tol_m), ("v", v, self.v, self.tol_v)):
            err = np.abs(R.f64(got).reshape(ref.shape) - ref)
            worst = float(np.max(err / np.maximum(tol, 1e-300)))
            print(f"{what}: {name} worst error / tolerance {worst:.3f} (max error {float(err.max()):.3e})")
            assert np.all(err <= tol), (what, name, worst)
