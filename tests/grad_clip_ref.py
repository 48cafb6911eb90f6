"""float64 reference arithmetic of the gradient clipping / accumulation tests: the global L2 norm and the clipping
coefficient as torch.nn.utils.clip_grad_norm_ forms them, the Adam / AdamW update as torch.optim forms it, and the weighted
fold of gradient accumulation.  numpy float64 throughout.

tests/test_grad_clip_cpu.py pins this module to torch.nn.utils.clip_grad_norm_ + torch.optim.Adam / AdamW run in float64 on
the CPU; the GPU tests compare the kernels and FusedAdam with it."""
import numpy as np

NORM_RTOL = 4 * 2.0 ** -23      # |norm - ref| <= NORM_RTOL * ref: the fp64 sum is exact to ~n 2^-53, what remains is the
                                # square root and one cast to fp32


def f64(a):
    return np.asarray(a, dtype=np.float64)


def global_norm(grads):
    """sqrt(sum over all tensors of g^2), float64."""
    return float(np.sqrt(sum(float(np.sum(f64(g) ** 2)) for g in grads)))


def clip_coef(norm, max_norm):
    """torch: clip_coef = max_norm / (total_norm + 1e-6), clamped to at most 1."""
    return min(1.0, float(max_norm) / (norm + 1e-6))


def clip(grads, max_norm):
    """(norm before clipping, coefficient, [scaled gradients])"""
    norm = global_norm(grads)
    c = clip_coef(norm, max_norm)
    return norm, c, [f64(g) * c for g in grads]


def coef_f32(norm_f32, max_norm):
    """The coefficient in fp32 arithmetic from an fp32 norm: float32(max_norm) / (norm + float32(1e-6)), clamped to 1 - what
    eav_grad_clip_finish computes from its own out2[0], bit for bit (an IEEE division)."""
    with np.errstate(all="ignore"):
        c = np.float32(max_norm) / (np.float32(norm_f32) + np.float32(1e-6))
    return c if np.isnan(c) else min(np.float32(1.0), c)


def fold(acc, g, weight, first):
    """acc = weight * g (first) or acc + weight * g"""
    return f64(weight) * f64(g) if first else f64(acc) + f64(weight) * f64(g)


def adam_step(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, decoupled=False):
    """One torch.optim.Adam (decoupled False) / AdamW (True) update; step = the count after the increment.
    Returns (p, m, v), float64."""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    if weight_decay != 0.0:
        if decoupled:
            p = p * (1.0 - lr * weight_decay)
        else:
            g = g + weight_decay * p
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    denom = np.sqrt(v) / np.sqrt(bc2) + eps
    return p - (lr / bc1) * (m / denom), m, v


class Stepper:
    """Adam / AdamW over a list of tensors with optional global-norm clipping, float64 state."""

    def __init__(self, params, lr, weight_decay=0.0, decoupled=False, max_grad_norm=None, betas=(0.9, 0.999), eps=1e-8):
        self.betas, self.eps = betas, eps
        self.p = [f64(p).copy() for p in params]
        self.m = [np.zeros_like(p) for p in self.p]
        self.v = [np.zeros_like(p) for p in self.p]
        self.t = 0
        self.lr, self.wd, self.decoupled, self.max_grad_norm = lr, weight_decay, decoupled, max_grad_norm
        self.last_norm = None

    def step(self, grads):
        grads = [f64(g) for g in grads]
        if self.max_grad_norm is not None:
            self.last_norm, _, grads = clip(grads, self.max_grad_norm)
        self.t += 1
        for i, g in enumerate(grads):
            self.p[i], self.m[i], self.v[i] = adam_step(self.p[i], g, self.m[i], self.v[i], self.t, self.lr,
                                                        self.betas[0], self.betas[1], self.eps, self.wd, self.decoupled)
