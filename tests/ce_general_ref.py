"""Reference of eav_ce_general_fwd_bwd (csrc/head_ce_soft.hip): torch.nn.functional.cross_entropy on the CPU, in float64
(the reference) or float32 (the yardstick of the parity rule), for class-index and class-probability targets, with class
weights and label smoothing.  Labels outside [0, classes) other than -100 are mapped to -100 first: the kernel treats
them as ignored and reports them; torch would raise."""
import numpy as np
import torch
import torch.nn.functional as F

from eav_amd import synth
from tests import kernel_check as kc


def cross_entropy(logits, target, weight, eps, dtype):
    """(loss, d loss / d logits) in `dtype` on the CPU; both NaN-free only where the divisor is non-zero."""
    x = logits.to(dtype).clone().requires_grad_(True)
    if target.dtype == torch.int64:
        NC = logits.shape[1]
        target = torch.where((target >= 0) & (target < NC), target, torch.full_like(target, -100))
    else:
        target = target.to(dtype)
    loss = F.cross_entropy(x, target, weight=None if weight is None else weight.to(dtype), label_smoothing=float(eps))
    loss.backward()
    return loss.detach(), x.grad


def divisor(target, weight, NC):
    """D of the index targets in float64: the weights of the valid labels."""
    ok = (target >= 0) & (target < NC)
    if weight is None:
        return float(ok.sum())
    return float(weight.double()[target[ok]].sum())


def planted_case(B, NC):
    """Logits and labels with the rows test_wide_head_gpu._ce_case plants, at any class count: row 0 two equal maxima with
    the label on the first (a hit), row 1 ignored, row 2 two equal maxima with the label on the second (no hit: the first
    maximum is the arg-maximum), row 3 linspace(-1e4, 1e4) logits (must stay finite), rows 4 and 5 the first and the last
    class.  The tied rows need three classes."""
    s = kc.seed_of("ce-general", B, NC)
    logits = kc.normal(s, (B, NC), 3.0)
    y = torch.from_numpy((synth.splitmix64(s + 1, B) % np.uint64(NC)).astype(np.int64))
    if NC >= 3:
        logits[0, NC // 3], logits[0, NC - 2], y[0] = 50.0, 50.0, NC // 3
    if B > 1:
        y[1] = -100
    if B > 2 and NC >= 3:
        logits[2, 1], logits[2, NC - 1], y[2] = 60.0, 60.0, NC - 1
    if B > 3:
        logits[3] = torch.linspace(-1e4, 1e4, NC)
        y[3] = NC // 2
    if B > 5:
        y[4], y[5] = 0, NC - 1
    return logits, y


def probability_targets(B, NC, seed):
    """Rows of class probabilities: positive, summing to 1 up to fp32 rounding."""
    t = torch.from_numpy(synth.uniform(seed, (B, NC))).double() + 0.05
    return (t / t.sum(1, keepdim=True)).float()


def class_weights(kind, NC, seed):
    """None, random positive weights, or the same with one class (NC // 2) at zero."""
    if kind == "none":
        return None
    w = torch.from_numpy(synth.uniform(seed, (NC,))).float() * 1.5 + 0.25
    if kind == "zero":
        w[NC // 2] = 0.0
    return w
