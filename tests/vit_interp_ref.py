"""Float64 reference of the ViT position-table resampling (HF ViTEmbeddings.interpolate_pos_encoding: bicubic,
align_corners=False, no antialiasing), written independently of eav_amd.pos_interp: dense per-axis matrices built entry by
entry from the published formula.

Per axis, scale = n_in / n_out, A = -0.75:  s = (o + 0.5) scale - 0.5 (not clamped), i = floor(s), t = s - i, taps at
i-1 .. i+2 with each index clamped to [0, n_in - 1] and the weights
    w0 = ((A (t+1) - 5A)(t+1) + 8A)(t+1) - 4A,   w1 = ((A+2) t - (A+3)) t^2 + 1,   w2 = w1 at 1 - t,   w3 = w0 at 1 - t.
The operator on the [g, g, D] patch rows is (Wy (x) Wx); rows before them (cls) are copied.
"""
import math

import numpy as np

A = -0.75

# (g, ny, nx): down- and up-sampling, non-square, identity along one axis (14 -> 14), a single output, a 2 x 2 source
GRIDS = [(14, 7, 7), (14, 3, 3), (14, 4, 9), (14, 14, 13), (14, 24, 24), (14, 1, 1), (2, 3, 5), (2, 1, 4)]


def _w_outer(x):
    return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A


def _w_inner(x):
    return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0


def axis_matrix(n_in, n_out):
    """[n_out, n_in] float64."""
    m = np.zeros((n_out, n_in), np.float64)
    scale = n_in / n_out
    for o in range(n_out):
        s = (o + 0.5) * scale - 0.5
        i = math.floor(s)
        t = s - i
        for k, wk in zip((i - 1, i, i + 1, i + 2), (_w_outer(t + 1.0), _w_inner(t), _w_inner(1.0 - t), _w_outer(2.0 - t))):
            m[o, min(max(k, 0), n_in - 1)] += wk
    return m


def resample(pos, g, ny, nx, nextra=1):
    """pos [nextra + g g, D] -> float64 [nextra + ny nx, D]."""
    pos = np.asarray(pos, np.float64)
    D = pos.shape[-1]
    Wy, Wx = axis_matrix(g, ny), axis_matrix(g, nx)
    grid = np.einsum("ab,cd,bdk->ack", Wy, Wx, pos[nextra:].reshape(g, g, D)).reshape(ny * nx, D)
    return np.concatenate([pos[:nextra], grid], 0)


def resample_adjoint(dout, g, ny, nx, nextra=1):
    """dout [nextra + ny nx, D] -> float64 [nextra + g g, D]: the transposed operator."""
    dout = np.asarray(dout, np.float64)
    D = dout.shape[-1]
    Wy, Wx = axis_matrix(g, ny), axis_matrix(g, nx)
    grid = np.einsum("ab,cd,ack->bdk", Wy, Wx, dout[nextra:].reshape(ny, nx, D)).reshape(g * g, D)
    return np.concatenate([dout[:nextra], grid], 0)


def error_bounds(x, g, ny, nx, nextra=1, adjoint=False):
    """Elementwise fp32 bound of a resampling of x (the adjoint's with adjoint=True):
    (n + 8) 2^-24 (|Wy| (x) |Wx|) |x|, n = the number of non-zero terms of that output - every weight is a float64 value
    rounded once (relative 2^-24 each, two per term), every product and every addition of the n terms rounds once more;
    the copied rows are exact."""
    x = np.abs(np.asarray(x, np.float64))
    D = x.shape[-1]
    Wy, Wx = np.abs(axis_matrix(g, ny)), np.abs(axis_matrix(g, nx))
    cy, cx = (Wy != 0).astype(np.float64), (Wx != 0).astype(np.float64)
    if adjoint:
        mag = np.einsum("ab,cd,ack->bdk", Wy, Wx, x[nextra:].reshape(ny, nx, D)).reshape(g * g, D)
        n = np.einsum("ab,cd->bd", cy, cx).reshape(g * g, 1)
    else:
        mag = np.einsum("ab,cd,bdk->ack", Wy, Wx, x[nextra:].reshape(g, g, D)).reshape(ny * nx, D)
        n = np.einsum("ab,cd->ac", cy, cx).reshape(ny * nx, 1)
    return np.concatenate([np.zeros((nextra, D)), (n + 8.0) * 2.0 ** -24 * mag], 0)


def frames(seed, B, H, W):
    """(pixel_values [B, 3, H, W] fp32 uniform [-1, 1), labels [B]) from the repository's seeded generators."""
    from eav_amd import synth
    return synth.uniform(seed, (B, 3, H, W), -1.0, 1.0), synth.labels(seed ^ 0x5EED, B)
