"""Float64 reference of the AST position-table fit along time, written independently of eav_amd.pos_time: dense [nx, nx0]
matrices built entry by entry from the rule.

The table is [nextra + ny nx0, D], rows frequency-major (nextra + f nx0 + t); the nextra rows are copied, the frequency axis
is untouched, and the time axis follows the length alone:
    nx == nx0   identity
    nx <  nx0   cut:    out[t] = pos[s + t],  s = nx0 // 2 - nx // 2                          (the centre window)
    nx >  nx0   linear: scale = nx0 / nx, src = max((o + 0.5) scale - 0.5, 0), i0 = floor(src), i1 = min(i0 + 1, nx0 - 1),
                        lam = src - i0, weights 1 - lam on i0 and lam on i1   (F.interpolate, bilinear, align_corners=False)
"""
import math

import numpy as np

# (ny, nx0, nx): odd and even cuts, a single output, one short of / one beyond the stored grid, an upsampling by a third,
# the checkpoint's own grid cut to 5 s clips, a 2-column and a 1-column source
GRIDS = [(12, 25, 9), (12, 25, 10), (12, 25, 1), (12, 25, 24), (12, 25, 26), (12, 25, 33), (12, 101, 50), (1, 2, 5), (3, 1, 4)]


def time_matrix(nx0, nx):
    """[nx, nx0] float64."""
    m = np.zeros((nx, nx0), np.float64)
    if nx <= nx0:
        s = nx0 // 2 - nx // 2
        for t in range(nx):
            m[t, s + t] = 1.0
        return m
    scale = nx0 / nx
    for o in range(nx):
        src = max((o + 0.5) * scale - 0.5, 0.0)
        i0 = math.floor(src)
        i1 = min(i0 + 1, nx0 - 1)
        lam = src - i0
        m[o, i0] += 1.0 - lam
        m[o, i1] += lam
    return m


def fit(pos, ny, nx0, nx, nextra=2):
    """pos [nextra + ny nx0, D] -> float64 [nextra + ny nx, D]."""
    pos = np.asarray(pos, np.float64)
    D = pos.shape[-1]
    grid = np.einsum("ts,fsd->ftd", time_matrix(nx0, nx), pos[nextra:].reshape(ny, nx0, D)).reshape(ny * nx, D)
    return np.concatenate([pos[:nextra], grid], 0)


def fit_adjoint(dout, ny, nx0, nx, nextra=2):
    """dout [nextra + ny nx, D] -> float64 [nextra + ny nx0, D]: the transposed operator."""
    dout = np.asarray(dout, np.float64)
    D = dout.shape[-1]
    grid = np.einsum("ts,ftd->fsd", time_matrix(nx0, nx), dout[nextra:].reshape(ny, nx, D)).reshape(ny * nx0, D)
    return np.concatenate([dout[:nextra], grid], 0)


def error_bounds(x, ny, nx0, nx, nextra=2, adjoint=False):
    """Elementwise fp32 bound of a fit of x (the adjoint's with adjoint=True): (n + 8) 2^-24 (|W| |x|), n = the number of
    non-zero terms of that output - every weight is a float64 value rounded once, every product and every addition of the n
    terms rounds once more (derived as vit_interp_ref.error_bounds is).  The copied rows are exact, and so is a cut: its
    only weights are 0 and 1, one term per output, nothing rounds - bound 0."""
    x = np.abs(np.asarray(x, np.float64))
    D = x.shape[-1]
    W = np.abs(time_matrix(nx0, nx))
    cnt = (W != 0).astype(np.float64)
    if adjoint:
        mag = np.einsum("ts,ftd->fsd", W, x[nextra:].reshape(ny, nx, D)).reshape(ny * nx0, D)
        n = np.broadcast_to(cnt.sum(0)[None, :, None], (ny, nx0, 1)).reshape(ny * nx0, 1)
    else:
        mag = np.einsum("ts,fsd->ftd", W, x[nextra:].reshape(ny, nx0, D)).reshape(ny * nx, D)
        n = np.broadcast_to(cnt.sum(1)[None, :, None], (ny, nx, 1)).reshape(ny * nx, 1)
    bound = (n + 8.0) * 2.0 ** -24 * mag
    if nx <= nx0:
        bound = np.zeros_like(bound)
    return np.concatenate([np.zeros((nextra, D)), bound], 0)


def cut_window(nx0, nx):
    """(s, s + nx): the source time indices a cut keeps."""
    s = nx0 // 2 - nx // 2
    return s, s + nx


def clips(seed, B, T, mel=128):
    """(input_values [B, T, mel] fp32, labels [B]) from the repository's seeded generators."""
    from eav_amd import synth
    return synth.mel_batch(seed, B, T, mel)
