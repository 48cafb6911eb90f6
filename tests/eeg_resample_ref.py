"""Plain-numpy restatement of scipy.signal.resample_poly(x, up, down, axis=1) in its centred form, the arithmetic that
eav_resample_poly_f64 states (include/eav_hip.h):

    y[c][m] = sum_i h[m*down + center - i*up] * x[c][i]     over 0 <= i < n_in with 0 <= m*down + center - i*up < ntaps
    n_out   = ceil(n_in * up / down),   center = half_len = 10 * max(up, down),   ntaps = 2 * half_len + 1

with h = firwin(ntaps, 1 / max(up, down), window=('kaiser', 5.0)) * up for the gcd-reduced pair.  scipy pads the filter
in front (n_pre_pad) and drops n_pre_remove outputs of upfirdn; as n_pre_remove * down = half_len + n_pre_pad, both
collapse to `center`.  `apply` evaluates the sum in any dtype (np.longdouble for the kernel tests) and returns, per
output, sum_i |h x| and the number of taps n_i - what the rounding bound of the tests is made of."""
import math

import numpy as np


def reduced(up, down):
    g = math.gcd(int(up), int(down))
    return int(up) // g, int(down) // g


def design(up, down):
    """(h float64 [2 half_len + 1] already times up, half_len) as scipy.signal.resample_poly designs it."""
    from scipy.signal import firwin
    up, down = reduced(up, down)
    max_rate = max(up, down)
    half_len = 10 * max_rate
    return firwin(2 * half_len + 1, 1.0 / max_rate, window=("kaiser", 5.0)) * up, half_len


def out_length(n_in, up, down):
    return -(-n_in * up // down)


def tap_ranges(n_in, up, down, ntaps, center):
    """(first input, last input) of every output, int64; last < first where an output has no tap."""
    b = np.arange(out_length(n_in, up, down), dtype=np.int64) * down + center
    lo = b - (ntaps - 1)
    ilo = np.where(lo <= 0, 0, -(-lo // up))
    ihi = np.minimum(n_in - 1, b // up)
    return b, ilo, ihi


def apply(x, h, up, down, center, dtype=np.float64):
    """x [nch, n_in], h [ntaps] -> (y [nch, n_out] in dtype, mag = sum_i |h x| [nch, n_out] float64, n_i [n_out])."""
    x = np.asarray(x)
    nch, n_in = x.shape
    ntaps = len(h)
    b, ilo, ihi = tap_ranges(n_in, up, down, ntaps, center)
    xw, hw = x.astype(dtype), np.asarray(h).astype(dtype)
    y = np.zeros((nch, len(b)), dtype)
    mag = np.zeros((nch, len(b)), dtype)
    count = np.maximum(ihi - ilo + 1, 0)
    for j in range(int(count.max(initial=0))):
        live = np.flatnonzero(j < count)
        i = ilo[live] + j
        term = hw[b[live] - i * up][None, :] * xw[:, i]
        y[:, live] += term
        mag[:, live] += np.abs(term)
    return y, mag.astype(np.float64), count


def bound(mag, count, dtype=np.longdouble):
    """|got - ref| <= (n_i + 2) 2^-53 sum_i |h x| + 1e-300: one rounding per fma, the reference's own rounding and one
    to spare; doubled when the reference itself is only float64 (no wider long double on the platform)."""
    wide = np.finfo(dtype).eps <= 2.0 ** -60
    return (1.0 if wide else 2.0) * (count[None, :] + 2) * 2.0 ** -53 * mag + 1e-300


def reference_dtype():
    return np.longdouble if np.finfo(np.longdouble).eps <= 2.0 ** -60 else np.float64
