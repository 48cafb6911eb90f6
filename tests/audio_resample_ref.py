"""Float64 restatement of torchaudio.transforms.Resample (resampling_method "sinc_interp_hann"), independent of the
package: the kernel design of torchaudio.functional._get_sinc_resample_kernel and the dense application of
_apply_sinc_resample_kernel - pad, strided dot product with every stored tap, keep ceil(new * L / orig) outputs."""
import math

import numpy as np


def design(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """(taps float64 [new, 2*width + orig], width, orig, new)."""
    g = math.gcd(int(orig_freq), int(new_freq))
    orig, new = int(orig_freq) // g, int(new_freq) // g
    base = min(orig, new) * rolloff
    width = math.ceil(lowpass_filter_width * orig / base)
    taps = np.empty((new, 2 * width + orig), dtype=np.float64)
    idx = np.arange(-width, width + orig, dtype=np.float64) / orig
    for p in range(new):
        t = (np.float64(-p) / new + idx) * base
        t = np.minimum(np.maximum(t, -lowpass_filter_width), lowpass_filter_width)
        window = np.cos(t * math.pi / lowpass_filter_width / 2) ** 2
        t = t * math.pi
        safe = np.where(t == 0, 1.0, t)
        taps[p] = np.where(t == 0, 1.0, np.sin(safe) / safe) * window * (base / orig)
    return taps, width, orig, new


def design_f32(orig_freq, new_freq, **kw):
    taps, width, orig, new = design(orig_freq, new_freq, **kw)
    return taps.astype(np.float32), width, orig, new


def out_length(length, orig, new):
    return -((-new * int(length)) // orig)


def frames(x, width, orig):
    """[nframes, 2*width + orig] windows of the padded waveform, one per output frame (stride orig)."""
    x = np.asarray(x, dtype=np.float64)
    xp = np.concatenate([np.zeros(width), x, np.zeros(width + orig)])
    nfr = (len(xp) - (2 * width + orig)) // orig + 1
    return np.lib.stride_tricks.sliding_window_view(xp, 2 * width + orig)[::orig][:nfr]


def apply(x, taps, width, orig, new):
    """Dense float64 application: (y [ceil(new*L/orig)], mag = sum_j |tap_j * x_j| per output)."""
    fr = frames(x, width, orig)
    t = np.asarray(taps, dtype=np.float64)
    n = out_length(len(x), orig, new)
    y = (fr @ t.T).reshape(-1)[:n]
    mag = (np.abs(fr) @ np.abs(t).T).reshape(-1)[:n]
    return y, mag


def resample(x, orig_freq, new_freq, taps_dtype=np.float32):
    """Resample(orig_freq, new_freq)(x) for a 1-D waveform, float64 arithmetic on the stored (float32) taps."""
    taps, width, orig, new = design(orig_freq, new_freq)
    if orig == new:
        return np.asarray(x, dtype=np.float64).copy()
    return apply(x, taps.astype(taps_dtype), width, orig, new)[0]
