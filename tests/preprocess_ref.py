"""Plain-numpy references of the pre-processing kernels (eav_amd/csrc/preprocess.hip) and the cases their tests share:
tests/test_preprocess_ref_cpu.py pins the references (to Pillow, scipy and the oracle), tests/test_preprocess_kernels_gpu.py
holds the kernels to them.  Nothing here needs a GPU.

frames    eav_resize_normalize_u8's contract, per channel: Pillow's 8-bit bilinear resampler (precompute_coeffs and
          normalize_coeffs_8bpc of src/libImaging/Resample.c: triangle filter, support max(in / out, 1), float64 weights
          rounded to 22-bit fixed point; horizontal pass rounded to uint8, then the vertical pass), then
          float32(float64(u8) * rescale), a float32 subtraction and a float32 division.
log-mel   eav_ast_fbank's recipe (HF ASTFeatureExtractor, numpy path) in float64 with the window, the mel matrix, the
          pre-emphasis, the floor, the mean and 2 std as parameters, and the per-output bound of the GPU test.
IIR       (a) the direct-form-II-transposed cascade in np.longdouble - the truth; (b) a float64 emulation of the three
          passes of eav_sosfilt_f64 (zero-state chunks, state scan, homogeneous fix-up) for a given chunk length.
The decimating FIR needs no arithmetic of its own: tests/eeg_resample_ref.apply / bound with up = 1."""
import functools

import numpy as np

from tests import eeg_resample_ref as rref

PRECISION_BITS = 32 - 8 - 2

# ------------------------------------------------------------------------------------------------ frames
# (H, W) -> (OH, OW): one pixel in or out, up- and down-scaling by non-integer factors, non-square, 65 taps (224 -> 7),
# and 65 184 bytes of LDS (C * H * OW) at C = 3.  (100, 3) -> (9, 300) needs 90 000 bytes at C = 3, more than the kernel's
# 64 KiB tile: that one combination is a refusal, at C = 1 and 2 it runs
FRAME_SIZES = [((1, 1), (1, 1)), ((1, 1), (5, 7)), ((5, 7), (1, 1)), ((2, 3), (3, 2)), ((7, 9), (20, 31)),
               ((33, 17), (16, 40)), ((64, 48), (32, 24)), ((224, 224), (7, 7)), ((100, 3), (9, 300)),
               ((97, 224), (224, 224))]
LDS_LAST_LEGAL = ((256, 8), (4, 256))       # C = 1: H * OW = 65 536 bytes exactly
NORMS = {"half": ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)), "imagenet": ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))}


def bilinear_coeffs(in_size, out_size):
    """(bounds int32 [out, 2] = (first input, tap count), coeffs int32 [out, ksize]) - one output at a time, as Pillow's
    C loop does."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    coeffs = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        count = min(int(center + support + 0.5), in_size) - xmin
        w = np.array([max(0.0, 1.0 - abs((x + xmin - center + 0.5) / filterscale)) for x in range(count)], np.float64)
        total = w.sum()
        if total != 0.0:
            w = w / total
        coeffs[xx, :count] = [int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
                              for v in w]
        bounds[xx] = (xmin, count)
    return bounds, coeffs


def _pass_u8(plane, bounds, coeffs):
    """One resampling pass along the LAST axis of a uint8 array, rounded to uint8."""
    src = plane.astype(np.int64)
    out = np.zeros(plane.shape[:-1] + (len(bounds),), np.uint8)
    for xx, (first, count) in enumerate(bounds):
        acc = (1 << (PRECISION_BITS - 1)) + (src[..., first:first + count] * coeffs[xx, :count].astype(np.int64)).sum(-1)
        out[..., xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize_u8(plane, out_h, out_w):
    """uint8 [..., H, W] -> uint8 [..., out_h, out_w]: the horizontal pass to uint8, then the vertical pass."""
    H, W = plane.shape[-2:]
    tmp = _pass_u8(plane, *bilinear_coeffs(W, out_w))                                # [..., H, OW]
    return np.swapaxes(_pass_u8(np.swapaxes(tmp, -1, -2), *bilinear_coeffs(H, out_h)), -1, -2)


def frames_ref(frames, size, mean, std, rescale=1.0 / 255.0):
    """uint8 [n, H, W, C] (C in 1..3) -> float32 [n, C, OH, OW], every channel on its own."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim == 4 and 1 <= frames.shape[3] <= 3
    u8 = resize_u8(np.ascontiguousarray(frames.transpose(0, 3, 1, 2)), *size)
    x = (u8.astype(np.float64) * rescale).astype(np.float32)
    m = np.asarray(mean, np.float32)[:frames.shape[3], None, None]
    s = np.asarray(std, np.float32)[:frames.shape[3], None, None]
    return ((x - m) / s).astype(np.float32)


# ------------------------------------------------------------------------------------------------ log-mel
MEL_FLOOR = 1.192092955078125e-07
AST_MEAN, AST_STD = -4.2677393, 4.5689974
FBANK_L = [400, 559, 560, 3000]          # one frame; the last length with one frame / the first with two; 17 frames
FBANK_MAX_LEN = [1, 2, 17, 24]           # truncation, exact fit (L = 560 / 3000) and padding
FBANK_NMEL = [1, 64, 128, 256]


def ulp32(v):
    """Spacing of float32 at |v| (float64 array)."""
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def fbank_ref(wav, max_len, filt, window=None, preemph=0.97, floor=MEL_FLOOR, mean=AST_MEAN, std2=AST_STD * 2):
    """wav float32 [n, L], filt float64 [257, nmel] -> (out float32 [n, max_len, nmel], bound float64 of the same shape).

    Frames of 400 every 160, DC removal, pre-emphasis, window, 512-point real FFT rounded to complex64, |.|^2, mel
    matrix, floor, log rounded to float32, zero padding / truncation to max_len frames, (x - mean) / std2 in float32.
    bound = 2 ((2^-22 + ulp32(log v)) / std2 + ulp32(out)): the mel energy v may move by a relative 2^-22 (each
    complex64-rounded component by one float32 ulp of itself), which moves log v by 2^-22; the float32 log by one ulp of
    itself; the output by one ulp of itself; doubled once for the reference's own roundings.  Padded frames hold an exact
    value: their bound is 0."""
    wav = np.asarray(wav, np.float32)
    window = np.hanning(400).astype(np.float64) if window is None else np.asarray(window, np.float64)
    filt = np.asarray(filt, np.float64)
    nmel = filt.shape[1]
    mean32, std32 = np.float32(mean), np.float32(std2)
    outs, bounds = [], []
    for w in wav:
        x = w.astype(np.float64)
        nfr = 1 + (x.size - 400) // 160
        fr = x[np.arange(400)[None, :] + 160 * np.arange(nfr)[:, None]]
        fr = fr - fr.mean(1, keepdims=True)
        pe = np.empty_like(fr)
        pe[:, 1:] = fr[:, 1:] - preemph * fr[:, :-1]
        pe[:, 0] = fr[:, 0] * (1 - preemph)
        buf = np.zeros((nfr, 512))
        buf[:, :400] = pe * window
        spec = np.fft.rfft(buf, axis=1).astype(np.complex64)
        power = np.abs(spec, dtype=np.float64) ** 2.0
        melspec = np.maximum(floor, filt.T @ power.T)                          # [nmel, nfr]
        logv = np.log(melspec).T                                               # float64 [nfr, nmel]
        fb = logv.astype(np.float32)
        tol = (2.0 ** -22 + ulp32(logv)) / float(std32)
        if nfr < max_len:
            fb = np.concatenate([fb, np.zeros((max_len - nfr, nmel), np.float32)], 0)
            tol = np.concatenate([tol, np.zeros((max_len - nfr, nmel))], 0)
        else:
            fb, tol = fb[:max_len], tol[:max_len]
        out = ((fb - mean32) / std32).astype(np.float32)
        live = (np.arange(max_len) < nfr)[:, None]
        outs.append(out)
        bounds.append(np.where(live, 2.0 * (tol + ulp32(out)), 0.0))
    return np.stack(outs), np.stack(bounds)


def one_hot_filters(first, count):
    """[257, count]: mel row m passes bin first + m alone."""
    filt = np.zeros((257, count))
    filt[first + np.arange(count), np.arange(count)] = 1.0
    return filt


# ------------------------------------------------------------------------------------------------ decimating FIR
DECIMATE_DOWN = [2, 4, 5]


def decimate_lengths(down):
    """One sample; fewer than the taps; the 41 taps of down = 2; 255, 256 and 256 outputs + one sample (the workgroup
    boundary); many workgroups and a ragged last one."""
    return [1, 7, 41, 255 * down, 256 * down, 256 * down + 1, 20011]


def decimate_ref(x, h, down, center):
    """x float64 [nch, n] -> (long-double sum [nch, n_out], per-output bound)."""
    dtype = rref.reference_dtype()
    ref, mag, count = rref.apply(x, h, 1, down, center, dtype)
    return ref, rref.bound(mag, count, dtype)


# ------------------------------------------------------------------------------------------------ IIR
SOS_N = 4099
SOS_NCH = 65                             # the second block of the scan kernel starts at channel 64
SOS_FILTERS = {"5-30": (5, [5, 30]), "0.3-45": (5, [0.3, 45]),           # the bands the loaders use
               "order1": (1, [8, 12]),                                   # one section
               "order8": (8, [5, 30])}                                   # eight sections: the most the kernel takes
# (n, chunk): one sample per chunk; 65 chunks with a ragged last one; an exact multiple (64 chunks); a last chunk of one
# sample (65 chunks); a chunk length that is no power of two; one chunk
SOS_CASES = [(4099, 1), (4099, 64), (4096, 64), (4097, 64), (4099, 257), (4099, 5000)]


@functools.lru_cache(maxsize=None)
def sos_of(name):
    from scipy.signal import butter
    order, band = SOS_FILTERS[name]
    sos = np.ascontiguousarray(butter(order, band, btype="bandpass", fs=100, output="sos"), np.float64)
    sos.setflags(write=False)
    return sos


def sos_cascade(sos, x, dtype):
    """Direct form II transposed, section after section, in `dtype`; x [nch, n] - every channel on its own (the
    channels are only carried side by side: no arithmetic crosses them)."""
    sos = np.asarray(sos, np.float64).astype(dtype)
    x = np.asarray(x).astype(dtype)
    nch, n = x.shape
    z0 = np.zeros((len(sos), nch), dtype)
    z1 = np.zeros((len(sos), nch), dtype)
    y = np.empty((nch, n), dtype)
    for i in range(n):
        v = x[:, i]
        for s, (b0, b1, b2, _, a1, a2) in enumerate(sos):
            o = b0 * v + z0[s]
            z0[s] = b1 * v - a1 * o + z1[s]
            z1[s] = b2 * v - a2 * o
            v = o
        y[:, i] = v
    return y


def sos_truth(sos, x):
    return sos_cascade(sos, x, rref.reference_dtype())


def sos_emulate(sos, x, chunk, tables=None):
    """eav_sosfilt_f64's three passes in float64 (no fma): x float64 [nch, n] -> y [nch, n]."""
    from eav_amd.eeg_data import sos_tables
    sos = np.asarray(sos, np.float64)
    x = np.asarray(x, np.float64)
    nch, n = x.shape
    nsec, ns = len(sos), 2 * len(sos)
    H, AL = sos_tables(sos, chunk) if tables is None else tables
    nchunk = -(-n // chunk)
    xp = np.zeros((nch, nchunk * chunk))
    xp[:, :n] = x
    xp = xp.reshape(nch, nchunk, chunk)
    length = np.minimum(chunk, n - chunk * np.arange(nchunk))                  # samples of every chunk
    # (1) every chunk from a zero state; the state is frozen where a (last) chunk has ended
    z = np.zeros((nsec, 2, nch, nchunk))
    y = np.zeros((nch, nchunk, chunk))
    for k in range(chunk):
        live = (k < length)[None, :]
        v = xp[:, :, k]
        for s, (b0, b1, b2, _, a1, a2) in enumerate(sos):
            o = b0 * v + z[s, 0]
            z[s, 0] = np.where(live, b1 * v - a1 * o + z[s, 1], z[s, 0])
            z[s, 1] = np.where(live, b2 * v - a2 * o, z[s, 1])
            v = o
        y[:, :, k] = v
    zend = z.transpose(2, 3, 0, 1).reshape(nch, nchunk, ns)
    # (2) chunk-start states: zs[q + 1] = zend[q] + AL zs[q], the sum over j in ascending order
    zstart = np.zeros((nch, nchunk, ns))
    zq = np.zeros((nch, ns))
    for q in range(nchunk):
        zstart[:, q] = zq
        a = zend[:, q].copy()
        for j in range(ns):
            a = a + AL[None, :, j] * zq[:, j:j + 1]
        zq = a
    # (3) the homogeneous response of every chunk but the first
    a = np.zeros((nch, nchunk, chunk))
    for j in range(ns):
        a = a + H[None, None, :, j] * zstart[:, :, None, j]
    y[:, 1:] = y[:, 1:] + a[:, 1:]
    return y.reshape(nch, nchunk * chunk)[:, :n]
