"""DataLoadEEG on MI355X - the reference's EEG pre-processing class (Dataload_eeg.py:35-160), same
constructor, methods and outputs, with the two data-heavy stages on the GPU in float64:

    downsampling()      scipy.signal.resample_poly(x, up, down), up/down = fs_target/fs_orig reduced
                        -> eav_decimate_fir_f64 (up == 1) / eav_resample_poly_f64 (any other ratio)
    bandpass_filter()   butter(5, band, 'bandpass', output='sos') + sosfilt    -> eav_sosfilt_f64

Filter *design* (Kaiser-windowed sinc of 20 max(up, down) + 1 taps; 5th-order Butterworth sections) stays on the host - it is a
few hundred flops - and follows scipy's published formulas (firwin / resample_poly, butter via scipy itself,
which is the reference's own dependency, requirements.txt).  `prepare_data()` returns what the reference
returns: (seg_f_div float64 [N, ch, 500], label_div int64 [N]); labels keep the reference's values
(argmax over the 10 one-hot rows, i.e. 1,3,5,7,9 - SURVEY Q8); `remap_labels=True` maps them to 0..4.
`window_seconds` (keyword only) gives the windows in seconds instead of the reference's fixed 500 samples, and
`feature_dev` keeps the selected windows on the device as float32 [N, ch, win] for the trainers.
"""
from __future__ import annotations

import math
import os
from fractions import Fraction

import numpy as np
import torch

from . import _lib

SELECTED_CLASSES = [1, 3, 5, 7, 9]


def read_subject_recording(parent_directory, subject):
    """(signal [channel, time, trial], one-hot labels [10, trial]) of one subject, or None when the signal file is
    absent.  Host file I/O, outside the accelerated path."""
    from scipy.io import loadmat
    stem = f'subject{int(subject):02d}'
    folder = os.path.join(parent_directory, stem, 'EEG')
    signal_path, label_path = (os.path.join(folder, stem + suffix) for suffix in ('_eeg.mat', '_eeg_label.mat'))
    if not os.path.isfile(signal_path):
        return None
    contents = loadmat(signal_path)
    recording = next((np.asarray(contents[name]) for name in ('seg1', 'seg') if name in contents), None)
    if recording is None:
        raise KeyError(f"{signal_path}: neither 'seg1' nor 'seg' present")
    labels = np.asarray(loadmat(label_path)['label'])
    return np.swapaxes(recording, 0, 1), labels          # stored time-major -> channel-major


def resample_poly_design(up, down):
    """(h float64 already times up, center = half_len) of scipy.signal.resample_poly(x, up, down), up / down reduced by
    their gcd: y[m] = sum_i h[m*down + center - i*up] x[i]  (window ('kaiser', 5.0), half_len = 10*max(up,down))."""
    up, down = int(up), int(down)
    if up < 1 or down < 1:
        raise ValueError(f"resample_poly_design: up {up} and down {down} must be positive")
    g = math.gcd(up, down)
    up, down = up // g, down // g
    max_rate = max(up, down)
    half_len = 10 * max_rate
    m = np.arange(-half_len, half_len + 1, dtype=np.float64)
    fc = 1.0 / max_rate
    h = fc * np.sinc(fc * m) * np.kaiser(2 * half_len + 1, 5.0)      # scipy.signal.firwin(..., window=('kaiser',5))
    h /= h.sum()
    return h * up, half_len


def sos_tables(sos, Lc):
    """H [Lc, 2 nsec] (cascade output at step k from unit initial state j, zero input) and
    AL [2 nsec, 2 nsec] (state after Lc zero-input steps), float64 - simulated with scipy's own recurrence."""
    sos = np.asarray(sos, np.float64)
    nsec = sos.shape[0]
    ns = 2 * nsec
    z = np.zeros((ns, nsec, 2))
    for j in range(ns):
        z[j, j // 2, j % 2] = 1.0
    H = np.zeros((Lc, ns))
    for k in range(Lc):
        v = np.zeros(ns)
        for s in range(nsec):
            b0, b1, b2, _, a1, a2 = sos[s]
            o = b0 * v + z[:, s, 0]
            z[:, s, 0] = b1 * v - a1 * o + z[:, s, 1]
            z[:, s, 1] = b2 * v - a2 * o
            v = o
        H[k] = v
    AL = z.reshape(ns, ns).T.copy()            # column j = final state started from e_j
    return H, AL


def decimate(x_dev, down):
    """x_dev float64 device [nch, n] -> [nch, ceil(n/down)] (resample_poly(x, 1, down, axis=1))."""
    h, center = resample_poly_design(1, down)
    nch, n = x_dev.shape
    n_out = n // down + bool(n % down)
    hd = torch.from_numpy(h).to(x_dev.device)
    y = torch.empty(nch, n_out, dtype=torch.float64, device=x_dev.device)
    _lib.call("eav_decimate_fir_f64", x_dev.data_ptr(), hd.data_ptr(), y.data_ptr(), nch, n, n_out, down, len(h), center,
              _lib.stream_ptr())
    torch.cuda.current_stream().synchronize()
    return y


def resample(x_dev, up, down):
    """x_dev float64 device [nch, n] -> [nch, ceil(n*up/down)] (resample_poly(x, up, down, axis=1)); up == down returns
    the input itself, up == 1 (after the gcd) is `decimate`."""
    up, down = int(up), int(down)
    if up < 1 or down < 1:
        raise ValueError(f"resample: up {up} and down {down} must be positive")
    g = math.gcd(up, down)
    up, down = up // g, down // g
    if up == down:
        return x_dev
    if up == 1:
        return decimate(x_dev, down)
    return resample_kernel(x_dev, up, down)


def resample_kernel(x_dev, up, down):
    """eav_resample_poly_f64 for a reduced up / down (any, up == 1 included - `resample` sends that to `decimate`)."""
    h, center = resample_poly_design(up, down)
    nch, n = x_dev.shape
    n_out = -(-n * up // down)
    hd = torch.from_numpy(h).to(x_dev.device)
    y = torch.empty(nch, n_out, dtype=torch.float64, device=x_dev.device)
    _lib.call("eav_resample_poly_f64", x_dev.data_ptr(), hd.data_ptr(), y.data_ptr(), nch, n, n_out, up, down, len(h), center,
              _lib.stream_ptr())
    torch.cuda.current_stream().synchronize()
    return y


def sosfilt(sos, x_dev, chunk=2048):
    """scipy.signal.sosfilt(sos, x, axis=-1) for x float64 device [nch, n]."""
    sos = np.ascontiguousarray(sos, np.float64)
    nsec = sos.shape[0]
    nch, n = x_dev.shape
    Lc = int(chunk)
    H, AL = sos_tables(sos, Lc)
    dev = x_dev.device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    sd, Hd, ALd = t(sos), t(H), t(AL)
    nchunk = (n + Lc - 1) // Lc
    zend = torch.empty(nch, nchunk, 2 * nsec, dtype=torch.float64, device=dev)
    zstart = torch.empty_like(zend)
    y = torch.empty_like(x_dev)
    _lib.call("eav_sosfilt_f64", x_dev.data_ptr(), y.data_ptr(), sd.data_ptr(), Hd.data_ptr(), ALd.data_ptr(),
              zend.data_ptr(), zstart.data_ptr(), nch, n, nsec, Lc, _lib.stream_ptr())
    torch.cuda.current_stream().synchronize()
    return y


class DataLoadEEG:
    def __init__(self, subject=1, band=[0.3, 50], fs_orig=500, fs_target=100, parent_directory='./Datasets/EAV',
                 device=None, remap_labels=False, *, window_seconds=None):
        self.subject = subject
        self.band = band
        self.fs_orig = fs_orig
        self.fs_target = fs_target
        self.parent_directory = parent_directory
        self.device = torch.device(device if device else ("cuda" if torch.cuda.is_available() else "cpu"))
        self.remap_labels = remap_labels
        self.window_seconds = window_seconds
        self.seg = None
        self.label = None
        self.seg_f = None
        self.seg_f_div = None
        self.label_div = None
        self.feature_dev = None

    def _dev(self, a):
        if self.device.type != "cuda":
            raise _lib.EavError("eav_amd.DataLoadEEG runs its filters on an MI355X (no CPU fallback)")
        return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(self.device)

    def load_mat_data(self):
        """Reads one subject's recording from disk (the file layout Dataload_eeg.py:54-83 expects:
        <parent>/subjectNN/EEG/subjectNN_eeg.mat with variable `seg1` or `seg` [time, channel, trial] and
        subjectNN_eeg_label.mat with `label` [10, trials]); leaves self.seg as [channel, time, trial]."""
        found = read_subject_recording(self.parent_directory, self.subject)
        tag = f'subject{self.subject:02d}'
        if found is None:
            print(f'[Error] EEG data not found for {tag}')
            return
        self.seg, self.label = found
        print(f'[Info] Loaded EEG data for {tag}')

    def rate_ratio(self):
        """(up, down) = fs_target / fs_orig in lowest terms; float rates such as 128.0 are accepted."""
        ratio = Fraction(self.fs_target).limit_denominator(1000) / Fraction(self.fs_orig).limit_denominator(1000)
        if ratio <= 0:
            raise ValueError(f"DataLoadEEG: fs_target {self.fs_target} / fs_orig {self.fs_orig} is not a positive rate ratio")
        return ratio.numerator, ratio.denominator

    def window_length(self, t):
        """Samples per window for trials of t samples: the reference's 500, or round(window_seconds * fs_target)."""
        if self.window_seconds is None:
            return 500
        win = int(round(self.window_seconds * self.fs_target))
        if win < 1 or win > t:
            raise ValueError(f"DataLoadEEG: window_seconds = {self.window_seconds} is {win} samples at {self.fs_target} Hz; "
                             f"it must be at least one sample and at most a trial ({t} samples)")
        return win

    def downsampling(self):
        # Dataload_eeg.py:85-102
        if self.seg is None:
            return
        ch, t, tri = self.seg.shape
        up, down = self.rate_ratio()
        if up != 1 and t * up % down:
            raise ValueError(f"DataLoadEEG.downsampling: trials of t = {t} samples do not resample to a whole number of "
                             f"samples at up / down = {up} / {down} (t * up must be a multiple of down)")
        seg = self._dev(self.seg)
        tm = seg.permute(0, 2, 1).reshape(ch, tri * t).contiguous()       # == np.reshape(seg, [ch, t*tri], order='F')
        if up == 1:                                                       # the reference's own arithmetic
            tm2 = decimate(tm, int(self.fs_orig / self.fs_target))
            new_time = int(t * (self.fs_target / self.fs_orig))
        else:
            tm2 = resample(tm, up, down)                                  # tri * t * up / down samples, exactly
            new_time = t * up // down
        self.seg = tm2.reshape(ch, tri, new_time).permute(0, 2, 1).contiguous()   # order='F' reshape back

    def bandpass_filter(self):
        # Dataload_eeg.py:104-121
        if self.seg is None:
            return
        from scipy.signal import butter
        seg = self.seg if isinstance(self.seg, torch.Tensor) else self._dev(self.seg)
        ch, t, tri = seg.shape
        dat = seg.permute(0, 2, 1).reshape(ch, tri * t).contiguous()
        sos = butter(5, self.band, btype='bandpass', fs=self.fs_target, output='sos')
        fdat = sosfilt(sos, dat)
        self.seg_f = fdat.reshape(ch, tri, t).permute(0, 2, 1).contiguous()

    def segment_and_select_classes(self):
        # Dataload_eeg.py:123-152 (20 s trials -> 4 x 5 s windows, listening classes only)
        if self.seg_f is None:
            return
        ch, t, tri = self.seg_f.shape
        win = self.window_length(t)
        nwin = t // win
        # tm1[c, a, b, d] = seg_f[c, a + win*b, d]; flattened F-order over (b, d): index b + nwin*d
        tm1 = self.seg_f[:, :win * nwin, :].reshape(ch, nwin, win, tri).permute(0, 2, 1, 3)     # [c, a, b, d]
        seg_div = tm1.permute(0, 1, 3, 2).reshape(ch, win, tri * nwin)                           # [c, a, d*nwin + b]
        label_div = np.repeat(self.label, repeats=nwin, axis=1)
        cls = np.argmax(label_div, axis=0)
        mask = np.isin(cls, SELECTED_CLASSES)
        idx = torch.from_numpy(np.flatnonzero(mask)).to(seg_div.device)
        data_subset = seg_div.index_select(2, idx)
        selected = data_subset.permute(2, 0, 1).contiguous()
        self.seg_f_div = selected.cpu().numpy()
        self.feature_dev = selected.float()                 # == seg_f_div.astype(float32), resident for the trainers
        lab = np.argmax(label_div[:, mask], axis=0)
        self.label_div = (lab - 1) // 2 if self.remap_labels else lab

    def prepare_data(self):
        self.load_mat_data()
        self.downsampling()
        self.bandpass_filter()
        self.segment_and_select_classes()
        return self.seg_f_div, self.label_div

    data_prepare = prepare_data      # the name the EEGNet driver calls (EEGNet_tor.py:149)
