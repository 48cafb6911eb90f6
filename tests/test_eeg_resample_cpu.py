"""Rational-rate EEG resampling, host side (no GPU): the filter design against scipy.signal.firwin, the centred formula
that eav_resample_poly_f64 implements (tests/eeg_resample_ref.py) against scipy.signal.resample_poly, the new entry
point's declaration and argument validation, and DataLoadEEG's host logic (rate ratio, windows in seconds, errors)."""
import inspect
import os

import numpy as np
import pytest

from tests import eeg_resample_ref as rref
from eav_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIOS = [(32, 125), (3, 2), (2, 1), (1, 5), (64, 250), (7, 3), (125, 32)]
LENGTHS = [1, 7, 250, 1001]


@pytest.mark.parametrize("up,down", [(32, 125), (3, 2), (2, 1), (125, 32), (64, 250)])
def test_design_equals_scipy_firwin(up, down):
    """Every tap within 1e-15 of scipy's, relative to that tap; (64, 250) gives the bits of (32, 125)."""
    from scipy.signal import firwin
    from eav_amd.eeg_data import resample_poly_design
    h, half_len = resample_poly_design(up, down)
    u, d = rref.reduced(up, down)
    assert half_len == 10 * max(u, d) and h.dtype == np.float64 and h.shape == (2 * half_len + 1,)
    ref = firwin(2 * half_len + 1, 1.0 / max(u, d), window=("kaiser", 5.0)) * u
    assert np.all(ref != 0.0)
    print(f"{up}/{down}: max |h - firwin * up| / |firwin * up| = {float((np.abs(h - ref) / np.abs(ref)).max()):.2e}")
    assert np.all(np.abs(h - ref) <= 1e-15 * np.abs(ref))
    assert np.array_equal(ref, rref.design(up, down)[0])
    if (up, down) == (64, 250):
        assert np.array_equal(h.view(np.uint64), resample_poly_design(32, 125)[0].view(np.uint64))


def test_design_of_pure_decimation_is_unchanged():
    """up == 1 keeps the arithmetic DataLoadEEG has always used: fc sinc(fc m) kaiser(5), normalised to sum 1."""
    from eav_amd.eeg_data import resample_poly_design
    h, half_len = resample_poly_design(1, 5)
    m = np.arange(-50, 51, dtype=np.float64)
    want = 0.2 * np.sinc(0.2 * m) * np.kaiser(101, 5.0)
    want /= want.sum()
    assert half_len == 50 and np.array_equal(h.view(np.uint64), (want * 1).view(np.uint64))
    with pytest.raises(ValueError):
        resample_poly_design(0, 5)


@pytest.mark.parametrize("up,down", RATIOS)
def test_centred_formula_equals_scipy_resample_poly(up, down):
    from scipy.signal import resample_poly
    h, center = rref.design(up, down)
    u, d = rref.reduced(up, down)
    dtype = rref.reference_dtype()
    for n in LENGTHS:
        x = synth.normal(300 + n, (3, n)).astype(np.float64) + 0.5
        want = resample_poly(x, up, down, axis=1)
        ref, mag, count = rref.apply(x, h, u, d, center, dtype)
        assert want.shape == ref.shape == (3, rref.out_length(n, u, d))
        ratio = float((np.abs(want - ref) / rref.bound(mag, count, dtype)).max())
        print(f"{up}/{down}, n {n}: scipy against the centred formula, worst err / bound {ratio:.3f}")
        assert ratio <= 1.0


def test_symbol_is_declared_exported_and_validates_its_arguments():
    from eav_amd import _lib
    header = open(os.path.join(ROOT, "include", "eav_hip.h")).read()
    assert "int eav_resample_poly_f64(const double* x, const double* h, double* y, int nch, int64_t n_in" in header
    assert "eav_resample_poly_f64" in _lib.EXPORTS and len(_lib.SIGNATURES["eav_resample_poly_f64"]) == 11
    assert hasattr(_lib.load(), "eav_resample_poly_f64")
    assert _lib.plain("eav_abi_version") == 3
    ok = (1, 1, 1, 1, 7, 2, 32, 125, 2501, 1250, None)          # n_out = ceil(7 * 32 / 125) = 2; refused before any launch
    bad = {"null": (None,) + ok[1:], "positive": ok[:6] + (0,) + ok[7:], "n_out": ok[:5] + (3,) + ok[6:],
           "center": ok[:9] + (2501, None)}
    for match, args in bad.items():
        with pytest.raises(_lib.EavError, match=match):
            _lib.call("eav_resample_poly_f64", *args)


def test_constructor_keeps_the_reference_arguments_first():
    from eav_amd.eeg_data import DataLoadEEG
    params = inspect.signature(DataLoadEEG.__init__).parameters
    assert list(params)[:6] == ["self", "subject", "band", "fs_orig", "fs_target", "parent_directory"]
    assert [params[k].default for k in list(params)[1:6]] == [1, [0.3, 50], 500, 100, './Datasets/EAV']
    assert params["window_seconds"].kind is inspect.Parameter.KEYWORD_ONLY and params["window_seconds"].default is None
    d = DataLoadEEG()
    assert d.window_seconds is None and d.feature_dev is None


def test_rate_ratio_and_window_arithmetic():
    from eav_amd.eeg_data import DataLoadEEG
    ratio = lambda orig, target: DataLoadEEG(fs_orig=orig, fs_target=target).rate_ratio()  # noqa: E731
    assert ratio(500, 128) == (32, 125) and ratio(500, 128.0) == (32, 125) and ratio(500.0, 100) == (1, 5)
    assert ratio(250, 100) == (2, 5) and ratio(512, 128) == (1, 4) and ratio(1000, 128) == (16, 125)
    assert DataLoadEEG().window_length(2000) == 500 and DataLoadEEG().window_length(10) == 500      # the reference's window
    assert DataLoadEEG(fs_target=128, window_seconds=1).window_length(256) == 128
    assert DataLoadEEG(fs_target=128, window_seconds=2.5).window_length(512) == 320
    assert DataLoadEEG(fs_target=100, window_seconds=0.01).window_length(512) == 1
    assert DataLoadEEG(fs_target=128, window_seconds=2).window_length(256) == 256


def test_windows_shorter_than_a_sample_or_longer_than_a_trial_are_refused():
    import torch
    from eav_amd.eeg_data import DataLoadEEG
    for seconds in (0.001, 3):
        d = DataLoadEEG(fs_target=128, window_seconds=seconds, device="cpu")
        d.seg_f, d.label = torch.zeros(2, 256, 3, dtype=torch.float64), np.eye(10, 3, dtype=np.int64)
        with pytest.raises(ValueError, match="window_seconds"):
            d.segment_and_select_classes()
        assert d.seg_f_div is None and d.feature_dev is None


def test_trials_that_do_not_resample_to_whole_samples_are_refused():
    from eav_amd.eeg_data import DataLoadEEG
    d = DataLoadEEG(fs_orig=500, fs_target=128, device="cpu")
    d.seg = np.zeros((2, 1001, 3))
    with pytest.raises(ValueError, match=r"t = 1001.*32 / 125"):
        d.downsampling()


def test_window_segmentation_on_the_host_tensor():
    """window_seconds = 1 at 128 Hz on a CPU tensor: the reference's F-order split, 128 samples a window."""
    import torch
    from eav_amd.eeg_data import DataLoadEEG
    seg_f = synth.normal(41, (3, 300, 4)).astype(np.float64)
    label = np.zeros((10, 4), np.int64)
    label[[1, 2, 9, 5], np.arange(4)] = 1
    d = DataLoadEEG(fs_target=128, window_seconds=1, device="cpu", remap_labels=True)
    d.seg_f, d.label = torch.from_numpy(seg_f), label
    d.segment_and_select_classes()
    keep = [0, 2, 3]                                            # classes 1, 9, 5 are listening classes; 2 is not
    want = np.stack([seg_f[:, w * 128:(w + 1) * 128, tr] for tr in keep for w in range(2)])
    assert np.array_equal(d.seg_f_div, want) and list(d.label_div) == [0, 0, 4, 4, 2, 2]
    assert d.feature_dev.dtype == torch.float32 and np.array_equal(d.feature_dev.numpy(), want.astype(np.float32))
