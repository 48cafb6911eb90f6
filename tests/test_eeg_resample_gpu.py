"""eav_resample_poly_f64, eeg_data.resample and DataLoadEEG at a non-dividing rate on the MI355X.

Kernel: against the centred formula of tests/eeg_resample_ref.py evaluated in np.longdouble on the same float64 taps,
per output within

    |got - ref| <= (n_i + 2) * 2^-53 * sum_i |h x| + 1e-300,        n_i = that output's tap count

(one rounding per fma, the reference's own rounding and one to spare; doubled if the platform's long double is no wider
than float64; nothing tuned).  Outputs land in NaN-sentinel buffers with a guard band (tests/kernel_check.py).
Class: 500 -> 128 Hz against the scipy chain on the host, stage by stage, within the 1e-9 * max(1, max|ref|) that the
sosfilt test of this kernel uses; 500 -> 100 Hz reproduces the decimating path bit for bit."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import eeg_resample_ref as rref
from tests import kernel_check as kc
from eav_amd import _lib, eeg_data as ed, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIOS = [(32, 125), (3, 2), (2, 1), (125, 32), (7, 3), (1, 5)]
LENGTHS = [1, 7, 250, 20011]          # one sample; fewer samples than taps; one workgroup or a few; many and a ragged one
NCH = 3
# where the taps / the workgroup's input tile live (LDS or global memory) beyond the (LDS, LDS) of the ratios above
OTHER_PATHS = [((3, 1024), 5000, "taps global, samples global"), ((1024, 3), 50, "taps global, samples LDS"),
               ((1, 400), 5000, "taps LDS, samples global")]


@functools.lru_cache(maxsize=None)
def case(up, down, n_in):
    """(x [NCH, n_in], h, center, long-double reference, per-output bound) - computed once, shared, read-only."""
    h, center = ed.resample_poly_design(up, down)
    x = synth.normal(kc.seed_of(up, down, n_in), (NCH, n_in)).astype(np.float64) + 0.25
    dtype = rref.reference_dtype()
    ref, mag, count = rref.apply(x, h, up, down, center, dtype)
    bound = rref.bound(mag, count, dtype)
    for a in (x, h, ref, bound):
        a.setflags(write=False)
    return x, h, center, ref, bound


def launch(x, h, up, down, center):
    """The raw entry point into a sentinel-filled buffer: every output written, nothing past the end."""
    nch, n_in = x.shape
    n_out = rref.out_length(n_in, up, down)
    xd, hd = kc.dev(x), kc.dev(h)
    buf = kc.sentinel_buf(2 * nch * n_out)                      # float32 words: two per float64 output
    _lib.call("eav_resample_poly_f64", xd.data_ptr(), hd.data_ptr(), buf.data_ptr(), nch, n_in, n_out, up, down, len(h),
              center, _lib.stream_ptr())
    words = kc.take(buf, 2 * nch * n_out, (2 * nch * n_out,), f"resample {up}/{down}, n {n_in}")
    return words.view(torch.float64).view(nch, n_out).numpy()


def check(got, ref, bound, what):
    assert got.shape == ref.shape and got.dtype == np.float64, (what, got.shape, ref.shape)
    err = np.abs(got.astype(ref.dtype) - ref).astype(np.float64)
    worst = float((err / bound).max())
    print(f"{what}: max |err| {err.max():.3e}, worst err / bound {worst:.3f}")
    assert np.all(err <= bound), (what, worst)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("n_in", LENGTHS)
@pytest.mark.parametrize("up,down", RATIOS)
def test_kernel_within_the_rounding_bound(up, down, n_in):
    x, h, center, ref, bound = case(up, down, n_in)
    got = launch(x, h, up, down, center)
    check(got, ref, bound, f"kernel {up}/{down}, n {n_in}")
    again = launch(x, h, up, down, center)
    assert same_bits(got, again), "two runs differ"
    through = ed.resample(torch.from_numpy(x).cuda(), up, down)
    assert through.is_cuda and through.dtype == torch.float64 and tuple(through.shape) == ref.shape
    if up == 1:                                                  # resample sends pure decimation to the decimating kernel
        check(through.cpu().numpy(), ref, bound, f"resample {up}/{down}, n {n_in}")
    else:
        assert same_bits(through.cpu().numpy(), got)


@pytest.mark.parametrize("ratio,n_in,where", OTHER_PATHS)
def test_tables_and_tiles_that_do_not_fit_lds(ratio, n_in, where):
    up, down = ratio
    x, h, center, ref, bound = case(up, down, n_in)
    assert (len(h) > 8192) == where.startswith("taps global")
    got = launch(x, h, up, down, center)
    check(got, ref, bound, f"kernel {up}/{down}, n {n_in} ({where})")
    assert same_bits(got, launch(x, h, up, down, center))
    if up != 1:
        assert same_bits(ed.resample(torch.from_numpy(x).cuda(), up, down).cpu().numpy(), got)


@pytest.mark.parametrize("up,down", [(32, 125), (125, 32), (3, 2)])
def test_an_impulse_reads_the_taps_back(up, down):
    h, center = ed.resample_poly_design(up, down)
    n_in = 700
    for pos in (0, 333, n_in - 1):
        x = np.zeros((1, n_in))
        x[0, pos] = 1.0
        k = np.arange(rref.out_length(n_in, up, down), dtype=np.int64) * down + center - pos * up
        want = np.where((k >= 0) & (k < len(h)), h[np.clip(k, 0, len(h) - 1)], 0.0)
        assert np.count_nonzero(want) > 0
        got = launch(x, h, up, down, center)[0]
        assert np.array_equal(got, want), (up, down, pos)


def test_unreduced_ratio_and_pure_decimation_give_the_same_bits():
    """An unreduced ratio is reduced before the design (64/250 gives the bits of 32/125; 3/15 is the 101-tap filter of
    1/5, not a 301-tap one).  Pure decimation has two kernels: eav_decimate_fir_f64 (`decimate`, where `resample` sends
    up == 1) walks the taps upwards, i.e. the samples downwards, and eav_resample_poly_f64 (`resample_kernel`) walks the
    samples upwards.  The orders differ, so the bits do (on the MI355X 10 451 of 12 009 outputs at 1/5, by 1.8e-15 at
    most): what holds is that both lie within the rounding bound of the long-double sum."""
    x = torch.from_numpy(case(32, 125, 20011)[0]).cuda()
    assert same_bits(ed.resample(x, 64, 250).cpu().numpy(), ed.resample(x, 32, 125).cpu().numpy())
    host, _, _, ref, bound = case(1, 5, 20011)
    x = torch.from_numpy(host).cuda()
    check(ed.decimate(x, 5).cpu().numpy(), ref, bound, "decimate by 5")
    check(ed.resample_kernel(x, 1, 5).cpu().numpy(), ref, bound, "resample_kernel 1/5")
    check(ed.resample(x, 3, 15).cpu().numpy(), ref, bound, "resample 3/15")
    assert ed.resample(x, 7, 7) is x


# ------------------------------------------------------------------------------------------------ the class
CH, T, TRI = 30, 1000, 12            # 2 s trials at 500 Hz


@functools.lru_cache(maxsize=None)
def recording():
    """[30, 1000, 12] float64: noise, an offset and a 10 Hz component; two trials of each listening class and two others."""
    x = synth.normal(811, (CH, T, TRI)).astype(np.float64)
    tt = np.arange(T, dtype=np.float64)[None, :, None] / 500.0
    x += 1.5 + 2.0 * np.sin(2 * np.pi * 10.0 * tt + np.arange(CH)[:, None, None])
    label = np.zeros((10, TRI), np.int64)
    label[[1, 4, 3, 5, 7, 9, 9, 0, 1, 3, 5, 7], np.arange(TRI)] = 1
    x.setflags(write=False)
    label.setflags(write=False)
    return x, label


@functools.lru_cache(maxsize=None)
def scipy_chain():
    """The reference's chain on the host at 500 -> 128 Hz with 1 s windows: (seg, seg_f, seg_f_div, label_div)."""
    from scipy import signal
    x, label = recording()
    tm = np.reshape(x, [CH, T * TRI], order='F')
    seg = np.reshape(signal.resample_poly(tm, 32, 125, axis=1), [CH, 256, TRI], order='F')
    sos = signal.butter(5, [5, 30], btype='bandpass', fs=128, output='sos')
    seg_f = signal.sosfilt(sos, np.reshape(seg, [CH, 256 * TRI], order='F'), axis=1).reshape((CH, 256, TRI), order='F')
    div = seg_f.reshape((CH, 128, 2, TRI), order='F').reshape((CH, 128, 2 * TRI), order='F')
    label_div = np.repeat(label, repeats=2, axis=1)
    mask = np.isin(np.argmax(label_div, axis=0), [1, 3, 5, 7, 9])
    return seg, seg_f, np.transpose(div[:, :, mask], (2, 0, 1)), np.argmax(label_div[:, mask], axis=0)


def close(got, ref, what):
    tol = 1e-9 * max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(got - ref).max())
    print(f"{what}: max |err| {err:.3e} (bound {tol:.3e})")
    assert got.shape == ref.shape and err <= tol, (what, err)


def check_class_outputs(d):
    seg, seg_f, div, label_div = scipy_chain()
    close(d.seg.cpu().numpy(), seg, "seg")
    close(d.seg_f.cpu().numpy(), seg_f, "seg_f")
    assert d.seg_f_div.dtype == np.float64 and d.seg_f_div.shape == (20, CH, 128)
    close(d.seg_f_div, div, "seg_f_div")
    assert d.label_div.dtype == np.int64 and np.array_equal(d.label_div, (label_div - 1) // 2)
    assert d.feature_dev.is_cuda and d.feature_dev.dtype == torch.float32
    assert np.array_equal(d.feature_dev.cpu().numpy().view(np.uint32), d.seg_f_div.astype(np.float32).view(np.uint32))


def test_class_at_500_to_128_hz_against_the_scipy_chain():
    x, label = recording()
    d = ed.DataLoadEEG(subject=1, band=[5, 30], fs_orig=500, fs_target=128, remap_labels=True, window_seconds=1)
    d.seg, d.label = x, label
    d.downsampling()
    assert tuple(d.seg.shape) == (CH, 256, TRI)
    d.bandpass_filter()
    d.segment_and_select_classes()
    check_class_outputs(d)
    first = d.seg.cpu().numpy()
    d.fs_target, d.seg = 128.0, x                                # a float rate takes the same path
    d.downsampling()
    assert same_bits(d.seg.cpu().numpy(), first)


def test_class_at_500_to_100_hz_keeps_the_decimating_path_bit_for_bit():
    """fs_target = 100, window_seconds = None on a recording of 5 s trials: every stage equals the kernels of the
    decimating path (decimate, sosfilt) and the reference's 500-sample window, bit for bit."""
    from scipy import signal
    ch, t, tri = 30, 2500, 6
    x = synth.normal(812, (ch, t, tri)).astype(np.float64) + 1.5
    label = np.zeros((10, tri), np.int64)
    label[[1, 4, 3, 9, 0, 5], np.arange(tri)] = 1
    d = ed.DataLoadEEG(subject=1, band=[5, 30], fs_orig=500, fs_target=100)
    d.seg, d.label = x, label
    d.downsampling()
    tm = torch.from_numpy(x).cuda().permute(0, 2, 1).reshape(ch, tri * t).contiguous()
    down = ed.decimate(tm, 5)
    want_seg = down.reshape(ch, tri, 500).permute(0, 2, 1).contiguous()
    assert torch.equal(d.seg.view(torch.int64), want_seg.view(torch.int64))
    d.bandpass_filter()
    sos = signal.butter(5, [5, 30], btype='bandpass', fs=100, output='sos')
    want_f = ed.sosfilt(sos, down).reshape(ch, tri, 500).permute(0, 2, 1).contiguous()
    assert torch.equal(d.seg_f.view(torch.int64), want_f.view(torch.int64))
    d.segment_and_select_classes()
    keep = [0, 2, 3, 5]                                          # classes 1, 3, 9, 5
    assert d.window_seconds is None and d.seg_f_div.shape == (4, ch, 500) and d.seg_f_div.dtype == np.float64
    assert same_bits(d.seg_f_div, want_f.cpu().numpy()[:, :, keep].transpose(2, 0, 1))
    assert list(d.label_div) == [1, 3, 9, 5]
    assert np.array_equal(d.feature_dev.cpu().numpy().view(np.uint32), d.seg_f_div.astype(np.float32).view(np.uint32))
    # and against scipy, within the bound of the class test above
    ref = signal.sosfilt(sos, signal.resample_poly(np.reshape(x, [ch, t * tri], order='F'), 1, 5, axis=1), axis=1)
    close(d.seg_f.cpu().numpy(), ref.reshape((ch, 500, tri), order='F'), "seg_f at 100 Hz")


# ------------------------------------------------------------------------------------------------ files and the driver
@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from scipy.io import savemat
    x, label = recording()
    root = tmp_path_factory.mktemp("eav")
    folder = root / "subject01" / "EEG"
    folder.mkdir(parents=True)
    savemat(str(folder / "subject01_eeg.mat"), {"seg1": np.swapaxes(x, 0, 1)})           # stored [time, channel, trial]
    savemat(str(folder / "subject01_eeg_label.mat"), {"label": label})
    return str(root)


def test_prepare_data_reads_the_recording_from_disk(dataset):
    d = ed.DataLoadEEG(subject=1, band=[5, 30], fs_orig=500, fs_target=128, parent_directory=dataset, remap_labels=True,
                       window_seconds=1)
    feature, labels = d.prepare_data()
    assert feature is d.seg_f_div and labels is d.label_div
    check_class_outputs(d)


def test_driver_trains_from_the_dataset_folder(dataset):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "run_eeg_subjects.py"), "--eeg-root", dataset, "--subjects", "1",
           "--epochs", "1", "--fs-target", "128", "--window-seconds", "1", "--kern-length", "64", "--quiet"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["subjects"] == 1 and line["world"] == 1 and 0.0 <= line["mean_test_acc"] <= 1.0
