"""eav_resample_sinc_f32 and DataLoadAudio on the MI355X: the kernel against the float64 restatement of torchaudio's
resampler applied to the same float32 taps (tests/audio_resample_ref.py), per output within

    |got - ref| <= (n_eff + 2) * 2^-24 * sum_j |tap_j * x_j| + 1e-30,     n_eff = taps of that phase above 1e-30

(one rounding per fmaf of the n_eff products that are not exactly zero, the reference's own rounding and one to spare;
sum_j |tap_j x_j| is computed per output, nothing is tuned), and the class against the golden of the reference class."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import audio_data_util as util
from tests import audio_resample_ref as rref
from eav_amd import _lib, synth
from eav_amd.preprocess import resample_waveforms, waveforms_to_input_values

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "audio_load.npz")
EPS = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def design(rate):
    taps, width, orig, new = rref.design_f32(rate, 16000)
    n_eff = (np.abs(taps) > 1e-30).sum(1)
    return taps, width, orig, new, n_eff


@functools.lru_cache(maxsize=None)
def case(rate, length, seed):
    """(x float32 [length], float64 reference, per-output bound) - computed once, shared, never modified."""
    taps, width, orig, new, n_eff = design(rate)
    x = synth.normal(seed, (length,), 0.0, 0.3)
    y, mag = rref.apply(x, taps, width, orig, new)
    bound = (n_eff[np.arange(len(y)) % new] + 2) * EPS * mag + 1e-30
    for a in (x, y, bound):
        a.setflags(write=False)
    return x, y, bound


def check(got, ref, bound, what):
    got = got.double().cpu().numpy()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    worst = float((err / bound).max())
    print(f"{what}: max |err| {err.max():.3e}, worst err / bound {worst:.3f}")
    assert np.all(err <= bound), (what, worst)


@pytest.mark.parametrize("rate", [44100, 48000, 22050, 8000, 11025])
def test_every_ratio_single_row(rate):
    x, ref, bound = case(rate, 2999, 21)
    y = resample_waveforms(x, rate, 16000)
    assert y.shape == (1, len(ref)) and y.dtype == torch.float32 and y.is_cuda
    check(y[0], ref, bound, f"{rate} -> 16000, L 2999")


@pytest.mark.parametrize("length", [5, 441, 442, 50021])
def test_lengths_around_the_frame_and_the_tile(length):
    """L < width, one frame, one frame plus a sample, seven full workgroup tiles plus a ragged one."""
    x, ref, bound = case(44100, length, 22)
    check(resample_waveforms(x, 44100, 16000)[0], ref, bound, f"441/160, L {length}")


def test_rows_of_different_lengths_in_one_launch():
    lengths = [50021, 442, 5]
    batch = np.zeros((3, max(lengths)), np.float32)
    for i, n in enumerate(lengths):
        batch[i, :n] = case(44100, n, 22)[0]
    y, out_lengths = resample_waveforms(batch, 44100, 16000, lengths=lengths)
    assert y.shape == (3, rref.out_length(max(lengths), 441, 160))
    assert list(out_lengths) == [rref.out_length(n, 441, 160) for n in lengths] and out_lengths.dtype == np.int64
    for i, n in enumerate(lengths):
        _, ref, bound = case(44100, n, 22)
        check(y[i, :int(out_lengths[i])], ref, bound, f"row {i} of 3, L {n}")


def test_guard_bands_stay_untouched_and_two_runs_agree_bit_for_bit():
    lengths = [50021, 442, 5]
    taps, width, orig, new, _ = design(44100)
    batch = np.zeros((3, max(lengths)), np.float32)
    for i, n in enumerate(lengths):
        batch[i, :n] = case(44100, n, 22)[0]
    xd, td = torch.from_numpy(batch).cuda(), torch.from_numpy(taps).cuda()
    n_in, n_out, guard, sentinel = batch.shape[1], rref.out_length(batch.shape[1], orig, new), 4096, -7.5
    outs = []
    for _ in range(2):
        buf = torch.full((guard + 3 * n_out + guard,), sentinel, dtype=torch.float32, device="cuda")
        y = buf[guard:guard + 3 * n_out]
        _lib.call("eav_resample_sinc_f32", xd.data_ptr(), td.data_ptr(), y.data_ptr(), 3, n_in, n_out, orig, new, width,
                  taps.shape[1], _lib.stream_ptr())
        torch.cuda.synchronize()
        assert bool((buf[:guard] == sentinel).all()) and bool((buf[guard + 3 * n_out:] == sentinel).all())
        outs.append(y.clone())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    _, ref, bound = case(44100, lengths[0], 22)
    check(outs[0][:len(ref)], ref, bound, "row 0 through the raw ABI")


def test_workgroups_that_walk_several_tiles_give_the_same_bits():
    """Above 2048 tiles in the launch a workgroup keeps its staged taps for several tiles: 1100 rows of 4 tiles (the
    last ragged) against the single-row launch, row i scaled by 2^-(i mod 3) - an exact scaling in fp32."""
    x, ref, bound = case(44100, 22000, 23)
    one = resample_waveforms(x, 44100, 16000)[0]
    check(one, ref, bound, "441/160, L 22000")
    rows = 1100
    scale = torch.tensor([1.0, 0.5, 0.25], device="cuda")[torch.arange(rows, device="cuda") % 3]
    many = resample_waveforms(torch.from_numpy(x).cuda()[None] * scale[:, None], 44100, 16000)
    assert torch.equal(many, one[None] * scale[:, None])


@pytest.mark.parametrize("rate", [44100, 8000])
def test_impulses_reproduce_the_taps(rate):
    """A unit impulse at 0, at orig - 1 and at L - 1 reads the float32 taps back: exact up to the skipped clamped taps."""
    taps, width, orig, new, _ = design(rate)
    length = 1000
    for pos in (0, orig - 1, length - 1):
        x = np.zeros(length, np.float32)
        x[pos] = 1.0
        ref, _ = rref.apply(x, taps, width, orig, new)
        got = resample_waveforms(x, rate, 16000)[0].double().cpu().numpy()
        assert got.shape == ref.shape
        assert float(np.abs(got - ref).max()) <= 1e-30, (rate, pos)
        assert np.count_nonzero(ref) > 0


def test_equal_rates_return_the_input_bitwise():
    x = synth.normal(24, (2, 777), 0.0, 0.3)
    y, out_lengths = resample_waveforms(x, 16000, 16000, lengths=[777, 100])
    assert torch.equal(y.cpu().view(torch.int32), torch.from_numpy(x).view(torch.int32))
    assert list(out_lengths) == [777, 100]


def test_dense_conv1d_form_agrees():
    """torchaudio's own application - F.conv1d of the padded waveform with every stored tap, stride orig - on this GPU."""
    taps, width, orig, new, _ = design(44100)
    x, ref, bound = case(44100, 2999, 21)
    xp = torch.nn.functional.pad(torch.from_numpy(x).cuda()[None, None], (width, width + orig))
    dense = torch.nn.functional.conv1d(xp, torch.from_numpy(taps).cuda()[:, None, :], stride=orig)
    dense = dense.transpose(1, 2).reshape(-1)[:len(ref)]
    print(f"conv1d against the float64 reference: max |err| {np.abs(dense.double().cpu().numpy() - ref).max():.3e}")
    got = resample_waveforms(x, 44100, 16000)[0]
    err = (got.double() - dense.double()).abs().cpu().numpy()
    print(f"kernel against conv1d: max |diff| {err.max():.3e}")
    assert np.all(err <= bound)


@pytest.fixture(scope="module")
def loaded(tmp_path_factory):
    from eav_amd.audio_data import DataLoadAudio
    root = str(tmp_path_factory.mktemp("eav"))
    folder = util.write_subject(root)
    d = DataLoadAudio(subject=util.SUBJECT, parent_directory=root, target_sampling_rate=util.TARGET)
    feature, label_indexes = d.process()
    return d, feature, label_indexes, os.listdir(folder)


def test_class_against_the_golden_of_the_reference_class(loaded, capsys):
    d, feature, label_indexes, names = loaded
    g = np.load(GOLDEN)
    want_x, want_idx, want_lab = util.expected_in_order(g, names)
    assert [os.path.basename(p) for p in d.file_path] == names
    assert d.file_emotion == [n.split("_")[4] for n in names]
    assert feature.dtype == np.float32 and feature.shape == want_x.shape
    assert label_indexes.dtype == np.int64 and np.array_equal(label_indexes, want_idx)
    assert list(d.label) == list(want_lab) and d.label.dtype.kind == "U"
    assert d.original_sampling_rate == util.RATE and d.seg_length == 5
    # kernel rounding (n_eff + 2) and the golden's own rounding to float32 (1), on sum |tap x| <= max_p sum|taps_p| max|x|
    taps, _, _, _, n_eff = design(44100)
    atol = (int(n_eff.max()) + 3) * EPS * float(np.abs(taps.astype(np.float64)).sum(1).max()) * 0.8
    err = float(np.abs(feature.astype(np.float64) - want_x).max())
    print(f"class against the golden: max |err| {err:.3e} (atol {atol:.3e})")
    assert err <= atol
    assert d.feature_dev.is_cuda and d.feature_dev.dtype == torch.float32
    assert np.array_equal(d.feature_dev.cpu().numpy(), feature)
    # label_emotion() on a fresh object: the same labels and the reference's printed line
    from eav_amd.audio_data import DataLoadAudio
    capsys.readouterr()
    lab = DataLoadAudio(util.SUBJECT, d.parent_directory, util.TARGET).label_emotion()
    assert list(lab) == list(want_lab)
    assert capsys.readouterr().out.splitlines() == [str(g["lines"][0])]


def test_clips_feed_the_ast_front_end(loaded):
    d = loaded[0]
    v = waveforms_to_input_values(d.feature_dev)
    assert v.shape == (d.feature_dev.shape[0], 1024, 128) and bool(torch.isfinite(v).all())
