"""DataLoadAudio and the sinc resampler, host side (no GPU): the filter design against the float64 restatement of
torchaudio's arithmetic (tests/audio_resample_ref.py), that restatement against an analytic sine, the class's interface
against the reference's (tests/golden/audio_load.npz), the ABI's argument validation, and the golden reproduced by the
float64 path plus the host logic alone."""
import inspect
import os

import numpy as np
import pytest

from tests import audio_data_util as util
from tests import audio_resample_ref as rref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "audio_load.npz")

RATES = [(44100, (441, 160, 17, 475)), (48000, (3, 1, 19, 41)), (22050, (441, 320, 9, 459)), (8000, (1, 2, 7, 15)),
         (11025, (441, 640, 7, 455))]


@pytest.mark.parametrize("rate,shape", RATES)
def test_design_equals_the_reference_taps_bit_for_bit(rate, shape):
    from eav_amd.preprocess import sinc_resample_design
    taps, width, orig, new = sinc_resample_design(rate, 16000)
    ref, rwidth, rorig, rnew = rref.design_f32(rate, 16000)
    assert (orig, new, width, taps.shape[1]) == shape == (rorig, rnew, rwidth, ref.shape[1])
    assert taps.dtype == np.float32 and taps.shape == (new, 2 * width + orig)
    assert np.array_equal(taps.view(np.uint32), ref.view(np.uint32))
    # what the banded kernel relies on: outside [floor(p*orig/new), +2*width] every stored tap is a clamped one
    outside = np.ones(taps.shape, dtype=bool)
    for p in range(new):
        outside[p, p * orig // new:p * orig // new + 2 * width + 1] = False
    assert float(np.abs(ref[outside]).max(initial=0.0)) <= 1e-30


@pytest.mark.parametrize("rate", [44100, 48000])
def test_reference_resampler_reproduces_a_sine(rate):
    """Pins delay and gain of the float64 restatement: a 1 kHz sine stays a 1 kHz sine at 16 kHz."""
    n = rate // 2
    x = np.sin(2 * np.pi * 1000.0 * np.arange(n) / rate)
    y = rref.resample(x, rate, 16000)
    assert len(y) == -(-16000 * n // rate)
    want = np.sin(2 * np.pi * 1000.0 * np.arange(len(y)) / 16000.0)
    err = float(np.abs(y - want)[200:-200].max())
    print(f"{rate} -> 16000: max error {err:.2e}")
    assert err <= 1e-3


def test_class_interface_equals_the_reference():
    from eav_amd.audio_data import DataLoadAudio
    g = np.load(GOLDEN)
    params = inspect.signature(DataLoadAudio.__init__).parameters
    assert list(params) == [str(p) for p in g["init_params"]]
    assert params["subject"].default == str(g["default_subject"])
    assert params["target_sampling_rate"].default == int(g["default_target_sampling_rate"])
    methods = sorted(k for k, v in vars(DataLoadAudio).items() if inspect.isfunction(v) and not k.startswith("_"))
    assert methods == [str(m) for m in g["methods"]]
    d = DataLoadAudio(subject=util.SUBJECT, parent_directory="nowhere", target_sampling_rate=util.TARGET)
    assert d.seg_length == int(g["seg_length"])
    assert set(str(a) for a in g["attributes"]) <= set(vars(d))
    assert d.feature is None and d.label is None and d.label_indexes is None and d.file_path == []


def test_abi_rejects_a_tap_count_that_does_not_match():
    from eav_amd import _lib
    with pytest.raises(_lib.EavError, match="ntaps"):
        _lib.call("eav_resample_sinc_f32", 1, 1, 1, 1, 441, 160, 441, 160, 17, 474, None)
    with pytest.raises(_lib.EavError, match="null"):
        _lib.call("eav_resample_sinc_f32", None, 1, 1, 1, 441, 160, 441, 160, 17, 475, None)
    with pytest.raises(_lib.EavError, match="positive"):
        _lib.call("eav_resample_sinc_f32", 1, 1, 1, 0, 441, 160, 441, 160, 17, 475, None)
    with pytest.raises(_lib.EavError, match="n_out"):
        _lib.call("eav_resample_sinc_f32", 1, 1, 1, 1, 442, 160, 441, 160, 17, 475, None)


def test_process_raises_without_a_gpu(tmp_path):
    import torch
    from eav_amd import _lib
    from eav_amd.audio_data import DataLoadAudio
    from eav_amd.preprocess import resample_waveforms
    with pytest.raises(_lib.EavError, match="MI355X"):
        resample_waveforms(np.zeros((1, 8), np.float32), 44100, 16000, device="cpu")
    util.write_subject(str(tmp_path))
    d = DataLoadAudio(subject=util.SUBJECT, parent_directory=str(tmp_path), target_sampling_rate=util.TARGET)
    d.device = torch.device("cpu")
    with pytest.raises(_lib.EavError, match="MI355X"):
        d.process()


def test_multi_channel_files_are_refused(tmp_path):
    from scipy.io import wavfile
    from eav_amd.audio_data import read_wav_mono
    path = str(tmp_path / "stereo.wav")
    wavfile.write(path, util.RATE, np.zeros((100, 2), np.int16))
    with pytest.raises(ValueError, match="stereo.wav"):
        read_wav_mono(path)


@pytest.mark.parametrize("kind,scale", [("int16", 32768.0), ("int32", 2.0 ** 31), ("uint8", None), ("float32", 1.0)])
def test_wav_reader_normalises_like_torchaudio_load(tmp_path, kind, scale):
    from scipy.io import wavfile
    from eav_amd.audio_data import read_wav_mono
    raw = {"int16": np.array([-32768, -1, 0, 1, 32767], np.int16),
           "int32": np.array([-2 ** 31, -65536, 0, 65536, 2 ** 31 - 1], np.int32),
           "uint8": np.array([0, 127, 128, 129, 255], np.uint8),
           "float32": np.array([-1.0, -0.25, 0.0, 0.3, 1.0], np.float32)}[kind]
    path = str(tmp_path / f"{kind}.wav")
    wavfile.write(path, 8000, raw)
    wav, rate = read_wav_mono(path)
    want = (raw.astype(np.float64) - 128.0) / 128.0 if kind == "uint8" else raw.astype(np.float64) / scale
    assert rate == 8000 and wav.dtype == np.float32
    assert np.array_equal(wav, want.astype(np.float32))
    assert np.array_equal(wav, util.read_wav(path)[0])


def test_golden_is_reproduced_by_the_float64_path_and_host_logic(tmp_path):
    """Listing, field 4 of the name, the mapping, floor division into clips and the dtypes, with the float64 resampler
    in place of the kernel: equal to what the reference class produced, bit for bit."""
    g = np.load(GOLDEN)
    folder = util.write_subject(str(tmp_path))
    names = os.listdir(folder)
    mapping = {"Neutral": 0, "Sadness": 1, "Anger": 2, "Happiness": 3, "Calmness": 4}
    seg = util.TARGET * int(g["seg_length"])
    feats, idx = [], []
    for name in names:
        wav, rate = util.read_wav(os.path.join(folder, name))
        y = rref.resample(wav, rate, util.TARGET).astype(np.float32)
        for i in range(len(y) // seg):
            feats.append(y[i * seg:(i + 1) * seg])
            idx.append(mapping[name.split("_")[4]])
    want_x, want_idx, want_lab = util.expected_in_order(g, names)
    assert np.array_equal(np.array(feats), want_x) and np.array_equal(np.array(idx), want_idx)
    assert [str(s) for s in g["dtypes"]] == ["float32", "int64", "U"]
    assert int(g["original_sampling_rate"]) == util.RATE
    assert str(g["lines"][0]) == f"Original sf: {util.RATE}, resampled into {util.TARGET}"
    # the golden's own listing order gives its stored arrays back
    own = util.expected_in_order(g, [str(n) for n in g["names"]])
    assert np.array_equal(own[0], g["features"]) and np.array_equal(own[1], g["label_indexes"])
    assert list(own[2]) == [str(s) for s in g["label"]]
