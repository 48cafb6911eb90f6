"""The references of tests/preprocess_ref.py, pinned without a GPU: the frame reference bit-equal to Pillow and to the
oracle, the log-mel reference equal to the oracle at the defaults, the IIR truth and emulation against scipy."""
import numpy as np
import pytest

from tests import kernel_check as kc
from tests import preprocess_ref as pr
from eav_amd import synth
from eav_amd.preprocess import kaldi_mel_filters, pillow_bilinear_tables
from oracle import preprocess_oracle as po


def frames_of(seed, n, H, W, C):
    return (synth.splitmix64(seed, n * H * W * C) % np.uint64(256)).astype(np.uint8).reshape(n, H, W, C)


SIZES = pr.FRAME_SIZES + [pr.LDS_LAST_LEGAL]


@pytest.mark.parametrize("src,dst", SIZES)
def test_coefficient_tables_equal_the_package_and_the_oracle(src, dst):
    for a, b in zip(src, dst):
        rb, rk = pr.bilinear_coeffs(a, b)
        for ob, ok in (pillow_bilinear_tables(a, b), po.precompute_coeffs(a, b)):
            assert np.array_equal(rb, ob) and np.array_equal(rk, ok), (a, b)


@pytest.mark.parametrize("src,dst", SIZES)
def test_frame_reference_is_bit_equal_to_pillow(src, dst):
    """C = 1 as mode L, C = 3 as RGB, C = 2 through the L path channel by channel; noise, all 0 and all 255."""
    from PIL import Image
    (H, W), (OH, OW) = src, dst
    for C in (1, 2, 3):
        noise = frames_of(kc.seed_of("pil", src, dst, C), 1, H, W, C)[0]
        for img in (noise, np.zeros_like(noise), np.full_like(noise, 255)):
            got = pr.resize_u8(np.ascontiguousarray(img.transpose(2, 0, 1)), OH, OW)          # [C, OH, OW]
            if C == 3:
                want = np.asarray(Image.fromarray(img, "RGB").resize((OW, OH), Image.BILINEAR)).transpose(2, 0, 1)
            else:
                want = np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(img[:, :, c]), "L")
                                            .resize((OW, OH), Image.BILINEAR)) for c in range(C)])
            assert got.dtype == np.uint8 and np.array_equal(got, want), (src, dst, C)


def test_frame_reference_is_bit_equal_to_the_oracle_at_its_defaults():
    frames = frames_of(92, 3, 56, 56, 3)
    got = pr.frames_ref(frames, (224, 224), *pr.NORMS["half"])
    want = po.vit_preprocess(frames)
    assert got.dtype == want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    odd = frames_of(93, 2, 40, 64, 3)
    mean, std = pr.NORMS["imagenet"]
    want = np.stack([((po.resize_bilinear_u8(f, 96, 48).transpose(2, 0, 1).astype(np.float64) / 255).astype(np.float32)
                      - np.float32(mean)[:, None, None]) / np.float32(std)[:, None, None] for f in odd])
    assert np.array_equal(pr.frames_ref(odd, (96, 48), mean, std, 1 / 255).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("L,max_len", [(400, 1), (3000, 17), (3000, 24), (3000, 2), (560, 2)])
def test_logmel_reference_equals_the_oracle_at_the_defaults(L, max_len):
    wav = synth.normal(kc.seed_of("fbank", L), (2, L), 0.0, 0.2)
    got, bound = pr.fbank_ref(wav, max_len, kaldi_mel_filters(257, 128))
    want = po.ast_fbank(wav, max_length=max_len)
    assert got.dtype == want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    nfr = 1 + (L - 400) // 160
    assert bound.shape == got.shape and (bound[:, :nfr] > 0).all() and (bound[:, nfr:] == 0).all()
    # what the bound is made of: at least two float32 ulps of the output, at most a few
    assert (bound[:, :nfr] >= 2 * pr.ulp32(got[:, :nfr])).all() and bound.max() < 4e-6


def test_one_hot_filters_read_single_bins():
    """All-ones window, no pre-emphasis: the output is the log power of single bins of the DC-removed frame."""
    x = np.zeros((1, 400), np.float32)
    x[0, 399] = 1.0
    got, _ = pr.fbank_ref(x, 1, pr.one_hot_filters(0, 256), window=np.ones(400), preemph=0.0, mean=0.0, std2=1.0)
    spec = np.fft.rfft(np.concatenate([x[0].astype(np.float64) - 1 / 400, np.zeros(112)]))
    want = np.log(np.maximum(pr.MEL_FLOOR, np.abs(spec[:256]) ** 2))
    assert np.abs(got[0, 0] - want).max() < 1e-6
    last, _ = pr.fbank_ref(x, 1, pr.one_hot_filters(256, 1), window=np.ones(400), preemph=0.0, mean=0.0, std2=1.0)
    assert abs(last[0, 0, 0] - np.log(max(pr.MEL_FLOOR, abs(spec[256]) ** 2))) < 1e-6


def sos_input():
    return synth.normal(kc.seed_of("sos"), (3, pr.SOS_N)).astype(np.float64) + 2.0


@pytest.mark.parametrize("name", list(pr.SOS_FILTERS))
def test_iir_references_agree(name):
    """scipy's float64 sosfilt and the emulation of the kernel's three passes lie within 1e-11 max(1, max|ref|) of the
    long-double cascade on the GPU test's cases (loose: this guards the references, not the kernel); one chunk is the plain
    float64 recurrence bit for bit."""
    from scipy.signal import sosfilt
    sos, x = pr.sos_of(name), sos_input()
    assert len(sos) == {"5-30": 5, "0.3-45": 5, "order1": 1, "order8": 8}[name]
    truth = pr.sos_truth(sos, x)
    assert truth.dtype == np.longdouble and np.finfo(np.longdouble).eps <= 2.0 ** -60
    tol = 1e-11 * max(1.0, float(np.abs(truth).max()))
    assert float(np.abs(sosfilt(np.array(sos), x, axis=1) - truth).max()) <= tol
    plain = pr.sos_cascade(sos, x, np.float64)
    for n, chunk in pr.SOS_CASES:
        emul = pr.sos_emulate(sos, x[:, :n], chunk)
        err = float(np.abs(emul - truth[:, :n]).max())
        assert emul.shape == (3, n) and err <= tol, (name, n, chunk, err)
        if chunk >= n:
            assert np.array_equal(emul.view(np.uint64), plain[:, :n].view(np.uint64))
    assert np.array_equal(pr.sos_emulate(sos, x[:, :100], 100).view(np.uint64), plain[:, :100].view(np.uint64))


def test_decimation_reuses_the_resampler_reference():
    from scipy.signal import resample_poly
    from eav_amd.eeg_data import resample_poly_design
    x = synth.normal(7, (2, 1281)).astype(np.float64) + 0.25
    for down in pr.DECIMATE_DOWN:
        h, center = resample_poly_design(1, down)
        assert len(h) == 20 * down + 1 and (down != 2 or len(h) == 41)
        ref, bound = pr.decimate_ref(x, h, down, center)
        want = resample_poly(x, 1, down, axis=1)
        assert ref.shape == want.shape == (2, -(-1281 // down))
        assert np.abs(ref.astype(np.float64) - want).max() < 1e-13 and (bound > 0).all()
