"""The pre-processing kernels of eav_amd/csrc/preprocess.hip at their edges, through the raw entry points, against the
plain references of tests/preprocess_ref.py (pinned on the CPU by tests/test_preprocess_ref_cpu.py).  Every output lands
in a NaN-sentinel buffer with a guard band (tests/kernel_check.py); a float64 output is 2 n float32 words viewed as float64.

eav_resize_normalize_u8   bit-equal to the reference (Pillow's fixed-point resampler, float32 normalisation).
eav_ast_fbank             exact statements bit-compared (padding, a constant clip, two launches); otherwise within

        tol = 2 ((2^-22 + ulp32(log v)) / std2 + ulp32(out))

    of the float64 recipe.  Derivation: kernel and reference round the 512-point spectrum to complex64 like the numpy
    path of the feature extractor; two float64 FFTs differ by ~1e-16 of the frame's largest bin, which can only flip the
    float32 rounding of a component - one float32 ulp of that component, a relative 2^-23 at most - so a bin's power
    r^2 + i^2, and with it the non-negative mel sum v, moves by a relative 2^-22 at most and log v by 2^-22.  The float32
    rounding of log v may then land one ulp32(log v) away, (x - mean) / std2 divides that by std2, and its own two float32
    roundings may move the output by one ulp32(out).  Doubled once for the reference's own roundings.  Nothing is fitted
    to what the kernel gives; padded frames have the bound 0.
    Measured on the MI355X: every output of the grid and of the FFT isolation case is bit-equal to the reference
    (error / bound 0) - a flip needs a component within ~1e-16 of a float32 rounding boundary.
eav_decimate_fir_f64      within tests/eeg_resample_ref.bound of the long-double sum, the bound eav_resample_poly_f64 is
    held to ((n_i + 2) 2^-53 sum |h x|).  Measured: worst error / bound 0.223.
eav_sosfilt_f64           the truth is the long-double cascade.  With e_emul the error of a float64 emulation of the
    same three passes and e_scipy that of scipy's float64 sosfilt, the kernel is allowed

        4 max(e_emul, e_scipy) + 2^-52 max|ref|

    (4: the device contracts multiply-adds into fma, the emulation does not - a margin over the reference's error, not
    over the kernel's).  Measured: worst e_gpu / max(e_emul, e_scipy) 1.332 (eight sections, chunk 257) over the 24
    (filter, n, chunk) cases x 3 channel counts; e_gpu / tolerance 0.323 at most."""
import functools

import numpy as np
import pytest
import torch

from tests import kernel_check as kc
from tests import preprocess_ref as pr
from eav_amd import _lib, synth
from eav_amd import eeg_data as ed
from eav_amd.preprocess import kaldi_mel_filters, pillow_bilinear_tables

pytestmark = pytest.mark.gpu


def f64_out(n):
    """Sentinel buffer of n float64 outputs (2 n float32 words) plus the guard band."""
    return kc.sentinel_buf(2 * n)


def take64(buf, shape, what):
    n = int(np.prod(shape))
    return kc.take(buf, 2 * n, (2 * n,), what).view(torch.float64).view(*shape).numpy()


def untouched(buf):
    torch.cuda.synchronize()
    return bool((buf.cpu().view(torch.int32) == kc.SENT).all())


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def check(got, ref, bound, what):
    """|got - ref| <= bound element by element; prints the worst error / bound.  -> that ratio"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert not np.isnan(got).any(), f"{what}: NaN"
    err = np.abs(got.astype(ref.dtype) - ref).astype(np.float64)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max())
    print(f"{what}: max |err| {err.max():.3e}, worst err / bound {worst:.3f}")
    assert worst <= 1.0, (what, worst, tuple(int(i) for i in np.unravel_index(ratio.argmax(), ratio.shape)))
    return worst


# ------------------------------------------------------------------------------------------------ frames
def frames_of(seed, n, H, W, C):
    f = (synth.splitmix64(seed, n * H * W * C) % np.uint64(256)).astype(np.uint8).reshape(n, H, W, C)
    if n >= 5:
        f[3], f[4] = 0, 255
    return f


def resize_launch(frames, size, mean, std, out=None):
    n, H, W, C = frames.shape
    OH, OW = size
    bx, kx = pillow_bilinear_tables(W, OW)
    by, ky = pillow_bilinear_tables(H, OH)
    fd, kxd, bxd, kyd, byd = (kc.dev(a) for a in (frames, kx, bx, ky, by))
    m = np.asarray(list(mean) + [0.0, 0.0], np.float32)[:3].copy()
    s = np.asarray(list(std) + [1.0, 1.0], np.float32)[:3].copy()
    buf = kc.sentinel_buf(n * C * OH * OW) if out is None else out
    _lib.call("eav_resize_normalize_u8", fd.data_ptr(), kxd.data_ptr(), bxd.data_ptr(), kyd.data_ptr(), byd.data_ptr(),
              buf.data_ptr(), n, H, W, C, OH, OW, kx.shape[1], ky.shape[1], 1.0 / 255.0, m.ctypes.data, s.ctypes.data,
              _lib.stream_ptr())
    return kc.take(buf, n * C * OH * OW, (n, C, OH, OW), f"resize {(H, W)} -> {size}, C {C}, n {n}")


@pytest.mark.parametrize("src,dst", pr.FRAME_SIZES)
def test_resize_normalize_is_bit_equal_to_the_reference(src, dst):
    """C in 1..3, one frame and five (the last two all 0 and all 255), both normalisations.  The horizontal pass of a
    frame lives in LDS: the one combination of the list that needs more than 64 KiB is refused, like any other."""
    for C in (1, 2, 3):
        for n in (1, 5):
            frames = frames_of(kc.seed_of("frames", src, dst, C, n), n, *src, C)
            for name, (mean, std) in pr.NORMS.items():
                if C * src[0] * dst[1] > 64 * 1024:       # (100, 3) -> (9, 300) at C = 3: 90 000 bytes, beyond the contract
                    buf = kc.sentinel_buf(n * C * dst[0] * dst[1])
                    with pytest.raises(_lib.EavError, match="64 KiB LDS tile"):
                        resize_launch(frames, dst, mean[:C], std[:C], out=buf)
                    assert (src, dst, C) == ((100, 3), (9, 300), 3) and untouched(buf)
                    continue
                got = resize_launch(frames, dst, mean[:C], std[:C])
                ref = pr.frames_ref(frames, dst, mean, std)
                kc.same(got, torch.from_numpy(ref), f"resize {src} -> {dst}, C {C}, n {n}, {name}")


def test_resize_normalize_at_the_last_legal_lds_size_and_one_byte_past_it():
    """C * H * OW = 65 536 bytes is the whole 64 KiB tile: valid and bit-equal.  One row more is refused before any
    launch - an error return that leaves the output alone."""
    (H, W), (OH, OW) = pr.LDS_LAST_LEGAL
    assert H * OW == 64 * 1024
    mean, std = pr.NORMS["imagenet"]
    frames = frames_of(kc.seed_of("lds"), 2, H, W, 1)
    kc.same(resize_launch(frames, (OH, OW), mean[:1], std[:1]), torch.from_numpy(pr.frames_ref(frames, (OH, OW), mean, std)),
            "resize at 64 KiB of LDS")
    buf = kc.sentinel_buf(OH * OW)
    with pytest.raises(_lib.EavError, match="64 KiB LDS tile"):
        resize_launch(frames_of(kc.seed_of("lds+1"), 1, H + 1, W, 1), (OH, OW), mean[:1], std[:1], out=buf)
    assert untouched(buf)


# ------------------------------------------------------------------------------------------------ log-mel
@functools.lru_cache(maxsize=None)
def fbank_tables():
    k = np.arange(256)
    tw = np.stack([np.cos(2 * np.pi * k / 512), -np.sin(2 * np.pi * k / 512)], 1)
    return kc.dev(np.ascontiguousarray(tw, dtype=np.float64))


def fbank_launch(wav, max_len, filt, window=None, preemph=0.97, floor=pr.MEL_FLOOR, mean=pr.AST_MEAN, std2=pr.AST_STD * 2):
    n, L = wav.shape
    nmel = filt.shape[1]
    window = np.hanning(400) if window is None else window
    wd, wind, meld = kc.dev(np.asarray(wav, np.float32)), kc.dev(np.asarray(window, np.float64)), kc.dev(np.ascontiguousarray(filt.T, dtype=np.float64))
    buf = kc.sentinel_buf(n * max_len * nmel)
    _lib.call("eav_ast_fbank", wd.data_ptr(), wind.data_ptr(), fbank_tables().data_ptr(), meld.data_ptr(), buf.data_ptr(), n, L,
              max_len, nmel, float(preemph), float(floor), float(np.float32(mean)), float(np.float32(std2)), _lib.stream_ptr())
    return kc.take(buf, n * max_len * nmel, (n, max_len, nmel), f"fbank L {L}, max_len {max_len}, nmel {nmel}, n {n}").numpy()


def pad_value(mean=pr.AST_MEAN, std2=pr.AST_STD * 2):
    return (np.float32(0.0) - np.float32(mean)) / np.float32(std2)


@pytest.mark.parametrize("nmel", pr.FBANK_NMEL)
@pytest.mark.parametrize("L", pr.FBANK_L)
def test_fbank_within_the_derived_bound(L, nmel):
    filt = kaldi_mel_filters(257, nmel)
    nfr = 1 + (L - 400) // 160
    worst, equal, total = 0.0, 0, 0
    for n in (1, 3):
        wav = synth.normal(kc.seed_of("fbank", L, nmel, n), (n, L), 0.0, 0.2)
        for max_len in pr.FBANK_MAX_LEN:
            got = fbank_launch(wav, max_len, filt)
            ref, bound = pr.fbank_ref(wav, max_len, filt)
            worst = max(worst, check(got, ref, bound, f"fbank L {L}, nmel {nmel}, n {n}, max_len {max_len}"))
            live = min(nfr, max_len)
            equal += int((bits(got[:, :live]) == bits(ref[:, :live])).sum())
            total += n * live * nmel
            assert (bits(got[:, live:]) == bits(pad_value())).all(), "a padded frame is not float32((0 - mean) / std2)"
    print(f"fbank L {L}, nmel {nmel}: worst err / bound {worst:.3f}, {100.0 * equal / total:.1f} % of {total} outputs bit-equal")


def test_fbank_exact_statements():
    """Padding, a constant clip (DC removal leaves exactly 0: every mel energy is the floor) and a second launch."""
    filt = kaldi_mel_filters(257, 128)
    const = np.full((2, 3000), 0.3, np.float32)
    const[1] = -1.75
    got = fbank_launch(const, 24, filt)
    floor_value = (np.float32(np.log(pr.MEL_FLOOR)) - np.float32(pr.AST_MEAN)) / np.float32(pr.AST_STD * 2)
    assert floor_value.dtype == np.float32
    assert (bits(got[:, :17]) == bits(floor_value)).all() and (bits(got[:, 17:]) == bits(pad_value())).all()
    other = fbank_launch(const[:1, :400], 2, filt, mean=1.5, std2=0.75)                     # other constants than the defaults
    assert (bits(other[:, 0]) == bits((np.float32(np.log(pr.MEL_FLOOR)) - np.float32(1.5)) / np.float32(0.75))).all()
    assert (bits(other[:, 1]) == bits(pad_value(1.5, 0.75))).all()
    wav = synth.normal(kc.seed_of("fbank twice"), (3, 3000), 0.0, 0.2)
    assert np.array_equal(bits(fbank_launch(wav, 24, filt)), bits(fbank_launch(wav, 24, filt)))


def test_fbank_fft_alone():
    """All-ones window, no pre-emphasis, one-hot mel rows: the output is the log power of single bins (0..255, and 256
    in a second call) of the DC-removed frame - what localises a wrong butterfly or twiddle.  A unit impulse at sample 0
    (every twiddle multiplies 0 but the first input), at sample 399 (the last input: every bin a different phase) and a
    cosine at bin 37 (one peak and its leakage)."""
    x = np.zeros((3, 400), np.float32)
    x[0, 0] = 1.0
    x[1, 399] = 1.0
    x[2] = np.cos(2 * np.pi * 37 * np.arange(400) / 512)
    kw = dict(window=np.ones(400), preemph=0.0, mean=0.0, std2=1.0)
    worst = 0.0
    for first, count in ((0, 256), (256, 1)):
        filt = pr.one_hot_filters(first, count)
        got = fbank_launch(x, 1, filt, **kw)
        ref, bound = pr.fbank_ref(x, 1, filt, **kw)
        worst = max(worst, check(got, ref, bound, f"fbank bins {first}..{first + count - 1}"))
    print(f"fbank FFT alone: worst err / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------ decimating FIR
@functools.lru_cache(maxsize=None)
def decimate_case(down, n_in):
    h, center = ed.resample_poly_design(1, down)
    x = synth.normal(kc.seed_of("decimate", down, n_in), (3, n_in)).astype(np.float64) + 0.25
    ref, bound = pr.decimate_ref(x, h, down, center)
    for a in (x, h, ref, bound):
        a.setflags(write=False)
    return x, h, center, ref, bound


def decimate_launch(x, h, down, center):
    nch, n_in = x.shape
    n_out = -(-n_in // down)
    xd, hd = kc.dev(x), kc.dev(h)
    buf = f64_out(nch * n_out)
    _lib.call("eav_decimate_fir_f64", xd.data_ptr(), hd.data_ptr(), buf.data_ptr(), nch, n_in, n_out, down, len(h), center,
              _lib.stream_ptr())
    return take64(buf, (nch, n_out), f"decimate by {down}, n {n_in}, nch {nch}")


@pytest.mark.parametrize("down", pr.DECIMATE_DOWN)
@pytest.mark.parametrize("which", range(7))
def test_decimate_within_the_rounding_bound(which, down):
    n_in = pr.decimate_lengths(down)[which]
    x, h, center, ref, bound = decimate_case(down, n_in)
    assert len(h) == 20 * down + 1
    for nch in (1, 3):
        got = decimate_launch(x[:nch], h, down, center)
        check(got, ref[:nch], bound[:nch], f"decimate by {down}, n {n_in}, nch {nch}")
    assert np.array_equal(bits(got), bits(decimate_launch(x, h, down, center))), "two runs differ"


# ------------------------------------------------------------------------------------------------ IIR
@functools.lru_cache(maxsize=None)
def sos_input():
    x = synth.normal(kc.seed_of("sos"), (pr.SOS_NCH, pr.SOS_N)).astype(np.float64) + 2.0
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def sos_truth(name):
    """(long-double cascade, scipy's float64 sosfilt) of all 65 channels and 4099 samples: the filter is causal and the
    channels are independent, so every case reads a corner of these."""
    from scipy.signal import sosfilt
    truth = pr.sos_truth(pr.sos_of(name), sos_input())
    sp = sosfilt(np.array(pr.sos_of(name)), sos_input(), axis=1)
    truth.setflags(write=False)
    sp.setflags(write=False)
    return truth, sp


@functools.lru_cache(maxsize=None)
def sos_tables(name, chunk):
    return ed.sos_tables(pr.sos_of(name), chunk)


def sos_launch(sos, tables, x, chunk, bufs=None):
    nch, n = x.shape
    nsec = len(sos)
    nchunk = -(-n // chunk)
    xd, sd, Hd, ALd = kc.dev(x), kc.dev(np.array(sos)), kc.dev(tables[0]), kc.dev(tables[1])
    y, zend, zstart = bufs or (f64_out(nch * n), f64_out(nch * nchunk * 2 * nsec), f64_out(nch * nchunk * 2 * nsec))
    _lib.call("eav_sosfilt_f64", xd.data_ptr(), y.data_ptr(), sd.data_ptr(), Hd.data_ptr(), ALd.data_ptr(), zend.data_ptr(),
              zstart.data_ptr(), nch, n, nsec, chunk, _lib.stream_ptr())
    what = f"sosfilt n {n}, chunk {chunk}, nch {nch}, {nsec} sections"
    for buf, name in ((zend, "zend"), (zstart, "zstart")):
        assert np.isfinite(take64(buf, (nch, nchunk, 2 * nsec), f"{what}: {name}")).all()
    return take64(y, (nch, n), what)


@pytest.mark.parametrize("n,chunk", pr.SOS_CASES)
@pytest.mark.parametrize("name", list(pr.SOS_FILTERS))
def test_sosfilt_within_four_times_the_float64_references_error(name, n, chunk):
    sos, tables = pr.sos_of(name), sos_tables(name, chunk)
    truth, sp = sos_truth(name)
    x = sos_input()[:, :n]
    emul = pr.sos_emulate(sos, x, chunk, tables)
    for nch in (1, 3, pr.SOS_NCH):
        ref = truth[:nch, :n]
        e_emul = float(np.abs(emul[:nch] - ref).max())
        e_scipy = float(np.abs(sp[:nch, :n] - ref).max())
        e_ref = max(e_emul, e_scipy)
        tol = 4.0 * e_ref + 2.0 ** -52 * float(np.abs(ref).max())
        got = sos_launch(sos, tables, x[:nch], chunk)
        e_gpu = float(np.abs(got - ref).max())
        print(f"sosfilt {name}, n {n}, chunk {chunk}, nch {nch}: e_gpu {e_gpu:.3e}, e_emul {e_emul:.3e}, e_scipy {e_scipy:.3e}, "
              f"e_gpu / max(e_emul, e_scipy) {e_gpu / e_ref:.3f}, e_gpu / tol {e_gpu / tol:.3f}")
        assert e_gpu <= tol, (name, n, chunk, nch, e_gpu / e_ref)
    assert np.array_equal(bits(got), bits(sos_launch(sos, tables, x, chunk))), "two runs differ"
    if chunk == 257:                                                        # and the wrapper launches the same thing
        through = ed.sosfilt(np.array(sos), torch.from_numpy(np.array(x[:3])).cuda(), chunk=chunk).cpu().numpy()
        assert np.array_equal(bits(through), bits(got[:3]))


def test_sosfilt_refuses_nine_sections():
    from scipy.signal import butter
    sos = np.ascontiguousarray(butter(9, [5, 30], btype="bandpass", fs=100, output="sos"))
    assert len(sos) == 9
    x = np.array(sos_input()[:2, :300])
    bufs = (f64_out(2 * 300), f64_out(2 * 3 * 18), f64_out(2 * 3 * 18))
    with pytest.raises(_lib.EavError, match="at most 8 sections"):
        sos_launch(sos, ed.sos_tables(sos, 100), x, 100, bufs)
    assert all(untouched(b) for b in bufs)
