"""tests/conv64_fft_ref.py against what it restates, without a GPU: the geometry against eav_conv64_fft_ws_floats /
eav_conv64_fft_nparts over a few thousand shapes, the float64 references against F.conv1d in float64, its autograd and the
direct module's references, the float32 restatement against the a-priori bounds on every listed case, and the teeth of the
criteria: three faults fail `RMS <= 2 x the restatement's`, also at sizes that rtol 1e-4 / atol 1e-5 lets through, and one
sample past T in the statistics trips the own-output bound."""
import numpy as np
import pytest
import scipy.fft as sf
import torch
import torch.nn.functional as F

from eav_amd import synth
from tests import conv64_fft_ref as R
from tests import eegnet_direct_ref as DR


@pytest.fixture(scope="module")
def L():
    from eav_amd import _lib
    _lib.load()
    return _lib


def test_scipy_fft_keeps_complex64_and_the_8x8_factorisation_is_the_transform():
    a = (synth.normal(1, (3, 64)) + 1j * synth.normal(2, (3, 64))).astype(np.complex64)
    assert sf.fft(a, axis=-1).dtype == np.complex64 and sf.ifft(a, axis=-1, norm="forward").dtype == np.complex64
    exact = sf.fft(a.astype(np.complex128), axis=-1)
    err = np.abs(sf.fft(a, axis=-1) - exact).max()
    assert 1e-8 < err < 1e-4
    assert np.allclose(sf.ifft(sf.fft(a), norm="forward"), 64 * a, rtol=1e-4, atol=1e-3)
    assert np.abs(R.fft64_8x8(a) - exact).max() < 1e-4
    # the twiddle table the kernel types by hand: cos / sin of 2 pi j / 64 at float32
    tw = R.twiddles64()
    j = np.outer(np.arange(8), np.arange(8))
    assert np.array_equal(tw.real, np.cos(2 * np.pi * j / 64).astype(np.float32))
    assert np.array_equal(tw.imag, (-np.sin(2 * np.pi * j / 64)).astype(np.float32))


def test_geometry_equals_the_exports_over_a_sweep(L):
    Bs = list(range(1, 40)) + [63, 64, 65, 127, 128, 129, 130, 255, 256, 257, 384, 385, 512, 513, 640, 1023, 1024, 1025, 2047,
                                2048, 2049, 2100, 4096, 4097]
    Ts = list(range(1, 150)) + [195, 196, 197, 245, 246, 392, 625, 2500]
    n = 0
    for B in Bs:
        for T in Ts:
            if B * T > 3_000_000:
                continue
            ws, parts = L.plain("eav_conv64_fft_ws_floats", B, T), L.plain("eav_conv64_fft_nparts", B, T)
            g = R.geometry(B, T)
            assert ws == R.ws_floats(B, T) == R.ws_offsets(B, T)["end"], (B, T)
            assert parts == R.nparts(B, T) == 4 * g["pack_wgs"], (B, T)
            assert R.ncolp_of_ws(ws) == g["ncolp"] and g["ncol"] <= g["ncolp"] < g["ncol"] + 128, (B, T)
            assert (4 * R.ws_offsets(B, T)["Zf"]) % 16 == 0
            # every column has a wave, a wave at most cols_per_wave columns
            assert g["waves"] * g["cols_per_wave"] >= g["ncolp"], (B, T)
            n += 1
    assert n >= 3000


@pytest.mark.parametrize("case", R.ALL, ids=str)
def test_each_case_reaches_what_it_is_listed_for(L, case):
    B, T = case
    g = R.geometry(B, T)
    assert R.ncolp_of_ws(L.plain("eav_conv64_fft_ws_floats", B, T)) == g["ncolp"]
    assert L.plain("eav_conv64_fft_nparts", B, T) == g["waves"]
    for k, v in R.COLUMNS.get(case, {}).items():
        assert g[k] == v, (k, g[k], v)
    if case in R.SMALL:
        assert g["ncolp"] == 128 and g["cols_per_wave"] == 1


def test_the_listed_shapes_sit_on_the_edges_they_name():
    g = {c: R.geometry(*c) for c in R.ALL}
    assert [g[c]["nblk"] for c in ((3, 49), (2, 50), (3, 98), (2, 99), (2, 147))] == [1, 2, 2, 3, 3]
    assert [g[c]["npair"] for c in ((3, 98), (2, 99))] == [1, 2]
    assert g[(257, 50)]["tiles"] % g[(257, 50)]["gemm_wgs"] != 0
    assert g[(2049, 8)]["ncol"] > g[(2049, 8)]["waves"]
    # "auto" takes the frequency-domain path from B * Samples // 4 >= 40000 on: far above every listed shape but the last
    assert all(B * T < 40000 for B, T in R.ALL)


@pytest.mark.parametrize("B,T", [(2, 1), (2, 7), (3, 16), (2, 48), (3, 49), (2, 50), (2, 99), (2, 147), (5, 33)])
def test_float64_references_against_conv1d_and_autograd(B, T):
    x, w, du = R.inputs(B, T, "normal")
    xt = torch.from_numpy(x).double().requires_grad_()
    wt = torch.from_numpy(w).double().requires_grad_()
    out = F.conv1d(F.pad(xt, (7, 8)), wt)
    out.backward(torch.from_numpy(du).double())
    for got, want in ((R.fwd_ref(x, w), out.detach()), (R.dgrad_ref(du, w), xt.grad), (R.wgrad_ref(du, x), wt.grad)):
        want = want.numpy()
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    # ... and the direct module's restatements of the same three maps
    xs, ws, dus = torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(du)
    assert np.abs(R.fwd_ref(x, w) - DR.conv64_fwd_ref(xs, ws)["out"].numpy()).max() <= 1e-12
    assert np.abs(R.dgrad_ref(du, w) - DR.conv64_dgrad_ref(dus, ws)["out"].numpy()).max() <= 1e-12
    assert np.abs(R.wgrad_ref(du, x) - DR.conv64_wgrad_ref(dus, xs)["dW"].numpy()).max() <= 1e-11
    st = R.stat_ref(out.detach().numpy())
    assert np.allclose(st[:64], out.detach().sum((0, 2)).numpy()) and np.allclose(st[64:], (out.detach() ** 2).sum((0, 2)).numpy())


@pytest.mark.parametrize("drop", [0.0, 0.5])
def test_fused_du_reference_against_autograd(drop):
    """du of the fused form = autograd of Dropout(AvgPool8(ELU(scale u + shift))) at m1 = m2 = 0, plus the two BatchNorm terms"""
    B, T = 2, 50
    dp, u, bn, mask = R.fused_inputs(B, T)
    r = R.du_ref(dp, u, bn, mask, drop)
    ut = u.double().requires_grad_()
    sc, sh = bn[2].double()[None, :, None], bn[3].double()[None, :, None]
    p = F.avg_pool1d(F.elu(sc * ut + sh), 8) * DR.pool_mult(mask, drop, (B, 64, T // 8))
    (p * dp.double()).sum().backward()
    mean, invstd, m1, m2 = (bn[i].double()[None, :, None] for i in (0, 1, 4, 5))
    want = ut.grad - sc * (m1 + (u.double() - mean) * invstd * m2)
    assert float((r["du"] - want).abs().max()) <= 1e-12
    assert bool((r["du"][:, :, 48:] != 0).all()), "the tail past the last whole window carries the BatchNorm terms"


WORST = {}


def note(k, v):
    WORST[k] = max(WORST.get(k, 0.0), v)


def yard_ratios(B, T, mode, arg=None):
    ref, bound, yard = R.refs(B, T, mode, arg), R.bounds(B, T, mode, arg), R.yardsticks(B, T, mode, arg)
    r = {k: float((np.abs(y - a) / b.clip(1e-300)).max()) for k, y, a, b in zip(("out", "dx", "dW"), yard, ref, bound)}
    if mode == "impulse" and T >= 16:
        assert np.abs(ref[0]).max() >= 1.0 and np.abs(ref[1]).max() >= 1.0, "an impulse case that moves nothing"
    for k, v in r.items():
        note(k, v)
    return r


@pytest.mark.parametrize("case", R.ALL, ids=str)
def test_restatement_stays_within_the_bound(case):
    B, T = case
    modes = [("normal", None)] + ([("dc", None), ("impulse", None)] if case in R.SMALL else [])
    modes += [("range", k) for k in R.RANGE_KINDS] if case in R.RANGE_CASES else []
    modes += [("tone", m) for m in R.TONE_BINS] if case == R.TONE_CASE else []
    for mode, arg in modes:
        r = yard_ratios(B, T, mode, arg)
        assert max(r.values()) <= 0.1, (mode, arg, r)
    print(f"float32 restatement, worst error / bound so far: {WORST}")


def test_restatement_of_the_statistics_and_one_sample_past_T():
    """sums of the restatement's own output are exact by construction; a sum that takes in the sample at t = T - which the
    kernel computes (it is inside the block) and must leave out - is outside the own-output bound"""
    for B, T in ((2, 50), (2, 99), (3, 16)):
        assert T % R.LV
        x, w, _ = R.inputs(B, T, "normal")
        full = R.fwd_c32(x, w, 7, full=True).astype(np.float64)
        own = full[..., :T]
        bound = R.stat_bound(own, B, T)
        wrong = R.stat_ref(full[..., :T + 1])
        over = np.abs(wrong - R.stat_ref(own)) / bound
        print(f"{(B, T)}: one sample past T moves the sums by {over[:64].min():.1f} .. {over[:64].max():.1f} and the sums of "
              f"squares by {over[64:].min():.1f} .. {over[64:].max():.1f} bounds")
        # (a channel whose sample at T happens to be tiny stays inside: the GPU test holds all 128 entries to the bound)
        assert (over[64:] > 1.0).mean() > 0.9 and (over[:64] > 1.0).mean() > 0.9


# --------------------------------------------------------------------------------------------------- the criteria have teeth
# Three faults at the sizes the issue names (s = 1): one twiddle of the input transform off by a relative 2^-12, one bin's
# filter spectrum times 1 + 1e-4, block B picking up 1e-5 of block A.  Measured here, element-wise rtol 1e-4 / atol 1e-5
# against float64 - what stood in front of these kernels - does NOT let all of them through at full size on N(0,1) data:
# 0.3 % - 10 % of the elements (those with |ref| < 0.3) exceed it; their largest error is 0.08 - 0.25 of
# atol + rtol max |ref|.  So the test asserts the criterion at full size, and the gap where it exists: the fault shrunk by
# powers of two until the old tolerance passes it (1/4 .. 1/16) still fails RMS <= 2 x.
def faulty(fault, s=1.0):
    if fault == "twiddle":
        tw = R.twiddles64()
        tw[3, 5] *= np.complex64(1 + s * 2.0 ** -12)
        return dict(fft=lambda a: R.fft64_8x8(a, tw))
    if fault == "bin":
        def hook(G):
            G = G.copy()
            G[:, :, 9] *= np.float32(1 + s * 1e-4)
            return G
        return dict(G_hook=hook)
    return dict(leak=s * 1e-5)


FAULTS = ["twiddle", "bin", "leak"]
TEETH = [(2, 147, "normal", None), (3, 98, "normal", None), (2, 147, "tone", 9), (2, 147, "tone", 31)]


@pytest.mark.parametrize("fault", FAULTS)
@pytest.mark.parametrize("B,T,mode,arg", TEETH)
def test_faults_fail_the_rms_criterion_where_the_old_tolerance_passed(B, T, mode, arg, fault):
    x, w, du = R.inputs(B, T, mode, arg)
    ref, refw = R.fwd_ref(x, w), R.wgrad_ref(du, x)
    plain = dict(fft=lambda a: R.fft64_8x8(a)) if fault == "twiddle" else {}
    e0 = R.rms(R.fwd_c32(x, w, 7, **plain) - ref)
    e0w = R.rms(R.wgrad_c32(x, du, **plain) - refw)
    if mode == "tone" and fault == "bin" and arg != 9:
        return                                           # a tone at bin 31 never meets bin 9's filter spectrum
    s, gap = 1.0, None
    while s >= 1.0 / 64:
        bad = R.fwd_c32(x, w, 7, **faulty(fault, s))
        e1 = R.rms(bad - ref)
        old = R.passes_old_tolerance(bad, ref)
        print(f"{(B, T, mode, arg)} {fault} x {s}: RMS error {e1:.3e} against {e0:.3e}, ratio {e1 / e0:.1f}; rtol 1e-4 / atol 1e-5 "
              f"{'passes' if old else 'fails'} it")
        if s == 1.0:
            assert e1 > R.RMS_MARGIN * e0, "the RMS criterion does not notice the fault at the size the issue names"
        if old:
            gap = e1 / e0
            break
        s /= 2
    if mode == "normal":
        assert gap is not None and gap > R.RMS_MARGIN, "no fault size that the old tolerance passes and the RMS criterion fails"
    if fault != "bin":                                   # the same transform / columns feed the weight gradient
        badw = R.wgrad_c32(x, du, **faulty(fault, 1.0))
        e1w = R.rms(badw - refw)
        old = R.passes_old_tolerance(badw, refw, atol=1e-4 * np.abs(refw).max())
        print(f"{(B, T, mode, arg)} {fault}: dW RMS error {e1w:.3e} against {e0w:.3e}, ratio {e1w / e0w:.1f}; rtol 1e-4 / atol 1e-4 "
              f"max |dW| {'passes' if old else 'fails'} it")
        assert e1w > R.RMS_MARGIN * e0w
        if mode == "normal":
            assert old
