"""tests/fir_fft_ref.py against what it restates, without a GPU: the deal against eav_eegnet_fir_fft_plan (the launchers'
own functions) and the two sizing exports over a few thousand shapes and grid caps, the float64 references against F.conv2d
and autograd, the complex64 restatement against the a-priori bound, and every case's listed property from the plan export."""
import numpy as np
import pytest
import scipy.fft as sf
import torch
import torch.nn.functional as F

from eav_amd import synth
from tests import fir_fft_ref as R


@pytest.fixture(scope="module")
def L():
    from eav_amd import _lib
    _lib.load()
    yield _lib
    _lib.load().eav_eegnet_fir_fft_set_grid_cap(0)


def set_cap(L, cap):
    assert L.load().eav_eegnet_fir_fft_set_grid_cap(cap or 0) == 0


def test_scipy_fft_keeps_complex64():
    a = (synth.normal(1, (3, 1024)) + 1j * synth.normal(2, (3, 1024))).astype(np.complex64)
    assert sf.fft(a, axis=-1).dtype == np.complex64 and sf.ifft(a, axis=-1, norm="forward").dtype == np.complex64
    # ... and computes in it: float32 rounding shows against the complex128 transform
    err = np.abs(sf.fft(a, axis=-1) - sf.fft(a.astype(np.complex128), axis=-1)).max()
    assert 1e-7 < err < 1e-3
    # norm='forward' leaves the inverse unscaled
    assert np.allclose(sf.ifft(sf.fft(a), norm="forward"), 1024 * a, rtol=1e-4, atol=1e-2)


@pytest.mark.parametrize("B,C,S,K", [(2, 3, 40, 7), (1, 2, 33, 8), (2, 1, 9, 2), (3, 2, 5, 1), (1, 3, 800, 300), (2, 2, 20, 31)])
def test_float64_references_against_conv2d_and_autograd(B, C, S, K):
    x, wf = synth.normal(3, (B, C, S)), synth.normal(4, (8, K))
    g1 = synth.normal(5, (B, 8, C, S))
    xt = torch.from_numpy(x).double()[:, None]
    w = torch.from_numpy(wf).double()[:, None, None, :].requires_grad_()
    y = F.conv2d(xt, w, padding="same")
    ref = R.fwd_ref(x, wf)
    assert np.abs(ref - y.detach().numpy()).max() <= 1e-12 * np.abs(ref).max()
    # train form: firstBN in training mode behind the convolution, d loss / d (BN output) = g1
    gamma = torch.from_numpy(synth.uniform(6, (8,), 0.5, 1.5)).double()
    z = F.batch_norm(y, None, None, gamma, None, True, 0.0, 1e-5)
    (z * torch.from_numpy(g1).double()).sum().backward()
    yd = y.detach()
    mean, var = yd.mean((0, 2, 3)), yd.var((0, 2, 3), unbiased=False)
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    yhat = (yd - mean[None, :, None, None]) * invstd[None, :, None, None]
    g = torch.from_numpy(g1).double()
    bn = np.concatenate([mean.numpy(), invstd.numpy(), (gamma * invstd).numpy(), np.zeros(8), g.mean((0, 2, 3)).numpy(),
                         (g * yhat).mean((0, 2, 3)).numpy()])
    got = R.wgrad_ref(x, R.dy_ref(g1.astype(np.float64), ref, bn, True), K)
    want = w.grad[:, 0, 0].numpy()
    assert np.abs(got - want).max() <= 1e-10 * max(1.0, np.abs(want).max())
    # eval form: dy = scale g
    w.grad = None
    (F.conv2d(xt, w, padding="same") * (gamma * invstd)[None, :, None, None] * g).sum().backward()
    got = R.wgrad_ref(x, R.dy_ref(g1, None, bn, False), K)
    assert np.abs(got - w.grad[:, 0, 0].numpy()).max() <= 1e-10 * max(1.0, np.abs(got).max())


@pytest.mark.parametrize("case", list(R.CASES), ids=str)
def test_each_case_reaches_what_it_is_listed_for(L, case):
    B, C, S, K, cap = case
    set_cap(L, cap)
    try:
        got = dict(zip(R.PLAN_FIELDS, R.export_plan(L, B, C, S, K)))
        assert tuple(got.values()) == R.plan(B, C, S, K, cap)
        facts = R.case_facts(case)
        for k in ("npair", "nmb", "nmain", "ntail", "npk", "t0t", "fwd_wgs", "wg_wgs"):
            assert facts[k] == got[k], k
        assert facts["groups"] == got["wg_groups"]
        assert L.plain("eav_eegnet_fir_fwd_fft_nparts", B, C, S) == facts["nparts"]
        for k, v in R.CASES[case].items():
            assert facts[k] == v, (k, facts[k], v)
    finally:
        set_cap(L, None)
    if cap is None:      # the hook is off by default: the plan of a library nobody has touched
        assert got["fwd_wgs"] == min(256, max(1, -(-(got["nmain"] + got["npk"]) // 12)))


def owners(B, C, S, K):
    q = R.units(B, C, S, K)
    n = q["nmain"] + q["npk"]
    seen = np.zeros((B, q["npair"], q["nblk"]), int)
    for u in range(n):
        for b, pr, blk, slot in R.unit_members(q, u):
            seen[b, pr, blk] += 1
            assert slot == 0 or (slot == 512 and u >= q["nmain"])
    assert (seen == 1).all(), "a (sample, pair, block) is owned by no unit or by two"
    return q, n


def test_plan_export_deal_and_sizes_over_the_sweep(L):
    combos = R.sweep()
    assert len(combos) >= 3000
    units_of = {}
    try:
        for B, C, S, K, cap in combos:
            set_cap(L, cap)
            what = (B, C, S, K, cap)
            got = R.export_plan(L, B, C, S, K)
            assert got == R.plan(B, C, S, K, cap), what
            if (B, C, S, K) not in units_of:
                units_of[(B, C, S, K)] = owners(B, C, S, K)
            q, n = units_of[(B, C, S, K)]
            fwd_wgs, groups, wg_wgs = got[6], got[7], got[8]
            assert 1 <= fwd_wgs <= (cap or 256) and 1 <= wg_wgs <= (cap or 256), what
            # every unit on exactly one wave, every group on exactly one workgroup
            dealt = np.bincount(np.concatenate([np.asarray(w, int) for w in R.fwd_deal(n, fwd_wgs)]), minlength=n)
            assert (dealt == 1).all(), what
            walked = [u for w in R.wgrad_walk(q, wg_wgs) for _, us in w for u in us]
            assert sorted(walked) == list(range(n)), what
            # the sizing exports do not know K: they must cover the grids of this K
            nparts, ws = L.plain("eav_eegnet_fir_fwd_fft_nparts", B, C, S), L.plain("eav_eegnet_fir_wgrad_fft_ws_floats", B, C, S)
            assert nparts == R.nparts(B, C, S, cap) and nparts >= 12 * fwd_wgs, what
            assert ws == R.ws_floats(B, C, S, cap) and ws >= (wg_wgs + 1) * 8 * 2 * 1024, what
            # the float64 tables of the table form start behind ws: 8-byte aligned
            assert (4 * ws) % 8 == 0, what
            assert L.plain("eav_eegnet_fir_wgrad_fft_xtab_ws_floats", B, C, S, K) == ws + 2 * (K * K + K), what
    finally:
        set_cap(L, None)


def test_fewer_groups_can_mean_more_workgroups(L):
    """13920 units = 1740 groups walk on 249 workgroups, the 1800 groups of the never-packing list on 225: the workspace is
    sized by the larger grid, not by the larger list"""
    assert R.fft_grid(1740) == 249 and R.fft_grid(1800) == 225
    assert L.plain("eav_eegnet_fir_wgrad_fft_ws_floats", 64, 30, 10000) == 250 * 8 * 2 * 1024
    assert R.export_plan(L, 64, 30, 10000, 300)[6:] == (256, 1740, 249)


def test_plan_export_rejects_what_the_launchers_reject(L):
    for args in ((1, 1, 1, 322), (1, 1, 1, 0), (0, 1, 1, 3), (1, 0, 1, 3), (1, 1, 0, 3)):
        with pytest.raises(L.EavError):
            R.export_plan(L, *args)
    with pytest.raises(L.EavError):
        L.call("eav_eegnet_fir_fft_plan", 1, 1, 1, 1, None)


WORST = {}


@pytest.mark.parametrize("case", list(R.CASES), ids=str)
def test_complex64_restatement_stays_within_the_bound(case):
    B, C, S, K, cap = case
    xs, idx, x, w, g1, y1, bn = R.normal_inputs(case)
    ratio = float((np.abs(R.fwd_c64(x, w) - R.fwd_ref(x, w)) / R.fwd_bound(x, w)).max())
    WORST["fwd"] = max(WORST.get("fwd", 0.0), ratio)
    assert ratio <= 1.0
    for train in (True, False):
        ref = R.wgrad_ref(x, R.dy_ref(g1, y1, bn, train), K)
        got = R.wgrad_c64(x, R.dy_f32(g1, y1, bn, train), K, cap)
        r = float((np.abs(got - ref) / R.wgrad_bound(x, g1, y1, bn, K, train, cap)).max())
        WORST["wgrad"] = max(WORST.get("wgrad", 0.0), r)
        assert r <= 1.0
    print(f"complex64 restatement, worst error / bound so far: {WORST}")


def test_structured_inputs_are_exact_shifts():
    """the impulse data: every reference output is an integer, and the complex64 restatement leaks less than the bound"""
    for case in R.CASES:
        x, w = R.impulse_inputs(case)
        ref = R.fwd_ref(x, w)
        assert np.abs(ref - np.rint(ref)).max() < 1e-9 and np.abs(ref).max() >= 1.0
        assert (np.abs(R.fwd_c64(x, w) - np.rint(ref)) <= R.fwd_bound(x, w)).all()
