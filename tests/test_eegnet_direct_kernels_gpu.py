"""The direct (non-FFT) EEGNet_tor kernels - csrc/eegnet_fir.hip, csrc/eegnet_block.hip, csrc/eegnet_conv64.hip - through
the C ABI against the float64 references of tests/eegnet_direct_ref.py, at the edges of every instantiation and with more
work items than blocks for every persistent kernel.  Every case runs in two data modes (see the reference module): "exact"
must reproduce the float64 result bit for bit, "rounded" must stay within the bound derived there, element by element.
Every output and every partial buffer starts as a NaN sentinel with a guard band: all promised elements must be written,
nothing beyond them.  The plan queries must agree with the thresholds restated in the reference module, so that a case
provably runs the form it is listed for.

The module prints, per kernel, the number of checks and the worst error / bound ratio of the rounded mode, and the time
spent per test function."""
import time

import numpy as np
import pytest
import torch

from tests import eegnet_direct_ref as R
from tests.kernel_check import SENT, dev, normal, ptr, same, sentinel_buf, take, within

pytestmark = pytest.mark.gpu

WORST, COUNT, SPENT = {}, {}, {}


@pytest.fixture(scope="module")
def L():
    from eav_amd import _lib
    _lib.load()
    yield _lib
    print("\nkernel: checks, worst error / bound (rounded mode)")
    for k in sorted(COUNT):
        print(f"  {k}: {COUNT[k]}, {WORST.get(k, 0.0):.3f}")
    print("test: seconds")
    for k in sorted(SPENT):
        print(f"  {k}: {SPENT[k]:.1f}")
    print(f"  total: {sum(SPENT.values()):.1f} s")


@pytest.fixture(autouse=True)
def _clock(request):
    t0 = time.perf_counter()
    yield
    name = request.node.originalname or request.node.name
    SPENT[name] = SPENT.get(name, 0.0) + time.perf_counter() - t0


def check(mode, got, ref, bound, what, kernel):
    COUNT[kernel] = COUNT.get(kernel, 0) + 1
    if mode == "exact":
        same(got, ref, f"{kernel} {what}")
        return
    err = (got.double() - ref.double()).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                            torch.zeros_like(err)))
    WORST[kernel] = max(WORST.get(kernel, 0.0), float(ratio.max()))
    print(f"{kernel} {what}: worst error / bound {float(ratio.max()):.3f}")
    within(got, ref, bound, f"{kernel} {what}")


def unchanged(d, h, what):
    assert torch.equal(d.cpu(), h), f"{what}: an input was written"


def plan(L, S, K, what):
    return L.plain("eav_eegnet_fir_plan", S, K, what)


FWD_NSTEP, FWD_NSEG, WG_NCHUNK, WG_CH, WG_NT, INF_NSEG = range(6)


# ----------------------------------------------------------------------------------------------------- firstConv
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", R.FIR_FWD_CASES, ids=str)
def test_fir_fwd(L, case, mode):
    B, C, S, K = case
    assert plan(L, S, K, FWD_NSTEP) == R.fir_nstep(K) and plan(L, S, K, FWD_NSEG) == R.fir_nseg(S)
    npart = L.plain("eav_eegnet_fir_fwd_nparts", B, C, S)
    assert npart == R.fir_fwd_grid(B, C, S)
    xs, idx, w = R.fir_inputs(mode, B, C, S, K)
    x = xs[idx]
    ref = R.fir_fwd_ref(x, w, R.fir_fwd_visits(B, C, S))
    xsd, xd, idxd, wd = dev(xs), dev(x), dev(idx), dev(w)
    for indexed in (False, True):
        y, part = sentinel_buf(B * 8 * C * S), sentinel_buf(npart * 16)
        if indexed:
            L.call("eav_eegnet_fir_fwd_indexed", ptr(xsd), ptr(idxd), ptr(wd), ptr(y), ptr(part), B, C, S, K, None)
        else:
            L.call("eav_eegnet_fir_fwd", ptr(xd), ptr(wd), ptr(y), ptr(part), B, C, S, K, None)
        k = "fir_fwd_indexed" if indexed else "fir_fwd"
        check(mode, take(y, B * 8 * C * S, (B, 8, C, S), "y1"), ref["y"], ref["y_bound"], f"{case} y1", k)
        st = take(part, npart * 16, (npart, 16), "stat_part").double().sum(0)
        check(mode, st[:8], ref["s"], ref["s_bound"], f"{case} sum", k)
        check(mode, st[8:], ref["q"], ref["q_bound"], f"{case} sum of squares", k)
    unchanged(xsd, xs, "fir_fwd_indexed x")


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", R.FIR_WGRAD_CASES, ids=str)
def test_fir_wgrad(L, case, mode):
    B, C, S, K = case
    nchunk, CH = R.wgrad_geometry(S)
    assert (plan(L, S, K, WG_NCHUNK), plan(L, S, K, WG_CH), plan(L, S, K, WG_NT)) == (nchunk, CH, R.wgrad_nt(K))
    npart = L.plain("eav_eegnet_fir_wgrad_nparts", B, C, S)
    assert npart == R.wgrad_grid(B, C, S)
    xs, idx, y1, g1, bn = R.fir_wgrad_inputs(mode, B, C, S, K)
    x = xs[idx]
    xsd, xd, idxd, y1d, g1d, bnd = dev(xs), dev(x), dev(idx), dev(y1), dev(g1), dev(bn)
    for train in (True, False):
        ref = R.fir_wgrad_ref(x, y1, g1, bn, K, train, mode)
        for indexed in (False, True):
            part = sentinel_buf(npart * 8 * K)
            yp = ptr(y1d) if train else None
            if indexed:
                L.call("eav_eegnet_fir_wgrad_indexed", ptr(xsd), ptr(idxd), yp, ptr(g1d), ptr(bnd), ptr(part), B, C, S, K, None)
            else:
                L.call("eav_eegnet_fir_wgrad", ptr(xd), yp, ptr(g1d), ptr(bnd), ptr(part), B, C, S, K, None)
            dW = take(part, npart * 8 * K, (npart, 8, K), "part").double().sum(0)
            k = "fir_wgrad" + ("" if train else "_eval") + ("_indexed" if indexed else "")
            check(mode, dW, ref["dW"], ref["bound"], f"{case} dW1", k)
    unchanged(xsd, xs, "x")
    unchanged(y1d, y1, "y1")
    unchanged(g1d, g1, "g1")


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", R.INFER_CASES, ids=str)
def test_block1_infer(L, case, mode):
    B, C, S, K = case
    assert plan(L, S, K, FWD_NSTEP) == R.fir_nstep(K) and plan(L, S, K, INF_NSEG) == R.infer_nseg(S)
    assert L.plain("eav_eegnet_block1_infer_nblocks", B, S) == R.infer_grid(B, S)
    xs, idx, w1, bn1, w2, bn2 = R.block1_inputs(mode, B, C, S, K)
    x = xs[idx]
    ref = R.block1_infer_ref(x, w1, bn1, w2, bn2)
    xsd, xd, idxd = dev(xs), dev(x), dev(idx)
    w1d, bn1d, w2d, bn2d = dev(w1), dev(bn1[:4]), dev(w2), dev(bn2[:4])        # the blocks of eav_bn_finalize(training = 0)
    n = B * 64 * (S // 4)
    for indexed in (False, True):
        p2 = sentinel_buf(n)
        L.call("eav_eegnet_block1_infer", ptr(xsd if indexed else xd), ptr(idxd) if indexed else None, ptr(w1d), ptr(bn1d),
               ptr(w2d), ptr(bn2d), ptr(p2), B, C, S, K, None)
        check(mode, take(p2, n, (B, 64, S // 4), "p2"), ref["p"], ref["bound"], f"{case} p2",
              "block1_infer" + ("_indexed" if indexed else ""))
    unchanged(xsd, xs, "x")


# ------------------------------------------------------------------------------------------------ depthwise passes
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", R.DW_CASES, ids=str)
def test_dw_fwd(L, case, mode):
    B, C, S = case
    assert L.plain("eav_eegnet_dw_plan", S) == R.dw_plan(S)
    y1, bn1, w2, bn2, _ = R.dw_inputs(mode, B, C, S)
    nchunk = R.cdiv(S, 1024)
    forms = [False, True] if S % 4 == 0 else [False]
    ref = R.dw_fwd_ref(y1, bn1, w2, bn2 if S % 4 == 0 else None)
    y1d, bn1d, w2d, bn2d = dev(y1), dev(bn1), dev(w2), dev(bn2[:4])
    for pool in forms:
        z, part, p2 = sentinel_buf(B * 64 * S), sentinel_buf(B * nchunk * 128), sentinel_buf(B * 64 * (S // 4))
        if pool:
            L.call("eav_eegnet_dw_fwd_pool_eval", ptr(y1d), ptr(bn1d), ptr(w2d), ptr(z), ptr(part), ptr(bn2d), ptr(p2), B, C, S, None)
        else:
            L.call("eav_eegnet_dw_fwd", ptr(y1d), ptr(bn1d), ptr(w2d), ptr(z), ptr(part), B, C, S, None)
        k = "dw_fwd_pool_eval" if pool else "dw_fwd"
        check(mode, take(z, B * 64 * S, (B, 64, S), "z"), ref["z"], ref["z_bound"], f"{case} z", k)
        st = take(part, B * nchunk * 128, (B, nchunk, 128), "stat_part")
        check(mode, st[:, :, :64], ref["s"], ref["s_bound"], f"{case} sum z", k)
        check(mode, st[:, :, 64:], ref["q"], ref["q_bound"], f"{case} sum z^2", k)
        if pool:
            check(mode, take(p2, B * 64 * (S // 4), (B, 64, S // 4), "p2"), ref["p"], ref["p_bound"], f"{case} p2", k)
    unchanged(y1d, y1, "y1")


def dw_bwd_outputs(B, C, S):
    nchunk = R.cdiv(S, 1024)
    return sentinel_buf(B * 8 * C * S), sentinel_buf(B * nchunk * 16), sentinel_buf(B * nchunk * 64 * C)


def check_dw_bwd(mode, ref, bufs, B, C, S, what, k):
    nchunk = R.cdiv(S, 1024)
    g1, pst, pw = bufs
    check(mode, take(g1, B * 8 * C * S, (B, 8, C, S), "g1"), ref["g1"], ref["g1_bound"], f"{what} g1", k)
    check(mode, take(pst, B * nchunk * 16, (B, nchunk, 16), "stat_part"), ref["st"], ref["st_bound"], f"{what} sums", k)
    check(mode, take(pw, B * nchunk * 64 * C, (B, nchunk, 64 * C), "w_part"), ref["dW"], ref["dW_bound"], f"{what} dW2", k)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", R.DW_CASES, ids=str)
def test_dw_bwd(L, case, mode):
    B, C, S = case
    y1, bn1, w2, _, dz = R.dw_inputs(mode, B, C, S)
    ref = R.dw_bwd_ref(y1, dz, None, bn1, w2)
    bufs = dw_bwd_outputs(B, C, S)
    L.call("eav_eegnet_dw_bwd", ptr(dev(y1)), ptr(dev(dz)), ptr(dev(bn1)), ptr(dev(w2)), *[ptr(b) for b in bufs], B, C, S, None)
    check_dw_bwd(mode, ref, bufs, B, C, S, str(case), "dw_bwd")


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", R.DW_FUSED_CASES, ids=str)
def test_dw_bwd_fused(L, case, mode):
    B, C, S, drop = case
    assert L.plain("eav_eegnet_dw_plan", S) == R.dw_plan(S)
    y1, z, dp2, bn2, bn1, w2, mask = R.dw_fused_inputs(mode, B, C, S, drop)
    mult = R.pool_mult(mask, drop, dp2.shape)
    nchunk = R.cdiv(S, 1024)
    y1d, zd, dpd, bn2d, bn1d, w2d = dev(y1), dev(z), dev(dp2), dev(bn2), dev(bn1), dev(w2)
    maskd = dev(mask) if mask is not None else None
    for train in (True, False):
        ref = R.dw_bwd_fused_ref(y1, z, dp2, bn2, bn1, w2, mult, train)
        bufs = dw_bwd_outputs(B, C, S)
        head = [ptr(y1d), ptr(zd), ptr(dpd), ptr(bn2d), ptr(bn1d), ptr(w2d)] + [ptr(b) for b in bufs]
        if train:
            L.call("eav_eegnet_dw_bwd_fused", *head, B, C, S, drop, 77, ptr(maskd), None, None)
        else:
            p2 = sentinel_buf(B * nchunk * 128)
            L.call("eav_eegnet_dw_bwd_fused_eval", *head, ptr(p2), B, C, S, drop, 77, ptr(maskd), None, None)
        k = "dw_bwd_fused" if train else "dw_bwd_fused_eval"
        check_dw_bwd(mode, ref, bufs, B, C, S, str(case), k)
        if not train:
            check(mode, take(p2, B * nchunk * 128, (B, nchunk, 128), "bn2_part"), ref["p2"], ref["p2_bound"],
                  f"{case} depthwiseBN sums", k)
    unchanged(y1d, y1, "y1")
    unchanged(zd, z, "z")
    unchanged(dpd, dp2, "dp2")


# ----------------------------------------------------------------------------------------------------- pool passes
def run_pool(L, mode, case, u, bn, dp, mult, drop, seed, maskd, seedd, tag=""):
    B, T, P, _ = case
    To = T // P
    ud, bnd, dpd = dev(u), dev(bn), dev(dp)
    tail = (drop, seed, ptr(maskd), ptr(seedd), None)
    if tag == "":                                    # (the generator case runs the forward itself, to read the mask back)
        out = sentinel_buf(B * 64 * To)
        L.call("eav_bn_elu_pool_fwd", ptr(ud), ptr(bnd), ptr(out), B, 64, T, P, *tail)
        ref = R.pool_fwd_ref(u, bn, P, mult)
        check(mode, take(out, B * 64 * To, (B, 64, To), "out"), ref["out"], ref["bound"], f"{case} out", "pool_fwd")
    r = R.pool_bwd_ref(dp, u, bn, P, mult)
    sums = R.pool_sums(r, R.pool_chain(T, P, False))
    part = sentinel_buf(B * 128)
    L.call("eav_bn_elu_pool_bwd_reduce", ptr(dpd), ptr(ud), ptr(bnd), ptr(part), B, 64, T, P, *tail)
    ph = take(part, B * 128, (B, 2, 64), "part")
    check(mode, ph[:, 0], sums["s"], sums["s_bound"], f"{case} sum g", "pool_bwd_reduce" + tag)
    check(mode, ph[:, 1], sums["q"], sums["q_bound"], f"{case} sum g uhat", "pool_bwd_reduce" + tag)
    du = sentinel_buf(B * 64 * T)
    L.call("eav_bn_elu_pool_bwd_apply", ptr(dpd), ptr(ud), ptr(bnd), ptr(bnd) + 4 * 4 * 64, ptr(du), B, 64, T, P, *tail)
    duh = take(du, B * 64 * T, (B, 64, T), "du")
    check(mode, duh, r["du"], r["e_du"], f"{case} du", "pool_bwd_apply" + tag)
    r0 = R.pool_bwd_ref(dp, u, bn, P, mult, train=False)
    sums0 = R.pool_sums(r0, R.pool_chain(T, P, True))
    du2, part2 = sentinel_buf(B * 64 * T), sentinel_buf(B * 128)
    L.call("eav_bn_elu_pool_bwd_eval", ptr(dpd), ptr(ud), ptr(bnd), ptr(du2), ptr(part2), B, 64, T, P, *tail)
    du2h = take(du2, B * 64 * T, (B, 64, T), "du (eval)")
    check(mode, du2h, r0["du"], r0["e_du"], f"{case} du", "pool_bwd_eval" + tag)
    ph = take(part2, B * 128, (B, 2, 64), "part (eval)")
    check(mode, ph[:, 0], sums0["s"], sums0["s_bound"], f"{case} sum g", "pool_bwd_eval" + tag)
    check(mode, ph[:, 1], sums0["q"], sums0["q_bound"], f"{case} sum g uhat", "pool_bwd_eval" + tag)
    unchanged(ud, u, "u")
    unchanged(dpd, dp, "dp")
    return duh, du2h


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", R.POOL_CASES, ids=str)
def test_pool_passes(L, case, mode):
    B, T, P, drop = case
    u, bn, dp, mask = R.pool_inputs(mode, B, T, P, drop)
    run_pool(L, mode, case, u, bn, dp, R.pool_mult(mask, drop, dp.shape), drop, 0, dev(mask) if mask is not None else None, None)


def test_pool_generator_mask_is_the_same_in_all_four_kernels(L):
    """No mask: the keep decisions come from the counter-based generator keyed by seed + 2 * (device counter).  The zeros of
    the forward output ARE the mask (an ELU mean is zero with probability 0); the three backward kernels must drop the same
    windows - their results are held to the reference evaluated with that mask - and, with m1 = m2 = 0, must leave exact
    zeros on exactly those windows."""
    case = (3, 1028, 4, 0.5)
    B, T, P, drop = case
    u, bn, dp, _ = R.pool_inputs("rounded", B, T, P, drop)
    bn[4:] = 0.0
    To = T // P
    seedd = dev(torch.tensor([3], dtype=torch.int64))
    out = sentinel_buf(B * 64 * To)
    L.call("eav_bn_elu_pool_fwd", ptr(dev(u)), ptr(dev(bn)), ptr(out), B, 64, T, P, drop, 1234, None, ptr(seedd), None)
    oh = take(out, B * 64 * To, (B, 64, To), "out")
    keep = (oh != 0).to(torch.uint8)
    assert abs(float(keep.float().mean()) - 0.5) < 0.02
    mult = R.pool_mult(keep, drop, dp.shape)
    ref = R.pool_fwd_ref(u, bn, P, mult)
    check("rounded", oh, ref["out"], ref["bound"], f"{case} out", "pool_fwd_generator")
    du, du2 = run_pool(L, "rounded", case, u, bn, dp, mult, drop, 1234, None, seedd, tag="_generator")
    dropped = (keep == 0).repeat_interleave(P, dim=2)
    for d in (du, du2):
        assert torch.equal(d[:, :, :To * P] == 0, dropped), "the backward dropped other windows than the forward"
    out2 = sentinel_buf(B * 64 * To)
    L.call("eav_bn_elu_pool_fwd", ptr(dev(u)), ptr(dev(bn)), ptr(out2), B, 64, T, P, drop, 1234 + 6, None, None, None)
    assert torch.equal(take(out2, B * 64 * To, (B, 64, To), "out"), oh), "seed + 2 * counter is not the effective seed"


# --------------------------------------------------------------------------------------------------- separableConv
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", R.CONV64_CASES, ids=str)
def test_conv64(L, case, mode):
    B, T = case
    assert L.plain("eav_conv64_plan", B, T) == R.conv64_tile(B, T)
    npart, npw = L.plain("eav_conv64_fwd_nparts", B, T), L.plain("eav_conv64_wgrad_nparts", B, T)
    assert (npart, npw) == (R.conv64_fwd_grid(B, T), R.conv64_wgrad_grid(B, T))
    x, w, du = R.conv64_inputs(mode, B, T)
    xd, wd, dud = dev(x), dev(w), dev(du)
    wTf, wTb = sentinel_buf(65536), sentinel_buf(65536)
    L.call("eav_conv64_prep_weights", ptr(wd), ptr(wTf), ptr(wTb), None)
    rf, rbk = R.conv64_prep_ref(w)
    COUNT["conv64_prep_weights"] = COUNT.get("conv64_prep_weights", 0) + 1
    same(take(wTf, 65536, (1024, 64), "wT_fwd"), rf, "wT_fwd")
    same(take(wTb, 65536, (1024, 64), "wT_bwd"), rbk, "wT_bwd")
    n = B * 64 * T
    ref = R.conv64_fwd_ref(x, w, R.conv64_visits(B, T))
    out, part = sentinel_buf(n), sentinel_buf(npart * 128)
    L.call("eav_conv64_fwd", ptr(xd), ptr(wTf), ptr(out), ptr(part), B, T, 7, None)
    check(mode, take(out, n, (B, 64, T), "out"), ref["out"], ref["bound"], f"{case} out", "conv64_fwd")
    st = take(part, npart * 128, (npart, 128), "stat_part").double().sum(0)
    check(mode, st[:64], ref["s"], ref["s_bound"], f"{case} sum", "conv64_fwd")
    check(mode, st[64:], ref["q"], ref["q_bound"], f"{case} sum of squares", "conv64_fwd")
    ref = R.conv64_dgrad_ref(du, w)
    dx = sentinel_buf(n)
    L.call("eav_conv64_fwd", ptr(dud), ptr(wTb), ptr(dx), None, B, T, 8, None)
    check(mode, take(dx, n, (B, 64, T), "dx"), ref["out"], ref["bound"], f"{case} dx", "conv64_dgrad")
    ref = R.conv64_wgrad_ref(du, x)
    pw = sentinel_buf(npw * 65536)
    L.call("eav_conv64_wgrad", ptr(dud), ptr(xd), ptr(pw), B, T, 7, None)
    dW = take(pw, npw * 65536, (npw, 64, 64, 16), "part").double().sum(0)
    check(mode, dW, ref["dW"], ref["bound"], f"{case} dW", "conv64_wgrad")
    unchanged(xd, x, "x")
    unchanged(dud, du, "du")


def test_step_prologue_prepares_the_weights_and_counts_the_given_counters(L):
    w = normal(5, (64, 64, 16))
    rf, rbk = R.conv64_prep_ref(w)
    wd = dev(w)
    cnt = dev(torch.tensor([5, 0, 41, 7, -1], dtype=torch.int64))
    c = cnt.data_ptr()
    for rep, args in enumerate([(c, None, c + 16, c + 24), (None, c + 8, None, None), (None, None, None, None)]):
        wTf, wTb = sentinel_buf(65536), sentinel_buf(65536)
        L.call("eav_eegnet_step_prologue", ptr(wd), ptr(wTf), ptr(wTb), *args, None)
        same(take(wTf, 65536, (1024, 64), "wT_fwd"), rf, "wT_fwd")
        same(take(wTb, 65536, (1024, 64), "wT_bwd"), rbk, "wT_bwd")
        assert cnt.tolist() == [[6, 0, 42, 8, -1], [6, 1, 42, 8, -1], [6, 1, 42, 8, -1]][rep]


# ------------------------------------------------------------------------------------------------ rejected arguments
def test_bad_arguments_are_rejected_before_any_launch(L):
    """kernLength outside [1, 300], more than 32 electrodes, a pool width other than 4 / 8, S % 4 != 0 where a thread's four
    samples are one pooling window, fewer than four samples for the fused backward, dropout p >= 1: an error status, and not
    one word of the output buffers written."""
    from eav_amd._lib import EavError
    n = 1 << 20
    src = dev(torch.zeros(n))
    idx = dev(torch.zeros(8, dtype=torch.int64))
    mask = dev(torch.ones(n, dtype=torch.uint8))
    outs = [sentinel_buf(n, guard=0) for _ in range(4)]
    s, (a, b, c, d) = ptr(src), [ptr(o) for o in outs]
    bad = []
    for K in (0, 301):
        bad += [("eav_eegnet_fir_fwd", s, s, a, b, 1, 2, 8, K, None),
                ("eav_eegnet_fir_fwd_indexed", s, ptr(idx), s, a, b, 1, 2, 8, K, None),
                ("eav_eegnet_fir_wgrad", s, s, s, s, a, 1, 2, 8, K, None),
                ("eav_eegnet_fir_wgrad_indexed", s, ptr(idx), None, s, s, a, 1, 2, 8, K, None),
                ("eav_eegnet_block1_infer", s, None, s, s, s, s, a, 1, 2, 8, K, None)]
    bad += [("eav_eegnet_block1_infer", s, None, s, s, s, s, a, 1, 33, 8, 9, None),
            ("eav_eegnet_dw_fwd", s, s, s, a, b, 1, 33, 8, None),
            ("eav_eegnet_dw_fwd_pool_eval", s, s, s, a, b, s, c, 1, 33, 8, None),
            ("eav_eegnet_dw_bwd", s, s, s, s, a, b, c, 1, 33, 8, None),
            ("eav_eegnet_dw_bwd_fused", s, s, s, s, s, s, a, b, c, 1, 33, 8, 0.0, 0, None, None, None),
            ("eav_eegnet_dw_bwd_fused_eval", s, s, s, s, s, s, a, b, c, d, 1, 33, 8, 0.0, 0, None, None, None)]
    bad += [("eav_bn_elu_pool_fwd", s, s, a, 1, 64, 20, 5, 0.0, 0, None, None, None),
            ("eav_bn_elu_pool_bwd_reduce", s, s, s, a, 1, 64, 20, 5, 0.0, 0, None, None, None),
            ("eav_bn_elu_pool_bwd_apply", s, s, s, s, a, 1, 64, 20, 5, 0.0, 0, None, None, None),
            ("eav_bn_elu_pool_bwd_eval", s, s, s, a, b, 1, 64, 20, 5, 0.0, 0, None, None, None)]
    bad += [("eav_eegnet_block1_infer", s, None, s, s, s, s, a, 1, 2, S, 9, None) for S in (6, 3)]
    bad += [("eav_eegnet_dw_fwd_pool_eval", s, s, s, a, b, s, c, 1, 2, 6, None),
            ("eav_eegnet_dw_bwd_fused", s, s, s, s, s, s, a, b, c, 1, 2, 3, 0.0, 0, None, None, None),
            ("eav_eegnet_dw_bwd_fused_eval", s, s, s, s, s, s, a, b, c, d, 1, 2, 3, 0.0, 0, None, None, None)]
    for p in (1.0, 1.5, -1.0):
        bad += [("eav_bn_elu_pool_fwd", s, s, a, 1, 64, 16, 4, p, 0, ptr(mask), None, None),
                ("eav_bn_elu_pool_bwd_reduce", s, s, s, a, 1, 64, 16, 4, p, 0, ptr(mask), None, None),
                ("eav_bn_elu_pool_bwd_apply", s, s, s, s, a, 1, 64, 16, 4, p, 0, ptr(mask), None, None),
                ("eav_bn_elu_pool_bwd_eval", s, s, s, a, b, 1, 64, 16, 4, p, 0, ptr(mask), None, None),
                ("eav_eegnet_dw_bwd_fused", s, s, s, s, s, s, a, b, c, 1, 2, 8, p, 0, ptr(mask), None, None),
                ("eav_eegnet_dw_bwd_fused_eval", s, s, s, s, s, s, a, b, c, d, 1, 2, 8, p, 0, ptr(mask), None, None)]
    for name, *args in bad:
        with pytest.raises(EavError):
            L.call(name, *args)
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o.view(torch.int32) == SENT).all()), "a rejected call wrote to its output"
    assert float(src.abs().max()) == 0.0
    assert np.all([L.plain("eav_eegnet_fir_plan", 8, K, 0) == 0 for K in (0, 301)]) and L.plain("eav_eegnet_dw_plan", 0) == 0
