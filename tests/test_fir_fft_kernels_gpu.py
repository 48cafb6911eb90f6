"""The FFT FIR kernels (csrc/eegnet_fir_fft.hip) through the C ABI against tests/fir_fft_ref.py: eav_eegnet_fir_fwd_fft
(with and without stat_part, indexed and not), eav_eegnet_fir_wgrad_fft (train and eval) and eav_eegnet_fir_wgrad_fft_xtab.

The persistent loops of both kernels - rounds of the forward's deal, its prefetch chain and its switch from main to packed
units, the weight gradient's walk over several groups per workgroup - need more units than 256 workgroups hold; the cases
reach them at a few hundred kilobytes by lowering the grids with eav_eegnet_fir_fft_set_grid_cap.  Every case asserts from
eav_eegnet_fir_fft_plan that it runs the deal it is listed for (tests/test_fir_fft_ref_cpu.py asserts the listed property).

"normal" data: every element within the a-priori bound of the reference module, and the RMS error of a case at most twice
that of the complex64 restatement of the algorithm on the same inputs.  "structured" data: impulses at the block edges
against impulse filters (the reference is a shifted copy, everything else 0 to within the bound), one pure tone per bin
class, and a quiet electrode beside a loud one.  Every output starts as a NaN sentinel with a guard band.

The module prints, per entry point, the number of checks, the worst error / bound, the worst RMS ratio against the
complex64 yardstick, and the time spent per test function.

Measured on an MI355X (60 tests, 4.4 s): RMS ratios 0.98 - 1.06 for the forward, 0.57 - 1.21 for the three weight-gradient
forms; worst error / bound 0.011 (y1), 0.049 (the statistics), 0.001 (dW).  Quiet electrode (1e-3) beside a loud one (1e3):
RMS error / own RMS magnitude 9.4e-2 for the FFT kernel against 3.0e-7 for the direct one (loud electrode: 1.7e-7 / 3.0e-7;
a quiet electrode alone in its pair, sharing only packed tails: 9.3e-3) - the price of the design, within its bound."""
import functools
import time

import numpy as np
import pytest
import torch

from tests import fir_fft_ref as R
from tests.kernel_check import SENT, dev, ptr, same, sentinel_buf, take, within

pytestmark = pytest.mark.gpu

WORST, RMS, COUNT, SPENT = {}, {}, {}, {}
RMS_MARGIN = 2.0      # another correct factorisation of the same depth: the expected ratio is about 1 (reference module)
ALL = list(R.CASES)


@pytest.fixture(scope="module")
def L():
    from eav_amd import _lib
    _lib.load()
    yield _lib
    _lib.load().eav_eegnet_fir_fft_set_grid_cap(0)
    print("\nentry point: checks, worst error / bound, worst RMS error / RMS error of the complex64 restatement")
    for k in sorted(COUNT):
        print(f"  {k}: {COUNT[k]}, {WORST.get(k, 0.0):.5f}, {RMS.get(k, float('nan')):.3f}")
    print("test: seconds")
    for k in sorted(SPENT):
        print(f"  {k}: {SPENT[k]:.1f}")
    print(f"  total: {sum(SPENT.values()):.1f} s")


@pytest.fixture(autouse=True)
def _clock_and_cap(request):
    t0 = time.perf_counter()
    yield
    from eav_amd import _lib
    _lib.load().eav_eegnet_fir_fft_set_grid_cap(0)
    name = request.node.originalname or request.node.name
    SPENT[name] = SPENT.get(name, 0.0) + time.perf_counter() - t0


def set_cap(L, cap):
    assert L.load().eav_eegnet_fir_fft_set_grid_cap(cap or 0) == 0


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def check_bound(kernel, what, got, ref, bound):
    COUNT[kernel] = COUNT.get(kernel, 0) + 1
    ref, bound = t64(ref), t64(bound).expand(ref.shape)
    ratio = float(((got.double() - ref).abs() / bound.clamp_min(1e-300)).max())
    WORST[kernel] = max(WORST.get(kernel, 0.0), ratio)
    print(f"{kernel} {what}: worst error / bound {ratio:.5f}")
    within(got, ref, bound, f"{kernel} {what}")


def rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, np.float64)))))


def rms_ratio(got, ref, yard):
    e, ey = rms(got.double().numpy() - ref), rms(yard.astype(np.float64) - ref)
    return (e / ey if ey > 0 else (0.0 if e == 0 else float("inf"))), e, ey


def check_rms(kernel, what, got, ref, yard):
    ratio, e, ey = rms_ratio(got, ref, yard)
    RMS[kernel] = max(RMS.get(kernel, 0.0), ratio)
    print(f"{kernel} {what}: RMS error {e:.3e}, complex64 restatement {ey:.3e}, ratio {ratio:.3f}")
    assert ratio <= RMS_MARGIN, f"{kernel} {what}: RMS error {e:.3e} is {ratio:.2f} x the complex64 restatement's {ey:.3e}"


def assert_plan(L, case):
    """the cap is set and the launchers' own plan is the one the case is listed for"""
    B, C, S, K, cap = case
    set_cap(L, cap)
    got = R.export_plan(L, B, C, S, K)
    assert got == R.plan(B, C, S, K, cap), (got, R.plan(B, C, S, K, cap))
    facts = R.case_facts(case)
    for k, v in R.CASES[case].items():
        assert facts[k] == v, (k, facts[k], v)
    return dict(zip(R.PLAN_FIELDS, got))


def unchanged(d, h, what):
    assert torch.equal(d.cpu(), torch.from_numpy(h)), f"{what}: an input was written"


# --------------------------------------------------------------------------------------------------------------- forward
def fwd(L, xd, idxd, wd, B, C, S, K, stats):
    """one call on sentinel buffers -> (y1, stat_part or None) on the host, everything promised written, nothing beyond"""
    n = B * 8 * C * S
    y = sentinel_buf(n)
    nparts = L.plain("eav_eegnet_fir_fwd_fft_nparts", B, C, S)
    part = sentinel_buf(nparts * 16) if stats else None
    L.call("eav_eegnet_fir_fwd_fft", ptr(xd), ptr(idxd), ptr(wd), ptr(y), ptr(part), B, C, S, K, None)
    return take(y, n, (B, 8, C, S), "y1"), (take(part, nparts * 16, (nparts, 16), "stat_part") if stats else None)


@functools.lru_cache(maxsize=None)
def fwd_refs(case):
    xs, idx, x, w, _, _, _ = R.normal_inputs(case)
    return R.fwd_ref(x, w), R.fwd_bound(x, w), R.fwd_c64(x, w)


def check_stats(case, plan, y, part, ref, bound, k):
    B, C, S, K, cap = case
    own = 12 * plan["fwd_wgs"]
    assert part.shape[0] >= own
    tail = part[own:].contiguous().view(torch.int32)
    assert bool((tail == 0).all()), "stat_part rows without a wave are not exact zeros"
    st = part.double().sum(0)
    yd = y.double()
    # (a) against float64 sums of the kernel's OWN output: only the order of fp32 additions lies between them - a chain
    # of n additions of terms t_i errs by at most n u sum |t_i| (1 % for the higher orders)
    tol = 1.01 * R.stat_chain(B, C, S, K, cap) * R.U
    check_bound(k, f"{case} sum vs own output", st[:8], yd.sum((0, 2, 3)).numpy(), tol * yd.abs().sum((0, 2, 3)).numpy())
    check_bound(k, f"{case} sum of squares vs own output", st[8:], (yd * yd).sum((0, 2, 3)).numpy(),
                tol * (yd * yd).sum((0, 2, 3)).numpy())
    # (b) against the reference's sums: the forward bound of every element on top
    r, b = t64(ref), t64(bound)
    check_bound(k, f"{case} sum vs reference", st[:8], r.sum((0, 2, 3)).numpy(),
                (b.sum((0, 2, 3)) + tol * (r.abs() + b).sum((0, 2, 3))).numpy())
    check_bound(k, f"{case} sum of squares vs reference", st[8:], (r * r).sum((0, 2, 3)).numpy(),
                ((2 * r.abs() * b + b * b).sum((0, 2, 3)) + tol * ((r.abs() + b) ** 2).sum((0, 2, 3))).numpy())


@pytest.mark.parametrize("case", ALL, ids=str)
def test_fwd_normal(L, case):
    B, C, S, K, cap = case
    plan = assert_plan(L, case)
    xs, idx, x, w, _, _, _ = R.normal_inputs(case)
    ref, bound, yard = fwd_refs(case)
    xsd, xd, idxd, wd = dev(xs), dev(x), dev(idx), dev(w)
    first = None
    for stats in (True, False):
        for indexed in (False, True):
            k = "fir_fwd_fft" + ("" if stats else "_nostats") + ("_indexed" if indexed else "")
            y, part = fwd(L, xsd if indexed else xd, idxd if indexed else None, wd, B, C, S, K, stats)
            check_bound(k, f"{case} y1", y, ref, bound)
            check_rms(k, f"{case} y1", y, ref, yard)
            if stats:
                check_stats(case, plan, y, part, ref, bound, k)
            if first is None:
                first = (y, part)
            else:      # statistics, the index and the call count change no arithmetic
                same(y, first[0], f"{k} {case} y1 against the first call")
                if stats:
                    same(part, first[1], f"{k} {case} stat_part against the first call")
    y2, part2 = fwd(L, xd, None, wd, B, C, S, K, True)
    same(y2, first[0], f"{case} y1 of a second call")
    same(part2, first[1], f"{case} stat_part of a second call")
    if cap is not None:      # the deal must not change arithmetic: the natural grid gives the same y1 bits
        set_cap(L, None)
        assert R.export_plan(L, B, C, S, K) == R.plan(B, C, S, K, None)
        y3, part3 = fwd(L, xd, None, wd, B, C, S, K, True)
        same(y3, first[0], f"{case} y1 at the natural grid")
        check_stats((B, C, S, K, None), dict(fwd_wgs=R.plan(B, C, S, K)[6]), y3, part3, ref, bound, "fir_fwd_fft")
    unchanged(xsd, xs, "x")
    unchanged(wd, w, "w1")


# ------------------------------------------------------------------------------------------------------- weight gradient
def wgrad(L, plan, xd, idxd, y1d, g1d, bnd, B, C, S, K):
    ws_n = L.plain("eav_eegnet_fir_wgrad_fft_ws_floats", B, C, S)
    ws, dW = sentinel_buf(ws_n), sentinel_buf(8 * K)
    L.call("eav_eegnet_fir_wgrad_fft", ptr(xd), ptr(idxd), ptr(y1d), ptr(g1d), ptr(bnd), ptr(ws), ptr(dW), B, C, S, K, None)
    written = (plan["wg_wgs"] + 1) * 8 * 2 * 1024       # one spectrum row per workgroup and their sum; nothing behind them
    assert written <= ws_n
    take(ws, written, (plan["wg_wgs"] + 1, 8, 2048), "ws")
    return take(dW, 8 * K, (8, K), "dW")


def wgrad_xtab(L, plan, xd, idxd, tabd, wd, g1d, bnd, B, C, S, K):
    ws_n = L.plain("eav_eegnet_fir_wgrad_fft_xtab_ws_floats", B, C, S, K)
    spec_n = L.plain("eav_eegnet_fir_wgrad_fft_ws_floats", B, C, S)
    assert ws_n == spec_n + 2 * (K * K + K)
    ws, dW = sentinel_buf(ws_n), sentinel_buf(8 * K)
    assert ws.data_ptr() % 8 == 0
    L.call("eav_eegnet_fir_wgrad_fft_xtab", ptr(xd), ptr(idxd), ptr(tabd), ptr(wd), ptr(g1d), ptr(bnd), ptr(ws), ptr(dW),
           B, C, S, K, None)
    out = take(dW, 8 * K, (8, K), "dW")
    bits = ws.cpu().view(torch.int32)
    written = (plan["wg_wgs"] + 1) * 8 * 2 * 1024
    assert not bool((bits[:written] == SENT).any()), "ws: spectrum rows left unwritten"
    assert bool((bits[written:spec_n] == SENT).all()), "ws: written between the spectra and the table sums"
    assert not bool((bits[spec_n:ws_n] == SENT).any()), "ws: table sums left unwritten"
    assert bool((bits[ws_n:] == SENT).all()), "ws: guard band written"
    return out


@functools.lru_cache(maxsize=None)
def wgrad_refs(case, form):
    """(float64 reference, bound, complex64 yardstick) of the train / eval / table form"""
    B, C, S, K, cap = case
    xs, idx, x, w, g1, y1, bn = R.normal_inputs(case)
    if form == "eval":
        return (R.wgrad_ref(x, R.dy_ref(g1, None, bn, False), K), R.wgrad_bound(x, g1, y1, bn, K, False, cap),
                R.wgrad_c64(x, R.dy_f32(g1, None, bn, False), K, cap))
    bound = R.wgrad_bound(x, g1, y1, bn, K, True, cap)
    if form == "train":
        return R.wgrad_ref(x, R.dy_ref(g1, y1, bn, True), K), bound, R.wgrad_c64(x, R.dy_f32(g1, y1, bn, True), K, cap)
    # the table form: y1 is the exact firstConv(x; w); the yardstick takes G from the complex64 walk on the raw g1 and the
    # shares of y1 and of the constant in float64, as the finishing kernels do
    y64 = R.fwd_ref(x, w)
    ref = R.wgrad_ref(x, R.dy_ref(g1, y64, bn, True), K)
    v = lambda o: bn[o:o + 8].astype(np.float64)[:, None]  # noqa: E731
    G = R.wgrad_c64(x, g1, K, cap).astype(np.float64)
    X1 = R.wgrad_ref(x, np.ones_like(y64), K)[:1]
    yard = (v(16) * (G - (v(32) - v(0) * v(8) * v(40)) * X1 - v(8) * v(40) * R.wgrad_ref(x, y64, K))).astype(np.float32)
    return ref, bound, yard


@pytest.mark.parametrize("case", ALL, ids=str)
def test_wgrad_normal(L, case):
    B, C, S, K, cap = case
    plan = assert_plan(L, case)
    xs, idx, x, w, g1, y1, bn = R.normal_inputs(case)
    xsd, xd, idxd, wd, g1d, y1d, bnd = dev(xs), dev(x), dev(idx), dev(w), dev(g1), dev(y1), dev(bn)
    for form in ("train", "eval"):
        ref, bound, yard = wgrad_refs(case, form)
        first = None
        for indexed in (False, True, False):      # (the third: a second call of the first)
            k = "fir_wgrad_fft" + ("" if form == "train" else "_eval") + ("_indexed" if indexed else "")
            dW = wgrad(L, plan, xsd if indexed else xd, idxd if indexed else None, y1d if form == "train" else None, g1d, bnd,
                       B, C, S, K)
            if first is None:
                first = dW
            else:
                same(dW, first, f"{k} {case} dW against the first call")
                if not indexed:
                    continue
            check_bound(k, f"{case} dW", dW, ref, bound)
            check_rms(k, f"{case} dW", dW, ref, yard)
    # the table form on the tables of the whole data set, the batch addressed through the index
    N = xs.shape[0]
    tab = sentinel_buf(L.plain("eav_eegnet_fir_xtab_floats", N, K))
    L.call("eav_eegnet_fir_xtab_build", ptr(xsd), N, C, S, K, ptr(tab), None)
    take(tab, N * (K * K + K), (N, K * K + K), "tables")
    ref, bound, yard = wgrad_refs(case, "xtab")
    a = wgrad_xtab(L, plan, xsd, idxd, tab, wd, g1d, bnd, B, C, S, K)
    b = wgrad_xtab(L, plan, xsd, idxd, tab, wd, g1d, bnd, B, C, S, K)
    same(b, a, f"fir_wgrad_fft_xtab {case} dW of a second call")
    check_bound("fir_wgrad_fft_xtab", f"{case} dW", a, ref, bound)
    check_rms("fir_wgrad_fft_xtab", f"{case} dW", a, ref, yard)
    for d, h, what in ((xsd, xs, "x"), (g1d, g1, "g1"), (y1d, y1, "y1"), (bnd, bn, "bn_params"), (wd, w, "w1")):
        unchanged(d, h, what)


# ------------------------------------------------------------------------------------------------------------ structured
@pytest.mark.parametrize("case", ALL, ids=str)
def test_impulses_come_out_as_shifted_copies(L, case):
    """Unit impulses at t = 0, 703, 704, S - 1, t0t, t0t - padl against impulse filters at tap 0, padl, K - 1: y1 is a
    shifted copy of x and 0 elsewhere - a wrong bin, twiddle or mirrored-bin conjugate leaks into the zeros.  The weight
    gradient of the same impulses (dy = g1 = x's impulses on every filter, eval form with scale 1) counts coincidences."""
    B, C, S, K, cap = case
    plan = assert_plan(L, case)
    x, w = R.impulse_inputs(case)
    ref = np.rint(R.fwd_ref(x, w))
    bound = R.fwd_bound(x, w)
    y, _ = fwd(L, dev(x), None, dev(w), B, C, S, K, False)
    zeros = ref == 0
    if zeros.any():
        print(f"{case}: largest |y1| where the reference is 0: {float(np.abs(y.numpy()[zeros]).max()):.3e} "
              f"(smallest bound there {bound[zeros].min():.3e})")
    check_bound("fir_fwd_fft_impulses", f"{case} y1", y, ref, bound)
    g1 = np.ascontiguousarray(np.broadcast_to(x[:, None], (B, 8, C, S)))
    bn = np.zeros(48, np.float32)
    bn[16:24] = 1.0
    refw = np.rint(R.wgrad_ref(x, g1.astype(np.float64), K))
    dW = wgrad(L, plan, dev(x), None, None, dev(g1), dev(bn), B, C, S, K)
    check_bound("fir_wgrad_fft_impulses", f"{case} dW", dW, refw, R.wgrad_bound(x, g1, None, bn, K, False, cap))


@pytest.mark.parametrize("k", R.TONE_BINS)
@pytest.mark.parametrize("case", R.TONE_CASES, ids=str)
def test_pure_tones(L, case, k):
    """One tone per bin class: DC, the first bin, both neighbours of the mirror and the mirror itself (bins 513 .. 1023 of a
    filter spectrum are read as conjugates of 511 .. 1)"""
    B, C, S, K, cap = case
    assert_plan(L, case)
    x, w = R.tone_inputs(case, k)
    ref = R.fwd_ref(x, w)
    y, _ = fwd(L, dev(x), None, dev(w), B, C, S, K, False)
    ratio, e, ey = rms_ratio(y, ref, R.fwd_c64(x, w))
    print(f"{case} bin {k}: RMS error {e:.3e}, complex64 restatement {ey:.3e}, ratio {ratio:.3f}")
    check_bound("fir_fwd_fft_tones", f"{case} bin {k} y1", y, ref, R.fwd_bound(x, w))


@pytest.mark.parametrize("case", R.RANGE_CASES, ids=str)
def test_quiet_electrode_beside_a_loud_one(L, case):
    """Even electrodes at 1e-3, odd ones at 1e3: the quiet one's outputs must stay within the bound of the PAIR's segment
    norm.  Their error relative to their own magnitude is printed beside the direct kernel's (csrc/eegnet_fir.hip), whose
    error scales with the electrode's own samples: a recorded fact of the design, not an assertion."""
    B, C, S, K, cap = case
    assert_plan(L, case)
    x, w = R.range_inputs(case)
    ref, bound = R.fwd_ref(x, w), R.fwd_bound(x, w)
    xd, wd = dev(x), dev(w)
    y, _ = fwd(L, xd, None, wd, B, C, S, K, False)
    check_bound("fir_fwd_fft_range", f"{case} y1", y, ref, bound)
    n = B * 8 * C * S
    yd, part = sentinel_buf(n), sentinel_buf(L.plain("eav_eegnet_fir_fwd_nparts", B, C, S) * 16)
    L.call("eav_eegnet_fir_fwd", ptr(xd), ptr(wd), ptr(yd), ptr(part), B, C, S, K, None)
    direct = take(yd, n, (B, 8, C, S), "y1 (direct)")
    paired = slice(0, C - (C % 2), 2)                     # quiet electrodes that share their transform with a loud one
    for name, sel in (("quiet beside loud", paired), ("loud", slice(1, C, 2))) + ((("quiet alone", slice(C - 1, C)),) if C % 2 else ()):
        own = rms(ref[:, :, sel])
        e_fft = rms(y.double().numpy()[:, :, sel] - ref[:, :, sel]) / own
        e_dir = rms(direct.double().numpy()[:, :, sel] - ref[:, :, sel]) / own
        print(f"{case} {name}: RMS error / RMS magnitude: FFT kernel {e_fft:.3e}, direct kernel {e_dir:.3e}")


# ------------------------------------------------------------------------------------------------------ rejected arguments
def test_klen_322_is_refused_by_all_three_entry_points(L):
    from eav_amd._lib import EavError
    assert L.plain("eav_eegnet_fir_fft_max_taps") == 321
    n = 1 << 16
    src = dev(torch.zeros(n))
    idx = dev(torch.zeros(4, dtype=torch.int64))
    outs = [sentinel_buf(n, guard=0) for _ in range(3)]
    s, (a, b, c) = ptr(src), [ptr(o) for o in outs]
    for K in (322, 0):
        for args in (("eav_eegnet_fir_fwd_fft", s, ptr(idx), s, a, b, 1, 2, 64, K, None),
                     ("eav_eegnet_fir_wgrad_fft", s, None, s, s, s, a, b, 1, 2, 64, K, None),
                     ("eav_eegnet_fir_wgrad_fft_xtab", s, None, s, s, s, s, a, b, 1, 2, 64, K, None)):
            with pytest.raises(EavError, match="kernLength"):
                L.call(*args)
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o.view(torch.int32) == SENT).all()), "a rejected call wrote to its output"
