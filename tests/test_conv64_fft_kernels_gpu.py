"""The frequency-domain separableConv kernels (csrc/eegnet_conv64_fft.hip) through the C ABI against
tests/conv64_fft_ref.py: eav_conv64_fft_fwd (forward with and without stat_part, data gradient on its own and on the
forward's filter spectra), eav_conv64_fft_wgrad and eav_conv64_fft_bwd (from du, and from dp3 / u3 with du formed while
loading).

Every case runs the calls in the model's order on ONE workspace: forward, forward without statistics, bwd = 2, bwd = 1 on a
fresh workspace (bit-equal), the weight gradient twice (bit-equal), the fused backward from du (bit-equal to the separate
calls) and from dp (no dropout, mask) - the last against float64 end to end.  out, dx, dW and stat_part start as NaN
sentinels with a guard band; the workspace is sentinel-filled too, with a guard band past eav_conv64_fft_ws_floats: no entry
point may depend on what it held (the weight-gradient GEMM contracts over the zero padding columns the pack kernels must
write), and the forward's input spectra must survive everything that follows.  Every case asserts from the two sizing
exports that it runs the column class it is listed for (tests/test_conv64_fft_ref_cpu.py asserts the listed property).

Checks: every element within the a-priori bound of the reference module; on "normal", "dc" and "tone" data the RMS error of
out, dx and dW at most twice that of the float32 restatement of the algorithm on the same inputs; stat_part against the
float64 sums of the kernel's own output over t < T (n u sum |v|, n = columns per wave x 98), rows of waves without a column
exact zeros.  "impulse" data: the reference is a shifted copy (a count for dW), everything else 0 to within the bound - and
the bound is 0 wherever no filter meets a non-zero column.  "range" data: a loud block beside a quiet one in the same
complex transform, loud channels beside quiet ones.

The module prints, per entry point, the number of checks, the worst error / bound, the worst RMS ratio against the float32
restatement, and the time spent per test function.

Measured on an MI355X (62 tests, 13 s; the slowest case, (2049, 8) with its 240 MB workspace, a few seconds): RMS ratios
0.96 - 1.14 for the forward, 0.96 - 1.14 for the data gradient, 0.93 - 1.25 for the weight gradient (1.25 at (2049, 8): 544
columns per chunk in ONE chain, where the restatement's matrix product sums them in blocks; 0.93 - 1.00 elsewhere); worst
error / bound 0.0070 (out), 0.0050 (dx), 0.021 (dW), 0.010 (the fused form from dp), 0.28 (the statistics against the
kernel's own output, at the DC tone where every term has one sign; <= 0.05 elsewhere).  A quiet block (1e-3) beside a loud
one (1e3) in the same column: RMS error / own RMS magnitude 0.15 - 0.16 for these kernels against 2.9e-7 for the direct one
(loud block: 2.0e-7 / 2.8e-7; quiet channels beside loud ones with filters inside a parity: 1.9e-7 / 2.0e-7) - the price of
two blocks per complex transform, within its bound.  No fault found: nothing in csrc/eegnet_conv64_fft.hip changed.

What the module notices, tried once with three deliberately wrong builds of the kernels: C64[15] wrong in its fourth digit
fails 46 of the 62 tests (every RMS criterion; the impulse cases stay within the worst-case bound), `t0 + j <= T` in the
statistics fails 36 (every T that is no multiple of 49), and a pack kernel that leaves the padding columns unwritten fails
60 - while test_conv64_fft, test_conv64_fft_gemm_gpu.py and test_conv64_fft_fused_gpu.py, which hand over a zeroed
workspace, pass all 54 of their cases with it (they do catch the other two, on 10 and 4 cases)."""
import time

import numpy as np
import pytest
import torch

from tests import conv64_fft_ref as R
from tests.kernel_check import GUARD, SENT, dev, ptr, same, sentinel_buf, take, within

pytestmark = pytest.mark.gpu

WORST, RMS, COUNT, SPENT = {}, {}, {}, {}
RMS_MARGIN = R.RMS_MARGIN      # another correct ordering of the same depth: the expected ratio is about 1 (reference module)
NONE = (0.0, 0, None, None)    # drop_p, seed, mask, seed_dev: no dropout


@pytest.fixture(scope="module")
def L():
    from eav_amd import _lib
    _lib.load()
    yield _lib
    print("\nentry point: checks, worst error / bound, worst RMS error / RMS error of the float32 restatement")
    for k in sorted(COUNT):
        print(f"  {k}: {COUNT[k]}, {WORST.get(k, 0.0):.5f}, {RMS.get(k, float('nan')):.3f}")
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


def t64(a):
    return a.double() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).double()


def check_bound(kernel, what, got, ref, bound):
    COUNT[kernel] = COUNT.get(kernel, 0) + 1
    ref = t64(ref)
    bound = t64(bound).expand(ref.shape)
    ratio = float(((got.double() - ref).abs() / bound.clamp_min(1e-300)).max())
    WORST[kernel] = max(WORST.get(kernel, 0.0), ratio)
    print(f"{kernel} {what}: worst error / bound {ratio:.5f}")
    within(got, ref, bound, f"{kernel} {what}")


def check_rms(kernel, what, got, ref, yard):
    e, ey = R.rms(got.double().numpy() - ref), R.rms(yard.astype(np.float64) - ref)
    ratio = e / ey if ey > 0 else (0.0 if e == 0 else float("inf"))
    RMS[kernel] = max(RMS.get(kernel, 0.0), ratio)
    print(f"{kernel} {what}: RMS error {e:.3e}, float32 restatement {ey:.3e}, ratio {ratio:.3f}")
    assert ratio <= RMS_MARGIN, f"{kernel} {what}: RMS error {e:.3e} is {ratio:.2f} x the float32 restatement's {ey:.3e}"


def assert_class(L, case):
    """the shape class from the two sizing exports: the columns the launchers will pad to, the waves of the pack grid"""
    B, T = case
    g = R.geometry(B, T)
    ws_n = L.plain("eav_conv64_fft_ws_floats", B, T)
    assert R.ncolp_of_ws(ws_n) == g["ncolp"] and ws_n == R.ws_floats(B, T)
    assert L.plain("eav_conv64_fft_nparts", B, T) == g["waves"]
    for k, v in R.COLUMNS.get(case, {}).items():
        assert g[k] == v, (k, g[k], v)
    return g, ws_n


def new_ws(n):
    """a sentinel-filled workspace with its guard band, filled on the device"""
    ws = torch.full((n + GUARD,), SENT, dtype=torch.int32, device="cuda").view(torch.float32)
    assert ws.data_ptr() % 16 == 0
    return ws


def guard_intact(ws, n, what):
    torch.cuda.synchronize()
    assert bool((ws[n:].view(torch.int32) == SENT).all()), f"{what}: written past eav_conv64_fft_ws_floats"


def bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def unchanged(d, h, what):
    h = h if isinstance(h, torch.Tensor) else torch.from_numpy(h)
    assert torch.equal(d.cpu(), h), f"{what}: an input was written"


def fft_call(L, ind, wd, ws, B, T, bwd, stats=False):
    """eav_conv64_fft_fwd on sentinel outputs -> (out, stat_part or None) on the host"""
    n, nparts = B * 64 * T, L.plain("eav_conv64_fft_nparts", B, T)
    out = sentinel_buf(n)
    part = sentinel_buf(nparts * 128) if stats else None
    L.call("eav_conv64_fft_fwd", ptr(ind), ptr(wd), ptr(out), ptr(part), ptr(ws), B, T, bwd, None)
    return take(out, n, (B, 64, T), "out"), (take(part, nparts * 128, (nparts, 128), "stat_part") if stats else None)


def wgrad_call(L, dud, ws, B, T):
    dW = sentinel_buf(65536)
    L.call("eav_conv64_fft_wgrad", ptr(dud), ptr(dW), ptr(ws), B, T, None)
    return take(dW, 65536, (64, 64, 16), "dW")


def bwd_call(L, dud, fz, drop, ws, B, T):
    """eav_conv64_fft_bwd from du, or (dud None) from fz = (dp, u, bn) on the device"""
    n = B * 64 * T
    dx, dW = sentinel_buf(n), sentinel_buf(65536)
    dp, u, bn = fz if dud is None else (None, None, None)
    m12 = None if bn is None else bn.data_ptr() + 4 * 4 * 64
    L.call("eav_conv64_fft_bwd", ptr(dud), ptr(dp), ptr(u), ptr(bn), m12, *drop, ptr(dx), ptr(dW), ptr(ws), B, T, None)
    return take(dx, n, (B, 64, T), "dx"), take(dW, 65536, (64, 64, 16), "dW")


def check_stats(case, g, out, part, ref, bound, k):
    B, T = case
    if g["ncol"] < g["waves"]:
        assert bool((part[g["ncol"]:].contiguous().view(torch.int32) == 0).all()), "rows of waves without a column are not exact zeros"
    st = part.double().sum(0)
    o = out.double().numpy()
    # (a) against float64 sums of the kernel's OWN output over exactly t < T: only the order of fp32 additions lies between
    check_bound(k, f"{case} sums vs own output", st, R.stat_ref(o), R.stat_bound(o, B, T))
    # (b) against the reference's sums: the forward bound of every element on top
    r, b = np.asarray(ref), np.asarray(bound)
    n = R.stat_chain(B, T)
    sb = 1.01 * R.U * np.concatenate([n * (np.abs(r) + b).sum((0, 2)), (n + 1) * ((np.abs(r) + b) ** 2).sum((0, 2))])
    sb += np.concatenate([b.sum((0, 2)), (2 * np.abs(r) * b + b * b).sum((0, 2))])
    check_bound(k, f"{case} sums vs reference", st, R.stat_ref(r), sb)


def sequence(L, case, mode, arg=None, rms=False, fused_dp=True):
    """the calls of one step in the model's order, every bit-equality among them, every result against float64"""
    B, T = case
    g, ws_n = assert_class(L, case)
    off = R.ws_offsets(B, T)
    x, w, du = R.inputs(B, T, mode, arg)
    ref, bound = R.refs(B, T, mode, arg), R.bounds(B, T, mode, arg)
    yard = R.yardsticks(B, T, mode, arg) if rms else None
    tag = f"{case} {mode}" + ("" if arg is None else f" {arg}")
    xd, wd, dud = dev(x), dev(w), dev(du)
    ws = new_ws(ws_n)

    out, part = fft_call(L, xd, wd, ws, B, T, 0, True)
    guard_intact(ws, ws_n, "forward")
    check_bound("fft_fwd", f"{tag} out", out, ref[0], bound[0])
    check_stats(case, g, out, part, ref[0], bound[0], "fft_fwd_stats")
    if rms:
        check_rms("fft_fwd", f"{tag} out", out, ref[0], yard[0])
    out2, _ = fft_call(L, xd, wd, ws, B, T, 0, False)
    same(out2, out, f"{tag} out without stat_part")
    zf, tables = ws[off["Zf"]:off["Zb"]].clone(), ws[:off["Zf"]].clone()
    assert not bool((zf.view(torch.int32) == SENT).any()), "input spectra: a column was never written"
    if g["ncol"] < g["ncolp"]:
        pad = zf.view(64, g["ncolp"], 128)[:, g["ncol"]:]
        assert bool((pad.contiguous().view(torch.int32) == 0).all()), "padding columns of the input spectra are not zeros"

    dx, _ = fft_call(L, dud, wd, ws, B, T, 2)
    check_bound("fft_dgrad", f"{tag} dx", dx, ref[1], bound[1])
    if rms:
        check_rms("fft_dgrad", f"{tag} dx", dx, ref[1], yard[1])
    ws1 = new_ws(ws_n)
    dx1, _ = fft_call(L, dud, wd, ws1, B, T, 1)
    guard_intact(ws1, ws_n, "bwd = 1")
    same(dx1, dx, f"{tag} dx: bwd = 1 on a fresh workspace against bwd = 2 on the forward's")
    assert bits_equal(ws1[off["BmB"]:off["Zf"]], ws[off["BmB"]:off["Zf"]]), "data-gradient filter spectra"
    assert bool((ws1[:off["BmB"]].view(torch.int32) == SENT).all()), "bwd = 1 wrote the forward's table"
    del ws1

    dW = wgrad_call(L, dud, ws, B, T)
    same(wgrad_call(L, dud, ws, B, T), dW, f"{tag} dW of a second call")
    check_bound("fft_wgrad", f"{tag} dW", dW, ref[2], bound[2])
    if rms:
        check_rms("fft_wgrad", f"{tag} dW", dW, ref[2], yard[2])

    dxb, dWb = bwd_call(L, dud, None, NONE, ws, B, T)
    COUNT["fft_bwd_du"] = COUNT.get("fft_bwd_du", 0) + 1
    same(dxb, dx, f"{tag} dx of the fused backward from du")
    same(dWb, dW, f"{tag} dW of the fused backward from du")
    guard_intact(ws, ws_n, "backward")
    assert bits_equal(ws[off["Zf"]:off["Zb"]], zf), "the forward's input spectra did not survive the backward calls"
    assert bits_equal(ws[:off["Zf"]], tables), "the filter spectra did not survive the backward calls"

    if fused_dp and T >= 8:
        dp, u, bn, mask = R.fused_inputs(B, T)
        fz = (dev(dp), dev(u), dev(bn))
        maskd = dev(mask)
        for name, drop_p, drop in (("none", 0.0, NONE), ("mask", 0.5, (0.5, 0, ptr(maskd), None))):
            r = R.du_ref(dp, u, bn, mask, drop_p)
            d64, e_du = r["du"].numpy(), r["e_du"].numpy()
            dxf, dWf = bwd_call(L, None, fz, drop, ws, B, T)
            check_bound("fft_bwd_dp", f"{tag} dropout {name} dx", dxf, R.dgrad_ref(d64, w), R.dgrad_bound(d64, w, e_du))
            check_bound("fft_bwd_dp", f"{tag} dropout {name} dW", dWf, R.wgrad_ref(d64, x), R.wgrad_bound(x, d64, e_du))
        assert bits_equal(ws[off["Zf"]:off["Zb"]], zf), "the forward's input spectra did not survive the fused backward"
        guard_intact(ws, ws_n, "fused backward")
        for d, h, what in zip(fz + (maskd,), (dp, u, bn, mask), ("dp", "u", "bn", "mask")):
            unchanged(d, h, what)
    for d, h, what in ((xd, x, "x"), (wd, w, "w"), (dud, du, "du")):
        unchanged(d, h, what)
    return out, dx, dW


# ------------------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("case", R.ALL, ids=str)
def test_normal(L, case):
    sequence(L, case, "normal", rms=True)


@pytest.mark.parametrize("case", R.SMALL, ids=str)
def test_dc_offset(L, case):
    """normal + 3: what the model feeds - p2 is an ELU / AvgPool output and not zero-mean"""
    sequence(L, case, "dc", rms=True, fused_dp=False)


@pytest.mark.parametrize("m", R.TONE_BINS)
def test_pure_tones(L, m):
    """one real tone per case with channel-dependent amplitude and phase: DC, the first bin, both neighbours of the first
    twiddle row (7, 8, 9), the last bin below the mirror and the mirror"""
    sequence(L, R.TONE_CASE, "tone", m, rms=True, fused_dp=False)


@pytest.mark.parametrize("case", R.SMALL, ids=str)
def test_impulses_come_out_as_shifted_copies(L, case):
    """unit impulses at the block edges and at the samples whose halo crosses them, against single-tap filters at taps 0, 7,
    8, 15: out and dx are shifted copies, dW counts coincidences, everything else is 0 to within the bound"""
    B, T = case
    out, dx, dW = sequence(L, case, "impulse", fused_dp=False)
    ref, bound = R.refs(B, T, "impulse"), R.bounds(B, T, "impulse")
    for name, got, r, b in zip(("out", "dx", "dW"), (out, dx, dW), ref, bound):
        zeros = np.broadcast_to(b, r.shape) == 0
        assert not (r[zeros] != 0).any()
        assert bool((got.numpy()[zeros] == 0).all()), f"{name}: not exactly 0 where no filter meets a non-zero column"
        print(f"{case} {name}: {int((r != 0).sum())} non-zero reference values, {int(zeros.sum())} of {r.size} outputs with bound 0")


@pytest.mark.parametrize("kind", R.RANGE_KINDS)
@pytest.mark.parametrize("case", R.RANGE_CASES, ids=str)
def test_quiet_beside_loud(L, case, kind):
    """'blocks': block A at 1e3 beside block B at 1e-3 - they share one complex transform, and the quiet block keeps the
    loud one's absolute error (within the bound of the COLUMN's norm).  'channels': odd channels at 1e3, even ones at 1e-3,
    filters only between channels of the same parity.  The quiet part's error relative to its own magnitude is printed
    beside the direct kernel's (csrc/eegnet_conv64.hip), whose error scales with the samples under the filter: a recorded
    fact of the design, not an assertion."""
    B, T = case
    out, _, _ = sequence(L, case, "range", kind, fused_dp=False)
    x, w, _ = R.inputs(B, T, "range", kind)
    ref = R.refs(B, T, "range", kind)[0]
    n = B * 64 * T
    wd = dev(w)
    wTf, wTb, direct = sentinel_buf(65536), sentinel_buf(65536), sentinel_buf(n)
    L.call("eav_conv64_prep_weights", ptr(wd), ptr(wTf), ptr(wTb), None)
    L.call("eav_conv64_fwd", ptr(dev(x)), ptr(wTf), ptr(direct), None, B, T, 7, None)
    direct = take(direct, n, (B, 64, T), "out (direct)").double().numpy()
    quiet = np.zeros((B, 64, T), bool)
    if kind == "blocks":
        # outputs of block B more than 8 samples from a loud block: every sample under their filter is quiet
        t = np.arange(T)
        quiet[:, :, ((t // R.LV) % 2 == 1) & (t % R.LV >= 7) & (t % R.LV < R.LV - 8)] = True
    else:
        quiet[:, 0::2] = True
    for name, sel in (("quiet", quiet), ("loud", ~quiet)):
        if sel.any():
            own = R.rms(ref[sel])
            print(f"{case} {kind} {name}: RMS error / RMS magnitude: FFT kernel {R.rms(out.double().numpy()[sel] - ref[sel]) / own:.3e}, "
                  f"direct kernel {R.rms(direct[sel] - ref[sel]) / own:.3e}")


# ------------------------------------------------------------------------------------------------------ rejected arguments
def test_refusals_come_before_any_launch(L):
    B, T = 1, 7
    n = B * 64 * 8
    src = dev(torch.zeros(65536))                         # large enough for every role, should a refusal be missing
    ws_n = L.plain("eav_conv64_fft_ws_floats", B, 8)
    ws = new_ws(ws_n)
    outs = [sentinel_buf(n, guard=0), sentinel_buf(65536, guard=0), sentinel_buf(L.plain("eav_conv64_fft_nparts", B, 8) * 128, guard=0)]
    s, (a, b, c), w = ptr(src), [ptr(o) for o in outs], ptr(ws)
    mask = ptr(dev(torch.ones(n, dtype=torch.uint8)))
    bad = [("< the pooling window", ("eav_conv64_fft_bwd", None, s, s, s, s, 0.0, 0, None, None, a, b, w, B, 7, None)),
           ("bwd must be", ("eav_conv64_fft_fwd", s, s, a, c, w, B, 8, 3, None)),
           ("bwd must be", ("eav_conv64_fft_fwd", s, s, a, c, w, B, 8, -1, None)),
           ("dropout", ("eav_conv64_fft_bwd", None, s, s, s, s, 1.0, 0, mask, None, a, b, w, B, 8, None)),
           ("dropout", ("eav_conv64_fft_bwd", s, None, None, None, None, -1.0, 0, None, None, a, b, w, B, 8, None)),
           ("16-byte aligned", ("eav_conv64_fft_fwd", s, s, a, c, w + 4, B, 8, 0, None)),
           ("16-byte aligned", ("eav_conv64_fft_bwd", s, None, None, None, None, 0.0, 0, None, None, a, b, w + 8, B, 8, None)),
           ("neither du nor", ("eav_conv64_fft_bwd", None, s, None, s, s, 0.0, 0, None, None, a, b, w, B, 8, None))]
    for text, (name, *args) in bad:
        with pytest.raises(L.EavError, match=text):
            L.call(name, *args)
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o.view(torch.int32) == SENT).all()), "a rejected call wrote to its output"
    assert bool((ws.view(torch.int32) == SENT).all()), "a rejected call wrote to the workspace"
    # T = 8 is the smallest the fused form accepts (test_normal runs it); from du every T is accepted, T = 7 included
    assert (2, 7) in R.SMALL and (2, 8) in R.SMALL
