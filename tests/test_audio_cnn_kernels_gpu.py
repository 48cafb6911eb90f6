"""Per-kernel parity of the audio CNN conv kernels (csrc/audio_cnn.hip, through the C ABI) against the float64 references
of tests/audio_conv_ref.py, written from the contracts in include/eav_hip.h.

Every case runs in two data modes.  "exact": small integers, quarter-integer weights and biases and dropout scales 2 or 4,
so that every fp32 product and partial sum is exact in any order (asserted from the shapes); the kernel must then equal
the reference bit for bit, argmax included.  "rounded": synth normal / uniform data and p = 0.1, held to the rigorous
bound gamma_n * sum|terms| (plus the epilogue's roundings), n the number of terms of that output's sum.

Every output is filled with a NaN sentinel (payload 0x7fc0dead; 0xFF for the argmax) and carries a guard band past its
end: everything the contract says is written must be overwritten, the guard band must be untouched."""
import numpy as np
import pytest
import torch

from eav_amd import synth
from tests import kernel_check as kc
from tests.audio_conv_ref import dgrad_ref, f32_scale, fwd_ref, gamma, wgrad_ref
from tests.kernel_check import assert_exact, dev, ints, keep_mask, normal, ptr, same, seed_of, take, within

pytestmark = pytest.mark.gpu

GUARD = 128 * 32 * 8        # guard band (elements) past every output: one conv tile of the dense pool-scatter output
EXACT_P = {0: 0.5, 1: 0.75}


@pytest.fixture(scope="module", autouse=True)
def L():
    from eav_amd import _lib
    _lib.load()
    return _lib


def sentinel_buf(n, dtype=torch.float32):
    return kc.sentinel_buf(n, dtype, GUARD)


# ------------------------------------------------------------------------------------------------------------- forward
def launch_fwd(x, w, b, Lout, pool, p=0.0, mask=None, seed=0, seed_dev=None, what="fwd"):
    B, C, Lin = x.shape
    N = w.shape[0]
    L_ = Lout // 8 if pool else Lout
    n = B * N * L_
    out = sentinel_buf(n)
    idx = sentinel_buf(n, torch.uint8) if pool else None
    xd, wd, bd = dev(x), dev(w), dev(b)
    md = dev(mask) if mask is not None else None
    from eav_amd import _lib
    _lib.call("eav_audio_conv5_fwd", xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), ptr(idx), B, C, N,
              Lin, Lout, pool, p, seed, ptr(md), ptr(seed_dev), None)
    o = take(out, n, (B, N, L_), what)
    return (o, take(idx, n, (B, N, L_), what + " idx")) if pool else o


def fwd_data(mode, B, C, N, Lin, seed, drop):
    """(x, w, b, p, mask) for one forward case.  Exact data with N >= 5 channels: channel 0 is zero everywhere (all-zero
    ReLU windows), channel 1 the constant 3/4 (ties on a live maximum), and the mask drops position 0 of that channel's
    first window and keeps position 1, so that its argmax moves from 0 to 1."""
    if mode == "exact":
        x = ints(seed, (B, C, Lin), -3, 3)
        w = ints(seed + 1, (N, C, 5), -3, 3) / 4
        b = ints(seed + 2, (N,), -8, 8) / 4
        p = EXACT_P[seed % 2] if drop else 0.0
        assert_exact((C * 5 * 3 * 0.75 + 2) * 4, 0.25, "fwd")
        if N >= 5:
            w[:2] = 0.0
            b[0], b[1] = 0.0, 0.75
    else:
        x = normal(seed, (B, C, Lin))
        w = normal(seed + 1, (N, C, 5), 0.3)
        b = torch.from_numpy(synth.uniform(seed + 2, (N,), -0.5, 0.5))
        p = 0.1 if drop else 0.0
    mask = keep_mask(seed + 3, (B, N, Lin), p) if drop else None
    if drop and mode == "exact" and N >= 5 and Lin >= 2:
        mask[0, 1, 0], mask[0, 1, 1] = 0, 1
    return x, w, b, p, mask


def fwd_tol(x, w, b, p):
    """gamma_{C*5+1} * sum|terms| for the conv and its bias, plus the dropout scale's rounding."""
    n = x.shape[1] * 5 + 1
    s = f32_scale(p) if p > 0 else 1.0
    return gamma(n + 1) * s * fwd_ref(x.abs(), w.abs(), b.abs(), x.shape[2])


# (C, N, L, B): every value of C in {1, 16, 48, 256}, N in {1, 5, 127, 128, 129, 300}, L in {1, 2, 31, 32, 33, 180, 183}
# and B in {1, 3}; C = 1 (conv5_kernel<1,fwd,relu>) and C % 16 == 0 (<16,fwd,relu>) both at ragged N and L
FWD_CASES = [(1, 1, 1, 1), (1, 129, 33, 3), (1, 300, 183, 1), (1, 127, 2, 3), (16, 5, 2, 3), (16, 127, 31, 1),
             (16, 129, 33, 3), (48, 128, 32, 3), (48, 300, 180, 1), (256, 5, 183, 3), (256, 128, 180, 1),
             (256, 1, 1, 3)]


@pytest.mark.parametrize("mode", ["exact", "rounded"])
@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "mask"])
@pytest.mark.parametrize("C,N,L_,B", FWD_CASES, ids=[f"C{c}-N{n}-L{l}-B{b}" for c, n, l, b in FWD_CASES])
def test_fwd_relu(C, N, L_, B, drop, mode):
    seed = seed_of("fwd", C, N, L_, B, drop, mode)
    x, w, b, p, mask = fwd_data(mode, B, C, N, L_, seed, drop)
    got = launch_fwd(x, w, b, L_, 0, p, mask)
    ref = fwd_ref(x, w, b, L_, 0, mask, p)
    if mode == "exact":
        same(got, ref, "out")
    else:
        within(got, ref, fwd_tol(x, w, b, p), "out")


@pytest.mark.parametrize("C", [1, 16])
def test_fwd_generated_dropout_seed_dev(C):
    """(seed, *seed_dev = k) draws the mask of (seed + 2k, NULL); every element is either dropped or the kept value
    times 2 exactly; about half the live elements survive; another seed draws another mask."""
    B, N, L_, seed, k = 3, 129, 33, 0x5EED, 3
    x, w, b, _, _ = fwd_data("exact", B, C, N, L_, seed_of("gen", C), False)
    cnt = dev(torch.tensor([k], dtype=torch.int64))
    a = launch_fwd(x, w, b, L_, 0, 0.5, None, seed, cnt)
    c = launch_fwd(x, w, b, L_, 0, 0.5, None, seed + 2 * k, None)
    assert torch.equal(a.view(torch.int32), c.view(torch.int32))
    other = launch_fwd(x, w, b, L_, 0, 0.5, None, seed, None)
    ref = fwd_ref(x, w, b, L_)
    live = ref > 0
    assert ((a.double() == 0) | (a.double() == 2 * ref)).all()
    kept = int((a[live] > 0).sum()) / int(live.sum())
    assert abs(kept - 0.5) < 5 * (0.25 / int(live.sum())) ** 0.5, kept
    assert not torch.equal(a > 0, other > 0)


# ------------------------------------------------------------------------------------------------------ forward, pool
# (C, N, Lout, Lin, B): Lout in {8, 40, 176}, Lin from Lout to Lout + 7 (all eight at 176); conv5_kernel<16,fwd,pool>
POOL_CASES = ([(16, 5, 8, 8, 1), (256, 200, 8, 15, 3), (16, 128, 40, 40, 3), (256, 5, 40, 43, 1), (16, 200, 40, 47, 2)]
              + [((16, 256)[j % 2], (5, 128, 200)[j % 3], 176, 176 + j, 1 + j % 3) for j in range(8)])


def pool_tol(x, w, b, p, Lout):
    """The bound of every pre-pool value, and its maximum over each window."""
    t = fwd_tol(x, w, b, p)[..., :Lout]
    return t, t.unflatten(2, (Lout // 8, 8)).amax(3)


def check_pool(x, w, b, Lout, p, mask, mode, what=""):
    got, gidx = launch_fwd(x, w, b, Lout, 1, p, mask, what="pool" + what)
    ref, ridx = fwd_ref(x, w, b, Lout, 1, mask, p)
    if mode == "exact":
        same(got, ref, "pooled" + what)
        assert torch.equal(gidx, ridx), f"idx{what}: {int((gidx != ridx).sum())} windows differ"
    else:
        t, tw = pool_tol(x, w, b, p, Lout)
        within(got, ref, tw, "pooled" + what)
        # the argmax is decided only where the top two values of the window are apart by more than twice the bound
        y = fwd_ref(x, w, b, Lout, 0, mask, p)[..., :Lout].unflatten(2, (Lout // 8, 8))
        top = y.topk(2, 3).values
        sure = (top[..., 0] - top[..., 1]) > 2 * tw
        assert sure.float().mean() > 0.5, "too few decided windows"
        assert torch.equal(gidx[sure], ridx[sure]), f"idx{what}: {int((gidx[sure] != ridx[sure]).sum())} windows differ"
    return ref, ridx


@pytest.mark.parametrize("mode", ["exact", "rounded"])
@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "mask"])
@pytest.mark.parametrize("C,N,Lout,Lin,B", POOL_CASES,
                         ids=[f"C{c}-N{n}-Lout{lo}-Lin{li}-B{b}" for c, n, lo, li, b in POOL_CASES])
def test_fwd_pool(C, N, Lout, Lin, B, drop, mode):
    seed = seed_of("pool", C, N, Lout, Lin, B, drop, mode)
    x, w, b, p, mask = fwd_data(mode, B, C, N, Lin, seed, drop)
    ref, ridx = check_pool(x, w, b, Lout, p, mask, mode)
    if mode == "exact":
        # the planted ties (fwd_data): all-zero windows record 0, the constant channel its first kept position
        assert (ref[:, 0] == 0).all() and (ridx[:, 0] == 0).all() and (drop or (ref[:, 1] > 0).all())
        assert ridx[0, 1, 0] == (1 if drop else 0)


def test_fwd_pool_constant_input_ties_on_all_eight():
    """A constant input: every interior window holds eight equal values, and the argmax is 0 there."""
    B, C, N, Lout = 2, 16, 128, 40
    x = torch.full((B, C, Lout), 2.0)
    w = ints(seed_of("const"), (N, C, 5), -3, 3) / 4
    w[:64] = w[:64].abs()                             # half the channels positive: ties on a live maximum
    b = ints(seed_of("const") + 1, (N,), -8, 8) / 4
    win = fwd_ref(x, w, b, Lout)[..., :Lout].unflatten(2, (Lout // 8, 8))
    assert (win[:, :64, 1:4] > 0).all() and (win[:, :, 1:4] == win[:, :, 1:4, :1]).all()
    _, ridx = check_pool(x, w, b, Lout, 0.0, None, "exact")
    assert (ridx[:, :, 1:4] == 0).all()


@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "mask"])
def test_fwd_pool_nan_records_the_last_nan(drop):
    """A NaN at input position t reaches conv outputs t-2..t+2.  Sample 0, t = 1: positions 0-3 of window 0 (first wave
    half only).  Sample 1, t = 6: positions 4-7 of window 0 (second half) and position 0 of window 1, then finite values
    in both halves.  Sample 2, t = 10: positions 0-4 of window 1, across both halves.  The pooled value is NaN and idx is
    torch's: the last NaN of the window."""
    B, C, N, Lout, Lin = 3, 16, 128, 40, 43
    x, w, b, p, mask = fwd_data("exact", B, C, N, Lin, seed_of("nan", drop), drop)
    for s, t in enumerate((1, 6, 10)):
        x[s, 5, t] = float("nan")
    ref, ridx = check_pool(x, w, b, Lout, p, mask, "exact")
    want = {0: {0: 3}, 1: {0: 7, 1: 0}, 2: {1: 4}}
    for s in range(B):
        for q in range(Lout // 8):
            if q in want[s]:
                assert torch.isnan(ref[s, :, q]).all() and (ridx[s, :, q] == want[s][q]).all(), (s, q)
            else:
                assert not torch.isnan(ref[s, :, q]).any(), (s, q)


# ------------------------------------------------------------------------------------------------------- data gradient
def launch_dgrad(g, w, Lout, gate_in=None, gscale_in=1.0, mode=0, aux=None, idx=None, gscale_out=1.0, what="dgrad"):
    B, C, Lin = g.shape
    N = w.shape[1]
    L_ = 8 * Lout if mode == 1 else Lout
    n = B * N * L_
    out = sentinel_buf(n)
    gd, wd = dev(g), dev(w)
    gi, ad, idd = (dev(t) if t is not None else None for t in (gate_in, aux, idx))
    from eav_amd import _lib
    _lib.call("eav_audio_conv5_dgrad", gd.data_ptr(), ptr(gi), gscale_in, wd.data_ptr(), out.data_ptr(), ptr(ad),
              ptr(idd), gscale_out, B, C, N, Lin, Lout, mode, None)
    return take(out, n, (B, N, L_), what)


def gate_data(seed, shape):
    """A ReLU-output-like gate: positives, zeros, -0.0 and NaN."""
    gt = ints(seed, shape, -1, 2)
    flat = gt.view(-1)
    flat[::7] = -0.0
    flat[3::11] = float("nan")
    return gt


def dgrad_data(mode, B, C, N, Lin, seed):
    if mode == "exact":
        return ints(seed, (B, C, Lin), -3, 3), ints(seed + 1, (C, N, 5), -3, 3) / 4
    return normal(seed, (B, C, Lin)), normal(seed + 1, (C, N, 5), 0.3)


# (C, N, Lin, Lout, B); (176, 183) is conv2's data gradient as the model calls it; conv5_kernel<16,trans,gate>
DGRAD0_CASES = [(16, 1, 1, 1, 1), (48, 129, 22, 22, 3), (128, 256, 33, 33, 2), (128, 256, 176, 183, 2),
                (16, 128, 183, 183, 1), (48, 1, 176, 183, 1)]


@pytest.mark.parametrize("mode", ["exact", "rounded"])
@pytest.mark.parametrize("use_aux", [False, True], ids=["noaux", "aux"])
@pytest.mark.parametrize("use_gate", [False, True], ids=["nogate", "gate"])
@pytest.mark.parametrize("C,N,Lin,Lout,B", DGRAD0_CASES,
                         ids=[f"C{c}-N{n}-Lin{li}-Lout{lo}-B{b}" for c, n, li, lo, b in DGRAD0_CASES])
def test_dgrad_relu_gate(C, N, Lin, Lout, B, use_gate, use_aux, mode):
    seed = seed_of("dgrad0", C, N, Lin, Lout, B, use_gate, use_aux, mode)
    g, w = dgrad_data(mode, B, C, N, Lin, seed)
    gate = gate_data(seed + 2, (B, C, Lin)) if use_gate else None
    aux = gate_data(seed + 3, (B, N, Lout)) if use_aux else None
    got = launch_dgrad(g, w, Lout, gate, 2.0, 0, aux)
    ref = dgrad_ref(g, w, Lout, gate, 2.0, 0, aux)
    if mode == "exact":
        assert_exact(C * 5 * 6 * 0.75, 0.25, "dgrad")
        same(got, ref, "din")
    else:
        tol = gamma(C * 5 + 1) * dgrad_ref(g.abs(), w.abs(), Lout, gate, 2.0)
        within(got, ref, tol, "din")


# (C, N, Lout, B): the pool backward scatter into the dense pre-pool gradient; conv5_kernel<16,trans,scatter>
DGRAD1_CASES = [(16, 5, 1, 3), (128, 128, 22, 2), (48, 130, 5, 1), (16, 130, 22, 2), (128, 5, 5, 3)]


@pytest.mark.parametrize("mode", ["exact", "rounded"])
@pytest.mark.parametrize("gscale_out", [2.0, f32_scale(0.1)], ids=["gs2", "gs1/0.9"])
@pytest.mark.parametrize("C,N,Lout,B", DGRAD1_CASES, ids=[f"C{c}-N{n}-Lout{lo}-B{b}" for c, n, lo, b in DGRAD1_CASES])
def test_dgrad_pool_scatter(C, N, Lout, B, gscale_out, mode):
    seed = seed_of("dgrad1", C, N, Lout, B, gscale_out, mode)
    g, w = dgrad_data(mode, B, C, N, Lout, seed)
    idx = torch.from_numpy((synth.splitmix64(seed + 2, B * N * Lout) % np.uint64(8)).astype(np.uint8)
                           .reshape(B, N, Lout))
    aux = ints(seed + 3, (B, N, Lout), -1, 2)
    aux.view(-1)[::9] = float("nan")
    aux.view(-1)[4::13] = -0.0
    if B * N * Lout >= 8:
        idx.view(-1)[:8] = torch.arange(8, dtype=torch.uint8)     # every offset at least once
    got = launch_dgrad(g, w, Lout, None, 1.0, 1, aux, idx, gscale_out)
    ref = dgrad_ref(g, w, Lout, mode=1, aux=aux, idx=idx, gscale_out=gscale_out)
    assert (ref != 0).any()
    if mode == "exact":
        assert_exact(C * 5 * 3 * 0.75, 0.25, "dgrad scatter")
        # the conv sum is exact; the kernel rounds its product with gscale_out once, as .float() does
        same(got, ref.float(), "din")
    else:
        tol = gamma(C * 5 + 2) * gscale_out * dgrad_ref(g.abs(), w.abs(), Lout, mode=1, aux=torch.ones_like(aux),
                                                         idx=idx)
        within(got, ref, tol, "din")


# ----------------------------------------------------------------------------------------------------- weight gradient
def nparts_regime(B, Cact, M, Lout):
    tiles = -(-Cact * 5 // 64) * -(-M // 64)
    nq = B * -(-Lout // 32)
    return "clamped" if -(-768 // tiles) >= nq else "split"


def launch_wgrad(dout, act, gate=None, gscale=1.0, what="wgrad"):
    B, M, Lout = dout.shape
    _, Cact, Lact = act.shape
    from eav_amd import _lib
    nparts = _lib.plain("eav_audio_wgrad_nparts", B, Cact, M, Lout)
    regime = nparts_regime(B, Cact, M, Lout)
    nq = B * -(-Lout // 32)
    assert nparts == (nq if regime == "clamped" else -(-768 // (-(-Cact * 5 // 64) * -(-M // 64))))
    size = M * Cact * 5 + M
    part = sentinel_buf(nparts * size)
    out = sentinel_buf(size)
    dd, ad = dev(dout), dev(act)
    gd = dev(gate) if gate is not None else None
    _lib.call("eav_audio_conv5_wgrad", dd.data_ptr(), ptr(gd), gscale, ad.data_ptr(), part.data_ptr(), B, Cact, M,
              Lact, Lout, nparts, None)
    take(part, nparts * size, (nparts, size), what + " partials")
    _lib.call("eav_reduce_partials", part.data_ptr(), nparts, size, size, 1.0, out.data_ptr(), None)
    o = take(out, size, (size,), what)
    return o[:M * Cact * 5].view(M, Cact, 5), o[M * Cact * 5:], nparts


# (Cact, M, Lact, Lout, B): Cact = 13 is 65 columns (a one-column second tile, 13 staged channels in the first); the
# id records the nparts regime: "clamped" (one chunk per part) or "split" (cdiv(768, tiles) parts over more chunks)
WGRAD_CASES = [(1, 256, 180, 180, 64), (13, 65, 33, 33, 2), (16, 1, 1, 1, 1), (128, 128, 22, 22, 300),
               (256, 128, 183, 176, 2), (256, 64, 176, 183, 64), (13, 128, 180, 180, 300), (1, 65, 22, 22, 1)]


@pytest.mark.parametrize("mode", ["exact", "rounded"])
@pytest.mark.parametrize("use_gate", [False, True], ids=["nogate", "gate"])
@pytest.mark.parametrize("Cact,M,Lact,Lout,B", WGRAD_CASES,
                         ids=[f"Cact{c}-M{m}-Lact{la}-Lout{lo}-B{b}-{nparts_regime(b, c, m, lo)}"
                              for c, m, la, lo, b in WGRAD_CASES])
def test_wgrad(Cact, M, Lact, Lout, B, use_gate, mode):
    seed = seed_of("wgrad", Cact, M, Lact, Lout, B, use_gate, mode)
    if mode == "exact":
        dout, act = ints(seed, (B, M, Lout), -3, 3), ints(seed + 1, (B, Cact, Lact), 0, 3)
        assert_exact(B * Lout * 6 * 3, 1.0, "wgrad")
    else:
        dout, act = normal(seed, (B, M, Lout)), normal(seed + 1, (B, Cact, Lact))
    gate = gate_data(seed + 2, (B, M, Lout)) if use_gate else None
    dw, db, nparts = launch_wgrad(dout, act, gate, 2.0)
    rw, rb = wgrad_ref(dout, act, gate, 2.0)
    if mode == "exact":
        same(dw, rw, "dW")
        same(db, rb, "db")
    else:
        n = B * Lout + 1
        aw, ab = wgrad_ref(dout.abs(), act.abs(), gate, 2.0)
        within(dw, rw, gamma(n) * aw, "dW")
        within(db, rb, gamma(n) * ab, "db")


# ---------------------------------------------------------------------------------------------------- reproducibility
def test_larger_cases_are_bit_reproducible():
    """One larger case per entry point, twice: bit-identical outputs (no float atomics, fixed summation orders)."""
    B, T = 8, 183
    x, w, b, p, mask = fwd_data("rounded", B, 256, 128, T, seed_of("rep"), True)
    a1, i1 = launch_fwd(x, w, b, 176, 1, p, mask)
    a2, i2 = launch_fwd(x, w, b, 176, 1, p, mask)
    assert torch.equal(a1.view(torch.int32), a2.view(torch.int32)) and torch.equal(i1, i2)
    g, wt = dgrad_data("rounded", B, 128, 256, 176, seed_of("rep") + 7)
    aux = gate_data(seed_of("rep") + 8, (B, 256, T))
    d1, d2 = (launch_dgrad(g, wt, T, None, 1.0, 0, aux) for _ in range(2))
    assert torch.equal(d1.view(torch.int32), d2.view(torch.int32))
    dout, act = normal(seed_of("rep") + 9, (64, 128, 176)), normal(seed_of("rep") + 10, (64, 256, T))
    (w1, b1, _), (w2, b2, _) = (launch_wgrad(dout, act) for _ in range(2))
    assert torch.equal(w1.view(torch.int32), w2.view(torch.int32)) and torch.equal(b1.view(torch.int32),
                                                                                   b2.view(torch.int32))
