"""Per-kernel parity of the canonical-EEGNet kernels (csrc/eegnet_canon.hip, through the C ABI) against the float64
references of tests/eegnet_canon_ref.py, written from the contracts in include/eav_hip.h.

Data modes.  "exact": small integers and quarter-integer weights, so that every fp32 product and partial sum is exact in
any order; this is asserted (assert_exact) from the sum of the absolute values of the terms of the largest output, which
bounds every partial sum of every summation order, and the kernel must then equal the reference bit for bit.  "sparse":
the same demand on data thin enough (inputs in {-1, 0, 1}, a few +-1 taps per filter) that the block sums of SQUARES
are exact as well; in "exact" mode those sums are too large for that and are held to the rounded bound instead.
"rounded": synth normal data, every element held to gamma(n + c) * magnitude, n the number of terms of that output's
sum, c the extra fp32 roundings per term (derived beside each check), the magnitude the same sum over absolute values.

Every output buffer, partial buffers included, is filled with a NaN sentinel and carries a guard band: all the contract
says is written must be written, the band must be untouched.  Partial rows are summed on the host in float64 (exact for
exact rows) and compared with the reference total; where the header fixes the row layout they are compared row by row.

The ELU of the spatial kernels is kept exact by drawing the BatchNorm outputs from {1, 2, 3} + {0} + {-18, -40}: elu_f is
the identity above 0, 0 at 0 and exactly -1 below -17.5.  Rounded mode covers (-17.5, 0) and allows 1 ulp of ELU(o)
(eav_common.h documents 0.97 ulp against float64) on top of the rounding carried in by o."""
import numpy as np
import pytest
import torch

from eav_amd import synth
from tests import eegnet_canon_ref as R
from tests.audio_conv_ref import gamma
from tests.kernel_check import SENT, assert_exact, dev, ints, normal, same, seed_of, sentinel_buf, take, within

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def L():
    from eav_amd import _lib
    _lib.load()
    return _lib


def call(name, *args):
    from eav_amd import _lib
    _lib.call(name, *[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], None)


def plain(name, *args):
    from eav_amd import _lib
    return _lib.plain(name, *args)


def cdiv(a, b):
    return -(-a // b)


def sparse_pm1(seed, rows, cols, nnz):
    """[rows, cols] with at most nnz entries of +-1 per row, zero elsewhere."""
    pos = (synth.splitmix64(seed, rows * nnz) % np.uint64(cols)).astype(np.int64).reshape(rows, nnz)
    sgn = (synth.splitmix64(seed + 1, rows * nnz) % np.uint64(2)).astype(np.float32).reshape(rows, nnz) * 2 - 1
    w = np.zeros((rows, cols), np.float32)
    np.put_along_axis(w, pos, sgn, 1)
    return torch.from_numpy(w)


def pick(seed, shape, values):
    """float32 values drawn uniformly from a list."""
    v = np.asarray(values, np.float32)
    n = int(np.prod(shape))
    return torch.from_numpy(v[(synth.splitmix64(seed, n) % np.uint64(len(v))).astype(np.int64)].reshape(shape))


def exact_or_bound(got, ref, absterms, quantum, tol, what):
    """Bit equality where the sum of the absolute terms proves every partial sum exact, the rounded bound otherwise."""
    if float(absterms.max()) / quantum < 2.0 ** 24:
        same(got, ref, what)
    else:
        within(got, ref, tol, what)


def sq_tol(mag, e, dims, n_sum):
    """Bound of a fp32 sum of squares of values known to |err| <= e with |value| <= mag: the squares' own error
    (2 |y| + e) e plus one rounding each, then gamma(n_sum) of the sum."""
    return ((2 * mag + e) * e).sum(dims) + gamma(n_sum + 1) * ((mag + e) ** 2).sum(dims)


# ===================================================================================================== eav_tconv_fwd
def tconv_path(F1, K):
    if F1 == 8 and K <= 300:
        return "mfma-fir"
    return f"NG{1 if F1 <= 8 else 2}-KM{512 if K <= 512 else 1024}"


# (B, C, S, F1, K): the four direct instantiations, the MFMA hand-over, both tap parities and K % 4 != 0, one S < K
TCONV_FWD = [(1, 1, 1, 1, 1), (2, 3, 33, 3, 2), (1, 2, 1023, 8, 301), (1, 1, 1024, 9, 3), (2, 2, 1025, 16, 64),
             (1, 1, 2049, 1, 512), (1, 2, 33, 9, 513), (1, 1, 1025, 16, 1024), (1, 1, 1024, 3, 1024),
             (2, 1, 1023, 9, 512), (1, 2, 2049, 3, 513), (2, 3, 1025, 8, 64)]


def tconv_data(mode, seed, B, C, S, F1, K):
    if mode == "exact":
        return ints(seed, (B, C, S), -3, 3), ints(seed + 1, (F1, K), -3, 3) / 4
    if mode == "sparse":
        return ints(seed, (B, C, S), -1, 1), sparse_pm1(seed + 1, F1, K, 4)
    return normal(seed, (B, C, S)), normal(seed + 1, (F1, K), 0.3)


@pytest.mark.parametrize("mode", ["exact", "sparse", "rounded"])
@pytest.mark.parametrize("B,C,S,F1,K", TCONV_FWD,
                         ids=[f"B{b}-C{c}-S{s}-F{f}-K{k}-{tconv_path(f, k)}" for b, c, s, f, k in TCONV_FWD])
def test_tconv_fwd(B, C, S, F1, K, mode):
    x, w = tconv_data(mode, seed_of("tconv_fwd", B, C, S, F1, K, mode), B, C, S, F1, K)
    direct = tconv_path(F1, K) != "mfma-fir"
    nparts = plain("eav_tconv_fwd_nparts", B, C, S, F1, K)
    if direct:
        assert nparts == B * C * cdiv(S, 1024)
    else:
        assert nparts == plain("eav_eegnet_fir_fwd_nparts", B, C, S)
    n = B * F1 * C * S
    y = sentinel_buf(n)
    part = sentinel_buf(nparts * 2 * F1)
    call("eav_tconv_fwd", dev(x), dev(w), y, part, B, C, S, F1, K)
    y = take(y, n, (B, F1, C, S), "y1")
    part = take(part, nparts * 2 * F1, (nparts, 2 * F1), "stat_part").double()
    ref, mag = R.tconv_fwd_ref(x, w), R.tconv_fwd_ref(x.abs(), w.abs())
    # K products accumulated by fma in one chain (the kernel pads the taps to a multiple of 4 with zeros: K + 3)
    e = gamma(K + 3) * mag
    if mode == "rounded":
        within(y, ref, e, "y1")
    else:
        assert_exact(float(mag.max()), 1.0 / 4, "y1")
        same(y, ref, "y1")
    # statistics: a row sums at most min(S, 1024) values per filter (direct) - the total count bounds any layout
    nrow = min(S, 1024) if direct else B * C * S
    if direct:      # row (b, c, tile), as the header lays them out
        tiles = [(t0, min(t0 + 1024, S)) for t0 in range(0, S, 1024)]
        rs = torch.stack([ref[..., a:b].sum(3) for a, b in tiles], 3).permute(0, 2, 3, 1).reshape(nparts, F1)
        rq = torch.stack([(ref[..., a:b] ** 2).sum(3) for a, b in tiles], 3).permute(0, 2, 3, 1).reshape(nparts, F1)
        ms = torch.stack([mag[..., a:b].sum(3) for a, b in tiles], 3).permute(0, 2, 3, 1).reshape(nparts, F1)
        mq = torch.stack([(mag[..., a:b] ** 2).sum(3) for a, b in tiles], 3).permute(0, 2, 3, 1).reshape(nparts, F1)
        tq = torch.stack([sq_tol(mag[..., a:b], e[..., a:b], 3, nrow) for a, b in tiles], 3).permute(0, 2, 3, 1) \
            .reshape(nparts, F1)
        gs, gq = part[:, :F1], part[:, F1:]
    else:
        rs, rq = R.stats(ref, (0, 2, 3))
        ms, mq = mag.sum((0, 2, 3)), (mag ** 2).sum((0, 2, 3))
        tq = sq_tol(mag, e, (0, 2, 3), nrow)
        gs, gq = part[:, :F1].sum(0), part[:, F1:].sum(0)
    ts = gamma(K + 3 + nrow) * ms
    if mode == "rounded":
        within(gs, rs, ts, "sum y1")
        within(gq, rq, tq, "sum y1^2")
    else:
        assert_exact(float(ms.max()), 1.0 / 4, "sum y1")
        same(gs, rs, "sum y1")
        if mode == "sparse":
            assert_exact(float(mq.max()), 1.0, "sum y1^2")
        exact_or_bound(gq, rq, mq, 1.0 / 16, tq, "sum y1^2")


# =================================================================================================== eav_tconv_wgrad
def wgrad_path(B, C, S, F1, K):
    jw = 64 if K <= 64 else (128 if K <= 128 else 256)
    ni = cdiv(K, jw)
    items = B * C * cdiv(S, 512)
    return f"NG{1 if F1 <= 8 else 2}-JW{jw}-NI{ni}{'as4' if ni == 3 else ''}-{'loop' if items > 1024 else 'flat'}"


# (B, C, S, F1, K): lag widths 64 / 128 / 256, NI 1-4, both filter groups, more than 1024 work items twice
TCONV_WGRAD = [(1, 1, 1, 1, 1), (2, 3, 700, 3, 64), (1, 2, 513, 9, 65), (2, 2, 1025, 16, 128), (1, 3, 512, 5, 129),
               (1, 2, 1024, 12, 256), (1, 2, 600, 7, 257), (2, 1, 1025, 16, 512), (1, 2, 1025, 2, 513),
               (1, 1, 700, 10, 768), (1, 2, 1030, 4, 769), (1, 1, 1025, 9, 1024), (3, 200, 1025, 2, 65),
               (2, 150, 1537, 9, 2)]


def bn6_data(mode, seed, F1, fold):
    """mean, invstd, scale, shift, m1, m2.  Exact mode: integer mean and m1, powers of two elsewhere, so that the staged
    dy = scale (g1 - m1 - (y1 - mean) invstd m2) is a multiple of 1/8 formed without rounding."""
    if mode == "exact":
        rows = [pick(seed, (F1,), [-1, 0, 1]), pick(seed + 1, (F1,), [0.5, 1]), pick(seed + 2, (F1,), [0.5, 1, -1]),
                ints(seed + 3, (F1,), -2, 2), pick(seed + 4, (F1,), [-1, 0, 1]), pick(seed + 5, (F1,), [0.5, 1, -0.5])]
    else:
        rows = [normal(seed, (F1,)), torch.from_numpy(synth.uniform(seed + 1, (F1,), 0.5, 2.0)), normal(seed + 2, (F1,)),
                normal(seed + 3, (F1,)), normal(seed + 4, (F1,), 0.3), normal(seed + 5, (F1,), 0.3)]
    bn = torch.stack(rows)
    if not fold:
        bn[4:] = 0.0
    return bn


@pytest.mark.parametrize("mode", ["exact", "rounded"])
@pytest.mark.parametrize("fold", [True, False], ids=["bnfold", "m0"])
@pytest.mark.parametrize("B,C,S,F1,K", TCONV_WGRAD,
                         ids=[f"B{b}-C{c}-S{s}-F{f}-K{k}-{wgrad_path(b, c, s, f, k)}" for b, c, s, f, k in TCONV_WGRAD])
def test_tconv_wgrad(B, C, S, F1, K, fold, mode):
    seed = seed_of("tconv_wgrad", B, C, S, F1, K, fold, mode)
    if mode == "exact":
        x, y1, g1 = (ints(seed + i, shp, -1, 1) for i, shp in enumerate([(B, C, S), (B, F1, C, S), (B, F1, C, S)]))
    else:
        x, y1, g1 = (normal(seed + i, shp) for i, shp in enumerate([(B, C, S), (B, F1, C, S), (B, F1, C, S)]))
    bn = bn6_data(mode, seed + 10, F1, fold)
    nparts = plain("eav_tconv_wgrad_nparts", B, C, S, F1, K)
    assert nparts == min(B * C * cdiv(S, 512), 1024)
    part = sentinel_buf(nparts * F1 * K)
    call("eav_tconv_wgrad", dev(x), dev(y1), dev(g1), dev(bn), part, B, C, S, F1, K)
    got = take(part, nparts * F1 * K, (nparts, F1, K), "part").double().sum(0)
    ref, mag = R.tconv_wgrad_ref(x, y1, g1, bn, K)
    if mode == "exact":
        assert_exact(float(mag.max()), 1.0 / 8, "dW")
        same(got, ref, "dW")
    else:
        # a term's dy carries 6 roundings (y1 - mean, * invstd, * m2, two subtractions, * scale); the B*C*S terms of a
        # tap are summed in fp32 within a row in an order the header leaves open, the rows in float64 here
        within(got, ref, gamma(B * C * S + 6) * mag, "dW")


# ======================================================================================== eav_spatial_fwd / eav_spatial_bwd
# (B, C, S, F1, D): float4 and scalar paths, ragged last quad, second tile
SPATIAL = [(1, 1, 1, 1, 1), (2, 30, 3, 5, 3), (1, 255, 4, 16, 8), (1, 256, 1023, 1, 3), (2, 30, 1024, 5, 8),
           (1, 30, 1028, 16, 1), (1, 255, 1029, 5, 3), (2, 256, 1029, 1, 8), (1, 1, 1028, 16, 3), (1, 30, 1023, 1, 1)]
SPATIAL_IDS = [f"B{b}-C{c}-S{s}-F{f}-D{d}-{'vec4' if s % 4 == 0 else 'scalar'}-tiles{cdiv(s, 1024)}"
               for b, c, s, f, d in SPATIAL]


def spatial_data(mode, seed, B, C, S, F1, D):
    """(y1, bn1 [4,F1], wd [F1*D,C], dz [B,F1*D,S])."""
    if mode == "exact":
        sc, sh = pick(seed, (F1,), [0.5, 1, 2]), pick(seed + 1, (F1,), [-2, 0, 2])
        o = pick(seed + 2, (B, F1, C, S), [-40, -18, 0, 0, 1, 1, 2, 3])
        y1 = (o - sh.view(1, -1, 1, 1)) / sc.view(1, -1, 1, 1)           # multiples of 1/2: scale y1 + shift = o exactly
        bn1 = torch.stack([pick(seed + 3, (F1,), [-1, 0, 1]), pick(seed + 4, (F1,), [0.5, 1]), sc, sh])
        return y1, bn1, sparse_pm1(seed + 5, F1 * D, C, 4), ints(seed + 7, (B, F1 * D, S), -1, 1)
    bn1 = torch.stack([normal(seed + 3, (F1,)), torch.from_numpy(synth.uniform(seed + 4, (F1,), 0.5, 2.0)),
                       normal(seed, (F1,)), normal(seed + 1, (F1,))])
    # BatchNorm outputs over (-17.5, 0) and beyond on both sides
    return normal(seed + 2, (B, F1, C, S), 4.0), bn1, normal(seed + 5, (F1 * D, C), 0.3), normal(seed + 7, (B, F1 * D, S))


def tiles_of(B, S, T=1024):
    return [(b, t0, min(t0 + T, S)) for b in range(B) for t0 in range(0, S, T)]


@pytest.mark.parametrize("mode", ["exact", "rounded"])
@pytest.mark.parametrize("elu", [0, 1], ids=["affine", "elu"])
@pytest.mark.parametrize("B,C,S,F1,D", SPATIAL, ids=SPATIAL_IDS)
def test_spatial_fwd(B, C, S, F1, D, elu, mode):
    y1, bn1, wd, _ = spatial_data(mode, seed_of("spatial", B, C, S, F1, D, elu, mode), B, C, S, F1, D)
    C2 = F1 * D
    nparts = plain("eav_spatial_nparts", B, S)
    assert nparts == B * cdiv(S, 1024)
    z = sentinel_buf(B * C2 * S)
    part = sentinel_buf(nparts * 2 * C2)
    call("eav_spatial_fwd", dev(y1), dev(bn1), dev(wd), z, part, B, C, S, F1, D, elu)
    z = take(z, B * C2 * S, (B, C2, S), "z")
    part = take(part, nparts * 2 * C2, (nparts, 2 * C2), "stat_part").double()
    ref, mag = R.spatial_fwd_ref(y1, bn1, wd, D, elu, f32_elu=(mode == "exact"))
    # per term: the affine (2 roundings, 1 as an fma) and, with the ELU, 1 ulp = 2 u of |ELU(o)| <= |o|; C terms
    e = gamma(C + 2 + 2 * elu) * mag
    rows = tiles_of(B, S)
    rs = torch.stack([ref[b, :, a:c].sum(1) for b, a, c in rows])
    rq = torch.stack([(ref[b, :, a:c] ** 2).sum(1) for b, a, c in rows])
    if mode == "exact":
        assert_exact(float(mag.max()), 1.0, "z")
        same(z, ref, "z")
        assert_exact(float(rq.max()), 1.0, "sum z^2")
        same(part[:, :C2], rs, "sum z")
        same(part[:, C2:], rq, "sum z^2")
    else:
        within(z, ref, e, "z")
        n = min(S, 1024)
        within(part[:, :C2], rs, torch.stack([gamma(C + 4 + n) * mag[b, :, a:c].sum(1) for b, a, c in rows]), "sum z")
        within(part[:, C2:], rq, torch.stack([sq_tol(mag[b, :, a:c], e[b, :, a:c], 1, n) for b, a, c in rows]),
               "sum z^2")


@pytest.mark.parametrize("mode", ["exact", "rounded"])
@pytest.mark.parametrize("elu", [0, 1], ids=["affine", "elu"])
@pytest.mark.parametrize("B,C,S,F1,D", SPATIAL, ids=SPATIAL_IDS)
def test_spatial_bwd(B, C, S, F1, D, elu, mode):
    y1, bn1, wd, dz = spatial_data(mode, seed_of("spatial", B, C, S, F1, D, elu, mode), B, C, S, F1, D)
    C2 = F1 * D
    nparts = plain("eav_spatial_nparts", B, S)
    g1 = sentinel_buf(B * F1 * C * S)
    sp = sentinel_buf(nparts * 2 * F1)
    wp = sentinel_buf(nparts * C2 * C)
    call("eav_spatial_bwd", dev(y1), dev(dz), dev(bn1), dev(wd), g1, sp, wp, B, C, S, F1, D, elu)
    g1 = take(g1, B * F1 * C * S, (B, F1, C, S), "g1")
    sp = take(sp, nparts * 2 * F1, (nparts, 2 * F1), "stat_part").double()
    wp = take(wp, nparts * C2 * C, (nparts, C2, C), "w_part").double()
    r = R.spatial_bwd_ref(y1, dz, bn1, wd, D, elu, f32_elu=(mode == "exact"))
    rows = tiles_of(B, S)
    rs = torch.stack([r["g1"][b, :, :, a:c].sum((1, 2)) for b, a, c in rows])
    rx = torch.stack([r["gx"][b, :, :, a:c].sum((1, 2)) for b, a, c in rows])
    ms = torch.stack([r["g1_mag"][b, :, :, a:c].sum((1, 2)) for b, a, c in rows])
    mx = torch.stack([r["gx_mag"][b, :, :, a:c].sum((1, 2)) for b, a, c in rows])
    rw = R.spatial_dw_rows(dz, r["a"], D, rows)
    if mode == "exact":
        same(g1, r["g1"], "g1")
        assert_exact(float(ms.max()), 1.0, "sum g1")
        assert_exact(float(mx.max()), 1.0 / 4, "sum g1 xhat")
        same(sp[:, :F1], rs, "sum g1")
        same(sp[:, F1:], rx, "sum g1 xhat")
        assert_exact(float(r["dW_mag"].max()), 1.0, "w_part")
        same(wp, rw, "w_part rows")
        same(wp.sum(0), r["dW"], "dW")
    else:
        # g1 = (D-term sum) * slope.  The slope ELU(o) + 1 = e^o is formed from the ELU OUTPUT, so it inherits that
        # output's ABSOLUTE error - 1 ulp of |ELU(o)| <= 1, i.e. 2 u |a| - however small e^o itself is, plus the affine's
        # rounding of o (gamma_2 |o|-bound) carried through d ELU / d o = e^o; the addition and the product round once
        # each.  Without the ELU the slope is 1 and only the sum rounds.
        u = 2.0 ** -24
        slope_err = (2 * u * r["a"].abs() + r["slope"] * gamma(2) * r["omag"]) if elu else 0.0
        e_g = r["g1_lin_mag"] * slope_err + gamma(D + 2) * r["g1_mag"]
        within(g1, r["g1"], e_g, "g1")
        # sums over the row's C * min(S, 1024) values; a term of the second is g1 (y1 - mean) invstd: three more roundings
        n = C * min(S, 1024)
        gb = r["g1_mag"] + e_g
        ts = torch.stack([e_g[b, :, :, a:c].sum((1, 2)) + gamma(n) * gb[b, :, :, a:c].sum((1, 2)) for b, a, c in rows])
        ex = (e_g + gamma(3) * gb) * r["xmag"]
        gxb = gb * r["xmag"]
        tx = torch.stack([ex[b, :, :, a:c].sum((1, 2)) + gamma(n) * gxb[b, :, :, a:c].sum((1, 2)) for b, a, c in rows])
        within(sp[:, :F1], rs, ts, "sum g1")
        within(sp[:, F1:], rx, tx, "sum g1 xhat")
        # dW: a term's ELU output is good to 1 ulp plus the affine's rounding, gamma_4 of the |o|-bound; <= 1024 terms a row
        within(wp.sum(0), r["dW"], gamma(min(S, 1024) + 4) * r["dW_mag"], "dW")


# =================================================================================================== eav_sepconv_fwd
# (B, C2, F2, T, K2): F2 splits into groups of four channels over the two wave pairs; one T < K2
SEPCONV = [(1, 1, 1, 1, 1), (2, 7, 4, 127, 2), (1, 64, 5, 128, 15), (2, 64, 63, 129, 16), (1, 7, 64, 300, 17),
           (1, 64, 64, 127, 31), (2, 1, 63, 300, 32), (1, 7, 5, 1, 16), (1, 64, 4, 129, 32), (2, 7, 1, 128, 31)]


@pytest.mark.parametrize("mode", ["exact", "sparse", "rounded"])
@pytest.mark.parametrize("B,C2,F2,T,K2", SEPCONV,
                         ids=[f"B{b}-C{c}-F{f}-T{t}-K{k}-groups{cdiv(f, 4)}" for b, c, f, t, k in SEPCONV])
def test_sepconv_fwd(B, C2, F2, T, K2, mode):
    seed = seed_of("sepconv", B, C2, F2, T, K2, mode)
    if mode == "exact":
        a, wdw, wp = ints(seed, (B, C2, T), -3, 3), ints(seed + 1, (C2, K2), -3, 3) / 4, ints(seed + 2, (F2, C2), -3, 3) / 4
    elif mode == "sparse":
        a, wdw, wp = ints(seed, (B, C2, T), -1, 1), sparse_pm1(seed + 1, C2, K2, 2), sparse_pm1(seed + 3, F2, C2, 4)
    else:
        a, wdw, wp = normal(seed, (B, C2, T)), normal(seed + 1, (C2, K2), 0.3), normal(seed + 2, (F2, C2), 0.3)
    nparts = plain("eav_sepconv_fwd_nparts", B, T)
    assert nparts == B * cdiv(T, 128)
    d3 = sentinel_buf(B * C2 * T)
    z = sentinel_buf(B * F2 * T)
    part = sentinel_buf(nparts * 2 * F2)
    call("eav_sepconv_fwd", dev(a), dev(wdw), dev(wp), d3, z, part, B, C2, F2, T, K2)
    d3 = take(d3, B * C2 * T, (B, C2, T), "d3")
    z = take(z, B * F2 * T, (B, F2, T), "z")
    part = take(part, nparts * 2 * F2, (nparts, 2 * F2), "stat_part").double()
    rd, rz = R.sepconv_fwd_ref(a, wdw, wp)
    md, mz = R.sepconv_fwd_ref(a.abs(), wdw.abs(), wp.abs())
    rows = tiles_of(B, T, 128)
    rs = torch.stack([rz[b, :, s:e].sum(1) for b, s, e in rows])
    rq = torch.stack([(rz[b, :, s:e] ** 2).sum(1) for b, s, e in rows])
    ms = torch.stack([mz[b, :, s:e].sum(1) for b, s, e in rows])
    mq = torch.stack([(mz[b, :, s:e] ** 2).sum(1) for b, s, e in rows])
    ez = gamma(K2 + C2) * mz                      # a term of z carries the K2-term sum of its d3, then C2 terms
    n = min(T, 128)
    tq = torch.stack([sq_tol(mz[b, :, s:e], ez[b, :, s:e], 1, n) for b, s, e in rows])
    if mode == "rounded":
        within(d3, rd, gamma(K2) * md, "d3")
        within(z, rz, ez, "z")
        within(part[:, :F2], rs, gamma(K2 + C2 + n) * ms, "sum z")
        within(part[:, F2:], rq, tq, "sum z^2")
    else:
        assert_exact(float(md.max()), 1.0 / 4, "d3")
        assert_exact(float(mz.max()), 1.0 / 16, "z")
        assert_exact(float(ms.max()), 1.0 / 16, "sum z")
        same(d3, rd, "d3")
        same(z, rz, "z")
        same(part[:, :F2], rs, "sum z")
        if mode == "sparse":
            assert_exact(float(mq.max()), 1.0, "sum z^2")
        exact_or_bound(part[:, F2:], rq, mq, 1.0 / 256, tq, "sum z^2")


# ================================================================================================= eav_pointwise_bwd
# (B, C2, F2, T): both regimes of min(B ceil(T/64), 512); F2 * C2 from 1 to 4096
POINTWISE = [(1, 1, 1, 1), (2, 7, 5, 100), (40, 16, 16, 900), (3, 64, 64, 129), (1, 64, 1, 64), (2, 1, 64, 65),
             (9, 7, 63, 3700)]


@pytest.mark.parametrize("mode", ["exact", "rounded"])
@pytest.mark.parametrize("B,C2,F2,T", POINTWISE,
                         ids=[f"B{b}-C{c}-F{f}-T{t}-{'loop' if b * cdiv(t, 64) > 512 else 'flat'}"
                              for b, c, f, t in POINTWISE])
def test_pointwise_bwd(B, C2, F2, T, mode):
    seed = seed_of("pointwise", B, C2, F2, T, mode)
    if mode == "exact":
        du, d3, wp = ints(seed, (B, F2, T), -3, 3), ints(seed + 1, (B, C2, T), -3, 3), ints(seed + 2, (F2, C2), -3, 3) / 4
    else:
        du, d3, wp = normal(seed, (B, F2, T)), normal(seed + 1, (B, C2, T)), normal(seed + 2, (F2, C2), 0.3)
    nparts = plain("eav_pointwise_bwd_nparts", B, T)
    assert nparts == min(B * cdiv(T, 64), 512)
    dd3 = sentinel_buf(B * C2 * T)
    part = sentinel_buf(nparts * F2 * C2)
    call("eav_pointwise_bwd", dev(du), dev(d3), dev(wp), dd3, part, B, C2, F2, T)
    dd3 = take(dd3, B * C2 * T, (B, C2, T), "dd3")
    got = take(part, nparts * F2 * C2, (nparts, F2, C2), "w_part").double().sum(0)
    rd, rw = R.pointwise_bwd_ref(du, d3, wp)
    md, mw = R.pointwise_bwd_ref(du.abs(), d3.abs(), wp.abs())
    if mode == "exact":
        assert_exact(float(md.max()), 1.0 / 4, "dd3")
        assert_exact(float(mw.max()), 1.0, "dWp")
        same(dd3, rd, "dd3")
        same(got, rw, "dWp")
    else:
        within(dd3, rd, gamma(F2) * md, "dd3")
        within(got, rw, gamma(B * T) * mw, "dWp")     # B*T terms; a row chains those of its block's work items in fp32


# ======================================================================================================= eav_dwt_bwd
# (B, C2, T, K2): one T < K2
DWT = [(1, 1, 1, 1), (2, 7, 255, 2), (1, 64, 256, 15), (2, 3, 257, 16), (1, 7, 700, 17), (1, 2, 255, 31),
       (2, 64, 256, 32), (1, 7, 9, 16), (1, 3, 700, 32)]


@pytest.mark.parametrize("mode", ["exact", "rounded"])
@pytest.mark.parametrize("B,C2,T,K2", DWT, ids=[f"B{b}-C{c}-T{t}-K{k}" for b, c, t, k in DWT])
def test_dwt_bwd(B, C2, T, K2, mode):
    seed = seed_of("dwt", B, C2, T, K2, mode)
    if mode == "exact":
        g, a, w = ints(seed, (B, C2, T), -3, 3), ints(seed + 1, (B, C2, T), -3, 3), ints(seed + 2, (C2, K2), -3, 3) / 4
    else:
        g, a, w = normal(seed, (B, C2, T)), normal(seed + 1, (B, C2, T)), normal(seed + 2, (C2, K2), 0.3)
    da = sentinel_buf(B * C2 * T)
    part = sentinel_buf(B * C2 * K2)
    call("eav_dwt_bwd", dev(g), dev(a), dev(w), da, part, B, C2, T, K2)
    da = take(da, B * C2 * T, (B, C2, T), "da")
    part = take(part, B * C2 * K2, (B, C2, K2), "w_part")         # row b, as the header lays them out
    rd, rw = R.dwt_bwd_ref(g, a, w)
    md, mw = R.dwt_bwd_ref(g.abs(), a.abs(), w.abs())
    if mode == "exact":
        assert_exact(float(md.max()), 1.0 / 4, "da")
        assert_exact(float(mw.max()), 1.0, "w_part")
        same(da, rd, "da")
        same(part, rw, "w_part")
    else:
        within(da, rd, gamma(K2) * md, "da")
        within(part, rw, gamma(T) * mw, "w_part")


# ==================================================================================================== eav_dconv_fwd
# (B, Cin, Cout, T, K)
DCONV = [(1, 1, 1, 1, 1), (2, 7, 8, 63, 2), (1, 8, 7, 64, 5), (2, 9, 64, 65, 15), (1, 64, 9, 200, 16), (1, 64, 64, 65, 2),
         (2, 1, 9, 200, 16), (1, 9, 1, 63, 16), (1, 7, 64, 64, 15)]


@pytest.mark.parametrize("mode", ["exact", "sparse", "rounded"])
@pytest.mark.parametrize("stat", [True, False], ids=["stats", "nostats"])
@pytest.mark.parametrize("transposed", [0, 1], ids=["fwd", "transposed"])
@pytest.mark.parametrize("B,Cin,Cout,T,K", DCONV,
                         ids=[f"B{b}-Ci{ci}-Co{co}-T{t}-K{k}-pad{(k - 1) // 2}.{k - 1 - (k - 1) // 2}"
                              for b, ci, co, t, k in DCONV])
def test_dconv_fwd(B, Cin, Cout, T, K, transposed, stat, mode):
    """transposed = 1 is checked against the float64 input gradient of the 'same' conv with the FORWARD weight
    [Cin][Cout][K] (Cin = that conv's output channels)."""
    seed = seed_of("dconv", B, Cin, Cout, T, K, transposed, mode)
    wshape = (Cin, Cout, K) if transposed else (Cout, Cin, K)
    if mode == "exact":
        x, w = ints(seed, (B, Cin, T), -3, 3), ints(seed + 1, wshape, -3, 3) / 4
    elif mode == "sparse":
        x = ints(seed, (B, Cin, T), -1, 1)
        w = sparse_pm1(seed + 1, 1, Cin * Cout * K, 3 * Cout).view(wshape)        # about three +-1 taps per output channel
    else:
        x, w = normal(seed, (B, Cin, T)), normal(seed + 1, wshape, 0.3)
    nparts = plain("eav_dconv_fwd_nparts", B, T)
    assert nparts == B * cdiv(T, 64)
    out = sentinel_buf(B * Cout * T)
    part = sentinel_buf(nparts * 2 * Cout) if stat else None
    call("eav_dconv_fwd", dev(x), dev(w), out, part, B, Cin, Cout, T, K, transposed)
    out = take(out, B * Cout * T, (B, Cout, T), "out")
    ref, mag = R.dconv_fwd_ref(x, w, transposed), R.dconv_fwd_ref(x.abs(), w.abs(), transposed)
    e = gamma(Cin * 16) * mag                      # the kernel walks 16 taps per input channel (zeros beyond K)
    if mode == "rounded":
        within(out, ref, e, "out")
    else:
        assert_exact(float(mag.max()), 1.0 / 4, "out")
        same(out, ref, "out")
    if not stat:
        return
    part = take(part, nparts * 2 * Cout, (nparts, 2 * Cout), "stat_part").double()
    rows = tiles_of(B, T, 64)
    rs = torch.stack([ref[b, :, s:t].sum(1) for b, s, t in rows])
    rq = torch.stack([(ref[b, :, s:t] ** 2).sum(1) for b, s, t in rows])
    ms = torch.stack([mag[b, :, s:t].sum(1) for b, s, t in rows])
    mq = torch.stack([(mag[b, :, s:t] ** 2).sum(1) for b, s, t in rows])
    n = min(T, 64)
    tq = torch.stack([sq_tol(mag[b, :, s:t], e[b, :, s:t], 1, n) for b, s, t in rows])
    if mode == "rounded":
        within(part[:, :Cout], rs, gamma(Cin * 16 + n) * ms, "sum out")
        within(part[:, Cout:], rq, tq, "sum out^2")
    else:
        assert_exact(float(ms.max()), 1.0 / 4, "sum out")
        same(part[:, :Cout], rs, "sum out")
        if mode == "sparse":
            assert_exact(float(mq.max()), 1.0, "sum out^2")
        exact_or_bound(part[:, Cout:], rq, mq, 1.0 / 16, tq, "sum out^2")


# ================================================================================================== eav_dconv_wgrad
# (B, Cin, Cout, T, K): Cout % 4 != 0 in most
DCONV_WGRAD = [(1, 1, 1, 127, 1), (2, 7, 9, 128, 2), (1, 8, 7, 129, 5), (2, 9, 64, 300, 15), (1, 64, 5, 127, 16),
               (1, 64, 64, 129, 16), (2, 1, 6, 300, 15), (1, 9, 8, 128, 16)]


@pytest.mark.parametrize("mode", ["exact", "rounded"])
@pytest.mark.parametrize("B,Cin,Cout,T,K", DCONV_WGRAD,
                         ids=[f"B{b}-Ci{ci}-Co{co}-T{t}-K{k}" for b, ci, co, t, k in DCONV_WGRAD])
def test_dconv_wgrad(B, Cin, Cout, T, K, mode):
    seed = seed_of("dconv_wgrad", B, Cin, Cout, T, K, mode)
    if mode == "exact":
        dy, x = ints(seed, (B, Cout, T), -3, 3), ints(seed + 1, (B, Cin, T), -3, 3)
    else:
        dy, x = normal(seed, (B, Cout, T)), normal(seed + 1, (B, Cin, T))
    n = B * Cout * Cin * K
    part = sentinel_buf(n)
    call("eav_dconv_wgrad", dev(dy), dev(x), part, B, Cin, Cout, T, K)
    part = take(part, n, (B, Cout, Cin, K), "part")               # row b, as the header lays them out
    ref, mag = R.dconv_wgrad_ref(dy, x, K), R.dconv_wgrad_ref(dy.abs(), x.abs(), K)
    if mode == "exact":
        assert_exact(float(mag.max()), 1.0, "part")
        same(part, ref, "part")
    else:
        within(part, ref, gamma(cdiv(T, 128) * 128) * mag, "part")    # T terms, walked in whole tiles of 128 (zeros beyond T)


# ========================================================================================================== refusals
REFUSED = [("eav_tconv_fwd", "pppp", (1, 1, 8, 4, 1025)), ("eav_tconv_fwd", "pppp", (1, 1, 8, 17, 8)),
           ("eav_tconv_wgrad", "ppppp", (1, 1, 8, 4, 1025)), ("eav_tconv_wgrad", "ppppp", (1, 1, 8, 17, 8)),
           ("eav_spatial_fwd", "ppppp", (1, 257, 8, 4, 2, 0)), ("eav_spatial_fwd", "ppppp", (1, 4, 8, 4, 9, 0)),
           ("eav_spatial_fwd", "ppppp", (1, 4, 8, 17, 2, 0)), ("eav_spatial_bwd", "ppppppp", (1, 257, 8, 4, 2, 0)),
           ("eav_spatial_bwd", "ppppppp", (1, 4, 8, 4, 9, 1)), ("eav_sepconv_fwd", "pppppp", (1, 65, 4, 8, 4)),
           ("eav_sepconv_fwd", "pppppp", (1, 4, 65, 8, 4)), ("eav_sepconv_fwd", "pppppp", (1, 4, 4, 8, 33)),
           ("eav_pointwise_bwd", "ppppp", (1, 65, 4, 8)), ("eav_pointwise_bwd", "ppppp", (1, 4, 65, 8)),
           ("eav_dwt_bwd", "ppppp", (1, 4, 8, 33)), ("eav_dwt_bwd", "ppppp", (1, 65, 8, 4)),
           ("eav_dconv_fwd", "pppp", (1, 65, 4, 8, 4, 0)), ("eav_dconv_fwd", "pppp", (1, 4, 65, 8, 4, 1)),
           ("eav_dconv_fwd", "pppp", (1, 4, 4, 8, 17, 0)), ("eav_dconv_wgrad", "ppp", (1, 4, 4, 8, 17)),
           ("eav_dconv_wgrad", "ppp", (1, 65, 4, 8, 4))]


@pytest.mark.parametrize("name,ptrs,dims", REFUSED, ids=[f"{n}-{'-'.join(map(str, d))}" for n, _, d in REFUSED])
def test_past_a_documented_limit_is_refused_without_a_launch(name, ptrs, dims):
    """One value past each limit of the header: a negative status with a message, and no kernel runs (the outputs keep
    their sentinel)."""
    from eav_amd import _lib
    bufs = [sentinel_buf(64) for _ in ptrs]
    with pytest.raises(_lib.EavError, match=name) as err:
        call(name, *bufs, *dims)
    assert "failed (-" in str(err.value)
    for b in bufs:
        assert (b.cpu().view(torch.int32) == SENT).all()
