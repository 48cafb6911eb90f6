"""Per-kernel parity of the ShallowConvNet / transformer-glue kernels (csrc/shallow_tf.hip, through the C ABI) against
the float64 references of tests/shallow_tf_ref.py, written from the contracts in include/eav_hip.h.

Data modes.  "exact": small integers, quarter-integer weights, power-of-two BatchNorm factors and dropout scale 2, so
that every fp32 product and partial sum is exact in any order (asserted from the sum of the absolute terms of the
largest output); the kernel must equal the reference bit for bit.  "rounded": synth normal data, every element held to
gamma(n + c) * magnitude (n terms, c extra roundings per term, derived beside each check).

Every output buffer, partial buffers included, is filled with a NaN sentinel and carries a guard band: all the contract
says is written must be written, the band must be untouched.

The logarithm of eav_sqpool_log_fwd is the device library's logf.  Its output is compared with the float64 log of the
kernel's OWN pooled mean (itself held to its bound).  test_device_logf_error measures logf against float64 over the
clamp range [1e-7, 1e4] on a log-spaced grid of 67 * 62 * 256 = 1 063 424 (> 2^20) arguments: the largest error measured
on the MI355X is 2.287 ulp of the result (at x = 2252.55444), LOGF_ULP = 2.29; the checks allow twice that, the factor
covering the arguments the grid did not sample."""
import numpy as np
import pytest
import torch

from eav_amd import synth
from tests import shallow_tf_ref as R
from tests.audio_conv_ref import f32_scale, gamma
from tests.kernel_check import SENT, assert_exact, dev, ints, keep_mask, normal, same, seed_of, sentinel_buf, take, within

pytestmark = pytest.mark.gpu

LOGF_ULP = 2.29             # measured: see the module docstring and test_device_logf_error
GRID_CAP = 16384 * 256      # elements one pass of the element-wise grids covers


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


def pick(seed, shape, values):
    v = np.asarray(values, np.float32)
    n = int(np.prod(shape))
    return torch.from_numpy(v[(synth.splitmix64(seed, n) % np.uint64(len(v))).astype(np.int64)].reshape(shape))


def bits(t):
    return t.contiguous().view(torch.int32)


# ============================================================================================ eav_shallow_embed_fwd / _bwd
# (B, C, ldv, S, NF, KC): ldv = 32 > C carries NaN in the padding columns of wv; S = KC is a single token
EMBED = [(1, 1, 1, 1, 1, 1), (2, 30, 32, 13, 40, 13), (1, 32, 32, 63, 48, 16), (2, 30, 30, 64, 1, 13),
         (1, 1, 32, 65, 40, 1), (1, 30, 32, 127, 48, 13), (2, 32, 32, 128, 40, 16), (1, 30, 32, 129, 40, 13),
         (1, 30, 32, 500, 40, 13), (2, 1, 1, 500, 48, 16)]
EMBED_IDS = [f"B{b}-C{c}-ldv{l}-S{s}-NF{n}-KC{k}" for b, c, l, s, n, k in EMBED]


def embed_data(mode, seed, B, C, ldv, S, NF, KC):
    if mode == "exact":
        x, wc, wv = ints(seed, (B, C, S), -3, 3), ints(seed + 1, (NF, KC), -3, 3) / 4, ints(seed + 2, (NF, C), -3, 3) / 4
    else:
        x, wc, wv = normal(seed, (B, C, S)), normal(seed + 1, (NF, KC), 0.3), normal(seed + 2, (NF, C), 0.3)
    wvp = torch.full((NF, ldv), float("nan"))
    wvp[:, :C] = wv
    return x, wc, wv, wvp


@pytest.mark.parametrize("mode", ["exact", "rounded"])
@pytest.mark.parametrize("B,C,ldv,S,NF,KC", EMBED, ids=EMBED_IDS)
def test_shallow_embed_fwd(B, C, ldv, S, NF, KC, mode):
    x, wc, wv, wvp = embed_data(mode, seed_of("embed", B, C, ldv, S, NF, KC, mode), B, C, ldv, S, NF, KC)
    T = S - KC + 1
    u = sentinel_buf(B * NF * S)
    v = sentinel_buf(B * T * NF)
    call("eav_shallow_embed_fwd", dev(x), dev(wc), dev(wvp), ldv, u, v, B, C, S, NF, KC)
    u = take(u, B * NF * S, (B, NF, S), "u")
    v = take(v, B * T * NF, (B, T, NF), "v")
    ru, rv = R.shallow_embed_fwd_ref(x, wc, wv)
    mu, mv = R.shallow_embed_fwd_ref(x.abs(), wc.abs(), wv.abs())
    if mode == "exact":
        assert_exact(float(mu.max()), 1.0 / 4, "u")
        assert_exact(float(mv.max()), 1.0 / 16, "v")
        same(u, ru, "u")
        same(v, rv, "v")
    else:
        within(u, ru, gamma(C) * mu, "u")
        within(v, rv, gamma(C + KC) * mv, "v")      # a term of v carries the C-term sum of its u, then KC terms


@pytest.mark.parametrize("mode", ["exact", "rounded"])
@pytest.mark.parametrize("B,C,ldv,S,NF,KC", EMBED, ids=EMBED_IDS)
def test_shallow_embed_bwd(B, C, ldv, S, NF, KC, mode):
    seed = seed_of("embed", B, C, ldv, S, NF, KC, mode)
    x, wc, wv, _ = embed_data(mode, seed, B, C, ldv, S, NF, KC)
    T = S - KC + 1
    u = R.shallow_embed_fwd_ref(x, wc, wv)[0].float()              # the forward's stored projection, as fp32 input
    dv = ints(seed + 5, (B, T, NF), -3, 3) if mode == "exact" else normal(seed + 5, (B, T, NF))
    nparts = plain("eav_shallow_embed_nparts", B, S)
    assert nparts == B * cdiv(S, 64)
    pc = sentinel_buf(nparts * NF * KC)
    pv = sentinel_buf(nparts * NF * C)
    call("eav_shallow_embed_bwd", dev(dv), dev(x), dev(u), dev(wc), pc, pv, B, C, S, NF, KC)
    pc = take(pc, nparts * NF * KC, (nparts, NF, KC), "part_c").double().sum(0)
    pv = take(pv, nparts * NF * C, (nparts, NF, C), "part_v").double().sum(0)
    rc, rv = R.shallow_embed_bwd_ref(dv, x, u, wc)
    mc, mv = R.shallow_embed_bwd_ref(dv.abs(), x.abs(), u.abs(), wc.abs())
    if mode == "exact":
        assert_exact(float(mc.max()), 1.0 / 4, "dWc")
        assert_exact(float(mv.max()), 1.0 / 4, "dWv")
        same(pc, rc, "dWc")
        same(pv, rv, "dWv")
    else:
        within(pc, rc, gamma(B * T) * mc, "dWc")
        within(pv, rv, gamma(B * S + KC) * mv, "dWv")   # a term of dWv carries the KC-term sum of its e


# ======================================================================= eav_relu_dropout / _bwd / eav_dropout_add
EW_N = [1, 255, 256, 257, GRID_CAP + 300]


def ew_data(seed, n):
    """Integers in [-3, 3] with -0.0, +0.0 and denormals of both signs planted."""
    h = ints(seed, (n,), -3, 3)
    for i, v in enumerate([-0.0, 0.0, 1e-40, -1e-40]):
        h[(7 * i + 3) % n::97] = v
    return h


@pytest.mark.parametrize("p", [0.0, 0.5, 0.1], ids=["p0", "p0.5", "p0.1"])
@pytest.mark.parametrize("n", EW_N, ids=[f"n{n}{'-wraps' if n > GRID_CAP else ''}" for n in EW_N])
def test_relu_dropout_with_a_mask_and_its_backward(n, p):
    """Kept values are exactly fl(h * 1.f/(1.f-p)): one rounding, as .float() of the float64 product."""
    seed = seed_of("relu", n, p)
    h, dact = ew_data(seed, n), ints(seed + 1, (n,), -3, 3)
    mask = keep_mask(seed + 2, (n,), p) if p > 0 else None
    buf = sentinel_buf(n)
    buf[:n] = dev(h)
    call("eav_relu_dropout", buf, n, p, 0, dev(mask) if p > 0 else None, None)
    act = take(buf, n, (n,), "act")
    same(act, R.relu_dropout_ref(h, p, mask).float(), "act")
    assert not (act < 0).any()
    g = sentinel_buf(n)
    g[:n] = dev(dact)
    call("eav_relu_dropout_bwd", g, dev(act), n, p)
    same(take(g, n, (n,), "dact"), R.relu_dropout_bwd_ref(dact, act, p).float(), "dact")


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_relu_dropout_propagates_nan_like_torch(p):
    """nn.ReLU returns NaN for NaN, nn.Dropout leaves it NaN whether kept or dropped; torch's ReLU backward passes the
    gradient at a NaN, and the backward here does so with the scale of a kept element."""
    n = 600
    h, dact = ew_data(seed_of("relunan"), n), ints(seed_of("relunan") + 1, (n,), 1, 3)
    mask = keep_mask(seed_of("relunan") + 2, (n,), p) if p > 0 else None
    planted = [0, 5, 255, 256, 599]
    h[planted] = float("nan")
    if p > 0:
        mask[0], mask[5] = 0, 1
    buf = sentinel_buf(n)
    buf[:n] = dev(h)
    call("eav_relu_dropout", buf, n, p, 0, dev(mask) if p > 0 else None, None)
    act = take(buf, n, (n,), "act")                                # (the planted NaN has another payload than the sentinel)
    ref = torch.relu(h.double()) * R.drop_mult((n,), p, mask)     # torch's own ops
    assert torch.isnan(act[planted]).all() and int(torch.isnan(act).sum()) == len(planted)
    same(act, ref.float(), "act")
    g = dev(dact.clone())
    call("eav_relu_dropout_bwd", g, dev(act), n, p)
    torch.cuda.synchronize()
    g = g.cpu()
    same(g, R.relu_dropout_bwd_ref(dact, act, p).float(), "dact")
    s = f32_scale(p) if p > 0 else 1.0
    assert (g[planted].double() == dact[planted].double() * s).all()


@pytest.mark.parametrize("form", ["resid", "noresid", "alias"])
@pytest.mark.parametrize("p", [0.0, 0.5, 0.1], ids=["p0", "p0.5", "p0.1"])
@pytest.mark.parametrize("n", EW_N, ids=[f"n{n}{'-wraps' if n > GRID_CAP else ''}" for n in EW_N])
def test_dropout_add(n, p, form):
    seed = seed_of("dropadd", n, p)
    y, resid = ew_data(seed, n), ew_data(seed + 1, n)
    mask = keep_mask(seed + 2, (n,), p) if p > 0 else None
    out = sentinel_buf(n)
    if form == "alias":                                            # out aliases resid (the header allows it)
        out[:n] = dev(resid)
        rd = out
    else:
        rd = dev(resid) if form == "resid" else None
    call("eav_dropout_add", dev(y), rd, out, n, p, 0, dev(mask) if p > 0 else None, None)
    got = take(out, n, (n,), "out")
    ref = R.dropout_add_ref(y, None if form == "noresid" else resid, p, mask)
    if p == 0.1 and form != "noresid":
        # resid + fl(y s) or one fma: at most two roundings of the two-term sum
        # (the planted denormals: a rounding in the subnormal range errs by up to half its fixed spacing 2^-149)
        within(got, ref, gamma(2) * R.dropout_add_ref(y.abs(), resid.abs(), p, mask) + 2.0 ** -149, "out")
    else:
        same(got, ref.float(), "out")                              # p in {0, 0.5}: exact; no residual: one rounding


@pytest.mark.parametrize("n", [100_000, GRID_CAP + 300], ids=["n100000", "wraps"])
def test_generated_dropout_mask_properties(n):
    """No reference exists for the generated mask: the keep fraction lies in the binomial 5-sigma interval, the pattern
    depends on (seed, index) alone - not on the data -, (seed, *seed_dev = k) draws the mask of (seed + 2k, NULL) bit for
    bit, and kept values are exactly fl(y * 1.f/(1.f-p))."""
    p, seed, k = 0.3, 0x5EED, 5
    y1, y2 = ints(seed_of("gen", n), (n,), 1, 3), ints(seed_of("gen", n) + 1, (n,), 1, 3)
    cnt = dev(torch.tensor([k], dtype=torch.int64))

    def relu(y, s, c):
        b = sentinel_buf(n)
        b[:n] = dev(y)
        call("eav_relu_dropout", b, n, p, s, None, c)
        return take(b, n, (n,), "act")

    def dadd(y, s, c):
        b = sentinel_buf(n)
        call("eav_dropout_add", dev(y), None, b, n, p, s, None, c)
        return take(b, n, (n,), "out")

    for f in (relu, dadd):
        a, b2, c, d, other = f(y1, seed, None), f(y2, seed, None), f(y1, seed, cnt), f(y1, seed + 2 * k, None), f(y1, seed + 1, None)
        keep = a != 0
        assert torch.equal(keep, b2 != 0), "the pattern depends on the data"
        assert torch.equal(bits(c), bits(d)), "seed_dev"
        assert not torch.equal(keep, c != 0) and not torch.equal(keep, other != 0)
        frac = float(keep.double().mean())
        assert abs(frac - (1 - p)) < 5 * (p * (1 - p) / n) ** 0.5, frac
        same(a[keep], (y1[keep].double() * f32_scale(p)).float(), "kept values")


# ====================================================================================================== eav_add_strided
# (M, n, lda, ldb, ldo); ldb = 0: b NULL
ADD = [(1, 1, 1, 1, 1), (5, 3, 7, 4, 9), (300, 40, 64, 40, 192), (40, 30, 30, 0, 32), (33000, 128, 128, 130, 128),
       (17, 40, 40, 0, 64)]


@pytest.mark.parametrize("M,n,lda,ldb,ldo", ADD,
                         ids=[f"M{m}-n{n}-ld{a}.{b}.{o}{'-wraps' if m * n > GRID_CAP else ''}" for m, n, a, b, o in ADD])
def test_add_strided(M, n, lda, ldb, ldo):
    seed = seed_of("add", M, n, lda, ldb, ldo)
    a = normal(seed, (M, lda))
    b = normal(seed + 1, (M, ldb)) if ldb else None
    out = sentinel_buf(M * ldo)
    call("eav_add_strided", dev(a), lda, dev(b) if ldb else None, ldb, out, ldo, M, n)
    torch.cuda.synchronize()
    h = out.cpu()
    assert (bits(h[M * ldo:]) == SENT).all(), "guard band"
    h = h[:M * ldo].view(M, ldo)
    assert (bits(h[:, n:]) == SENT).all(), "columns beyond n written"
    same(h[:, :n], R.add_strided_ref(a, b, n).float(), "out")     # one addition: the rounded float64 sum


def test_add_strided_in_place_as_the_model_calls_it():
    """transformer_eeg.py, the "+ V" branch of the attention backward: out == a, a block of 40 columns at offset 128 of
    rows of 192, b with rows of 40."""
    M, n = 77, 40
    qkv, da = normal(seed_of("inplace"), (M, 192)), normal(seed_of("inplace") + 1, (M, n))
    d = dev(qkv.clone())
    from eav_amd import _lib
    _lib.call("eav_add_strided", d.data_ptr() + 4 * 128, 192, dev(da).data_ptr(), n, d.data_ptr() + 4 * 128, 192, M, n, None)
    torch.cuda.synchronize()
    want = qkv.clone()
    want[:, 128:168] = (qkv[:, 128:168].double() + da.double()).float()
    assert torch.equal(bits(d.cpu()), bits(want))


# ========================================================================================================= eav_colstats
# (M, N, ld): 256 % N != 0 leaves lanes idle; N > 128 leaves one row lane
COLSTATS = [(1, 1, 1), (255, 40, 40), (256, 85, 96), (257, 128, 128), (1000, 129, 130), (1000, 256, 256), (257, 40, 64),
            (1000, 85, 85), (256, 256, 300)]


@pytest.mark.parametrize("mode", ["exact", "rounded"])
@pytest.mark.parametrize("M,N,ld", COLSTATS, ids=[f"M{m}-N{n}-ld{l}-lanes{256 // n}" for m, n, l in COLSTATS])
def test_colstats(M, N, ld, mode):
    seed = seed_of("colstats", M, N, ld, mode)
    x = ints(seed, (M, ld), -3, 3) if mode == "exact" else normal(seed, (M, ld))
    nparts = plain("eav_colstats_nparts", M)
    assert nparts == cdiv(M, 256)
    part = sentinel_buf(nparts * 2 * N)
    call("eav_colstats", dev(x), part, M, N, ld)
    part = take(part, nparts * 2 * N, (nparts, 2 * N), "part")
    ref = R.colstats_ref(x, N)                                     # row p = rows [256 p, 256 p + 256), as the header says
    if mode == "exact":
        assert_exact(256 * 9, 1.0, "colstats")
        same(part, ref, "part")
    else:
        mag = R.colstats_ref(x.abs(), N)
        tol = torch.cat([gamma(256) * mag[:, :N], gamma(257) * mag[:, N:]], 1)      # the squares round once more
        within(part, ref, tol, "part")


# ===================================================================================== eav_sqpool_log_fwd / _bwd
def ulp32(v):
    return torch.from_numpy(np.spacing(np.abs(v.double().numpy()).astype(np.float32)).astype(np.float64))


def test_device_logf_error():
    """The device logf against float64 over the clamp range: with win = stride = 1, scale 1 and shift 0 the kernel's
    pooled value is fl(v^2) and out = logf(pooled), so every argument and its logarithm come back through the C ABI."""
    B, NP, NF = 67, 62, 256
    n = B * NP * NF
    assert n >= 2 ** 20
    arg = np.exp(np.linspace(np.log(1e-7), np.log(1e4), n))
    v = torch.from_numpy(np.sqrt(arg).astype(np.float32)).view(B, NP, NF)
    bn = torch.zeros(4, NF)
    bn[1:3] = 1.0
    pooled, out = sentinel_buf(n), sentinel_buf(n)
    call("eav_sqpool_log_fwd", dev(v), dev(bn), pooled, out, B, NP, NF, NP, 1, 1, 1e-7, 1e4, 0.0, 0, None, None)
    pooled, out = take(pooled, n, (n,), "pooled"), take(out, n, (n,), "out")
    same(pooled, (v.double() ** 2).float().transpose(1, 2).reshape(n), "pooled")
    ref = torch.log(torch.clamp(pooled.double(), float(np.float32(1e-7)), float(np.float32(1e4))))
    err = (out.double() - ref).abs() / ulp32(ref)
    worst = int(err.argmax())
    print(f"device logf: max error {float(err.max()):.3f} ulp at x = {float(pooled[worst]):.9g} over {n} arguments")
    assert float(err.max()) <= 2 * LOGF_ULP


# (B, T, NF, NP, win, stride): every T leaves tail tokens beyond the last window
POOL = [(2, 500, 40, 65, 35, 7), (2, 40, 1, 5, 2, 7), (1, 30, 40, 6, 4, 4), (2, 33, 256, 4, 8, 3), (1, 70, 256, 62, 8, 1),
        (3, 21, 40, 1, 16, 16)]
POOL_IDS = [f"B{b}-T{t}-NF{f}-NP{n}-win{w}-str{s}-{'gaps' if w < s else ('tiled' if w == s else 'overlap')}"
            for b, t, f, n, w, s in POOL]


def pool_data(mode, seed, B, T, NF):
    """v [B,T,NF] and bn = mean, invstd, scale, shift."""
    if mode == "exact":
        v = ints(seed, (B, T, NF), -3, 3)
        bn = torch.stack([pick(seed + 1, (NF,), [-1, 0, 1]), pick(seed + 2, (NF,), [0.5, 1, 2]),
                          pick(seed + 3, (NF,), [0.5, 1, 2]), pick(seed + 4, (NF,), [-1, 0, 1])])
    else:
        v = normal(seed, (B, T, NF))
        bn = torch.stack([normal(seed + 1, (NF,)), torch.from_numpy(synth.uniform(seed + 2, (NF,), 0.5, 2.0)),
                          normal(seed + 3, (NF,)), normal(seed + 4, (NF,))])
    return v, bn


def clamp_bounds(pooled):
    """lo, hi = two of the values themselves (fp32): some means lie below lo, some above hi, one or more on each bound."""
    srt = pooled.float().flatten().unique()
    k = max(1, len(srt) // 8) if len(srt) > 2 else 0
    return float(srt[k]), float(srt[len(srt) - 1 - k])


@pytest.mark.parametrize("mode", ["exact", "rounded"])
@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "mask"])
@pytest.mark.parametrize("B,T,NF,NP,win,stride", POOL, ids=POOL_IDS)
def test_sqpool_log_fwd(B, T, NF, NP, win, stride, drop, mode):
    seed = seed_of("pool", B, T, NF, NP, win, stride, drop, mode)
    v, bn = pool_data(mode, seed, B, T, NF)
    assert (NP - 1) * stride + win < T
    rp, _, _, mp = R.sqpool_ref(v, bn, NP, win, stride)
    lo, hi = clamp_bounds(rp)
    p = 0.5 if drop else 0.0
    mask = keep_mask(seed + 9, (B, NF, NP), p) if drop else None
    n = B * NF * NP
    pooled, out = sentinel_buf(n), sentinel_buf(n)
    call("eav_sqpool_log_fwd", dev(v), dev(bn), pooled, out, B, T, NF, NP, win, stride, lo, hi, p, 0,
         dev(mask) if drop else None, None)
    pooled, out = take(pooled, n, (B, NF, NP), "pooled"), take(out, n, (B, NF * NP), "out")
    if mode == "exact" and win & (win - 1) == 0:
        assert_exact(float(mp.max()) * win, 1.0 / 4, "pooled")
        same(pooled, rp, "pooled")
    elif mode == "exact":
        within(pooled, rp, gamma(1) * mp, "pooled")               # an exact sum, one division
    else:
        # per term: the affine (fma: 1, bounded by 2) and the square accumulated by fma; win terms; the division
        within(pooled, rp, gamma(win + 2 * 2 + 1) * mp, "pooled")
    # out against the float64 log of the kernel's own mean; the dropout scale is 2: no further rounding
    ro = R.sqpool_log_out_ref(pooled, lo, hi, p, mask)
    within(out, ro, 2 * LOGF_ULP * ulp32(ro), "out")
    if drop:
        assert ((out == 0) == (mask.view(B, -1) == 0) | (ro == 0)).all()


@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "mask"])
def test_sqpool_log_fwd_propagates_a_nan_mean(drop):
    """torch.clamp hands a NaN through; so does the head: the mean, its logarithm and the dropped logarithm are NaN."""
    B, T, NF, NP, win, stride = 2, 40, 40, 5, 8, 7
    v, bn = pool_data("exact", seed_of("poolnan"), B, T, NF)
    v[0, 9, 3] = float("nan")                                      # token 9 lies in windows 1 (7..14) only
    v[1, 14, 7] = float("nan")                                     # token 14 lies in windows 1 and 2
    p = 0.5 if drop else 0.0
    mask = keep_mask(seed_of("poolnan") + 1, (B, NF, NP), p) if drop else None
    if drop:
        mask[0, 3, 1], mask[1, 7, 1], mask[1, 7, 2] = 0, 1, 0
    n = B * NF * NP
    pooled, out = dev(torch.zeros(n)), dev(torch.zeros(n))
    call("eav_sqpool_log_fwd", dev(v), dev(bn), pooled, out, B, T, NF, NP, win, stride, 1e-7, 1e4, p, 0,
         dev(mask) if drop else None, None)
    torch.cuda.synchronize()
    pooled, out = pooled.cpu().view(B, NF, NP), out.cpu().view(B, NF, NP)
    rp = R.sqpool_ref(v, bn, NP, win, stride)[0]
    same(pooled, rp, "pooled")
    want = torch.zeros(B, NF, NP, dtype=torch.bool)
    want[0, 3, 1] = want[1, 7, 1] = want[1, 7, 2] = True
    assert torch.equal(torch.isnan(pooled), want) and torch.equal(torch.isnan(out), want)
    ro = R.sqpool_log_out_ref(pooled, float(np.float32(1e-7)), 1e4, p, mask).view(B, NF, NP)
    ok = ~want
    within(out[ok], ro[ok], 2 * LOGF_ULP * ulp32(ro[ok]), "out")


@pytest.mark.parametrize("mode", ["exact", "rounded"])
@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "mask"])
@pytest.mark.parametrize("B,T,NF,NP,win,stride", POOL, ids=POOL_IDS)
def test_sqpool_log_bwd(B, T, NF, NP, win, stride, drop, mode):
    """pooled is an input here: the reference means rounded to fp32, with lo and hi two of those values, so that means lie
    below lo, exactly on lo, inside, exactly on hi and above hi.  The quotients dy / pooled round: g and the sums are held
    to the rounded bound in both modes."""
    seed = seed_of("poolbwd", B, T, NF, NP, win, stride, drop, mode)
    v, bn = pool_data(mode, seed, B, T, NF)
    pooled = R.sqpool_ref(v, bn, NP, win, stride)[0].float()
    pooled[pooled == 0] = 0.25                                     # (an all-zero window: keep the quotient finite)
    lo, hi = clamp_bounds(pooled)
    if len(pooled.unique()) > 4:
        assert (pooled < lo).any() and (pooled == lo).any() and (pooled == hi).any() and (pooled > hi).any()
    p = 0.5 if drop else 0.0
    mask = keep_mask(seed + 9, (B, NF, NP), p) if drop else None
    dy = ints(seed + 5, (B, NF * NP), -3, 3) if mode == "exact" else normal(seed + 5, (B, NF * NP))
    g, part = sentinel_buf(B * T * NF), sentinel_buf(B * 2 * NF)
    call("eav_sqpool_log_bwd", dev(dy), dev(pooled), dev(v), dev(bn), g, part, B, T, NF, NP, win, stride, lo, hi, p, 0,
         dev(mask) if drop else None, None)
    g, part = take(g, B * T * NF, (B, T, NF), "g"), take(part, B * 2 * NF, (B, 2 * NF), "part")
    r = R.sqpool_log_bwd_ref(dy, pooled, v, bn, NP, win, stride, lo, hi, p, mask)
    assert (g[:, (NP - 1) * stride + win:] == 0).all(), "tail tokens"
    # a token lies in nwin windows; per term the quotient (1), then 2/win (its rounding and the product: 2), the affine
    # (2), the final product (1); the dropout scale 2 is exact
    nwin = cdiv(win, stride)
    within(g, r["g"], gamma(nwin + 6) * r["g_mag"], "g")
    tol = torch.cat([gamma(nwin + 6 + T) * r["part_mag"][:, :NF], gamma(nwin + 6 + 3 + T) * r["part_mag"][:, NF:]], 1)
    within(part, r["part"], tol, "part")                            # xhat: a subtraction and two products more


# ====================================================================================================== eav_bn_rows_bwd
# (M, NF): the last is the video stem's BatchNorm rows (B 112 112 pixels of 64 channels) at B = 6, past one grid pass
BN_ROWS = [(1, 1), (300, 40), (50, 2048), (6 * 112 * 112, 64)]


@pytest.mark.parametrize("mode", ["exact", "rounded"])
@pytest.mark.parametrize("M,NF", BN_ROWS, ids=[f"M{m}-NF{f}{'-wraps' if m * f > GRID_CAP else ''}" for m, f in BN_ROWS])
def test_bn_rows_bwd(M, NF, mode):
    seed = seed_of("bnrows", M, NF, mode)
    if mode == "exact":
        g, v = ints(seed, (M, NF), -3, 3), ints(seed + 1, (M, NF), -3, 3)
        bn = torch.stack([pick(seed + 2, (NF,), [-1, 0, 1]), pick(seed + 3, (NF,), [0.5, 1, 2]),
                          pick(seed + 4, (NF,), [0.5, 1, 2, -1]), ints(seed + 5, (NF,), -2, 2),
                          pick(seed + 6, (NF,), [-1, 0, 1]), pick(seed + 7, (NF,), [0.5, 1, -0.5])])
    else:
        g, v = normal(seed, (M, NF)), normal(seed + 1, (M, NF))
        bn = torch.stack([normal(seed + 2, (NF,)), torch.from_numpy(synth.uniform(seed + 3, (NF,), 0.5, 2.0)),
                          normal(seed + 4, (NF,)), normal(seed + 5, (NF,)), normal(seed + 6, (NF,), 0.3),
                          normal(seed + 7, (NF,), 0.3)])
    dx = sentinel_buf(M * NF)
    call("eav_bn_rows_bwd", dev(g), dev(v), dev(bn), dx, M, NF)
    dx = take(dx, M * NF, (M, NF), "dx")
    ref, mag = R.bn_rows_bwd_ref(g, v, bn)
    if mode == "exact":
        same(dx, ref, "dx")                                         # every intermediate is a small multiple of 1/8
    else:
        within(dx, ref, gamma(6) * mag, "dx")    # v - mean, * invstd, * m2, two subtractions, * scale


# ============================================================================================================= refusals
def test_past_a_documented_limit_is_refused_without_a_launch():
    from eav_amd import _lib
    b = [sentinel_buf(64) for _ in range(6)]
    P = [t.data_ptr() for t in b]
    bad = [("eav_shallow_embed_fwd", (P[0], P[1], P[2], 33, P[3], P[4], 1, 33, 64, 4, 4, None)),
           ("eav_shallow_embed_fwd", (P[0], P[1], P[2], 32, P[3], P[4], 1, 4, 64, 49, 4, None)),
           ("eav_shallow_embed_fwd", (P[0], P[1], P[2], 32, P[3], P[4], 1, 4, 64, 4, 17, None)),
           ("eav_shallow_embed_fwd", (P[0], P[1], P[2], 32, P[3], P[4], 1, 4, 3, 4, 4, None)),
           ("eav_shallow_embed_fwd", (P[0], P[1], P[2], 3, P[3], P[4], 1, 4, 64, 4, 4, None)),
           ("eav_shallow_embed_bwd", (P[0], P[1], P[2], P[3], P[4], P[5], 1, 33, 64, 4, 4, None)),
           ("eav_shallow_embed_bwd", (P[0], P[1], P[2], P[3], P[4], P[5], 1, 4, 64, 4, 17, None)),
           ("eav_relu_dropout", (P[0], 8, 1.0, 0, None, None, None)),
           ("eav_relu_dropout_bwd", (P[0], P[1], 8, 1.0, None)),
           ("eav_dropout_add", (P[0], None, P[1], 8, -0.5, 0, None, None, None)),
           ("eav_add_strided", (P[0], 3, None, 0, P[1], 8, 2, 4, None)),
           ("eav_colstats", (P[0], P[1], 4, 257, 257, None)),
           ("eav_colstats", (P[0], P[1], 4, 8, 7, None)),
           ("eav_sqpool_log_fwd", (P[0], P[1], P[2], P[3], 1, 16, 257, 2, 4, 4, 1e-7, 1e4, 0.0, 0, None, None, None)),
           ("eav_sqpool_log_fwd", (P[0], P[1], P[2], P[3], 1, 16, 4, 4, 5, 4, 1e-7, 1e4, 0.0, 0, None, None, None)),
           # NF * NP + 512 floats must fit 64 KB: 256 * 62 does, 256 * 63 does not
           ("eav_sqpool_log_fwd", (P[0], P[1], P[2], P[3], 1, 70, 256, 63, 8, 1, 1e-7, 1e4, 0.0, 0, None, None, None)),
           ("eav_sqpool_log_bwd", (P[0], P[1], P[2], P[3], P[4], P[5], 1, 70, 256, 63, 8, 1, 1e-7, 1e4, 0.0, 0, None,
                                   None, None)),
           ("eav_bn_rows_bwd", (P[0], P[1], P[2], P[3], 0, 4, None))]
    for name, args in bad:
        with pytest.raises(_lib.EavError, match=name) as err:
            _lib.call(name, *args)
        assert "failed (-" in str(err.value), name
    for t in b:
        assert (bits(t.cpu()) == SENT).all()
