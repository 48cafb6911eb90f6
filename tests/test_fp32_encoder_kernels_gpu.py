"""Per-kernel parity of eav_gemm_f32 / eav_gemm_f32_splitk (csrc/gemm_f32.hip) and of the encoder's row-wise and
element-wise kernels (csrc/tf_kernels.hip), through the C ABI, against the float64 references of
tests/fp32_kernels_ref.py, at the tile forms, instantiations, loop passes and direction flags the older kernel tests do
not reach.

Every GEMM case first asserts, through eav_gemm_f32_plan (and the split-K queries), the tile form and reduce kernel it
is meant to run.  Contractions run in two data modes (fp32_kernels_ref.py): "exact" must equal the float64 result bit for
bit, "rounded" is held to (n + 12) 2^-24 sum|terms| per element.  Every output lives in a guarded buffer: the bands
before and after it, its pad columns and the gaps between batch slabs hold a NaN sentinel and are compared bit for bit
after the launch; operand pads hold 3e30, so a read past an edge shows in the result."""
import numpy as np
import pytest
import torch

from eav_amd import synth
from tests import fp32_kernels_ref as R

pytestmark = pytest.mark.gpu

MODES = ["exact", "rounded"]


@pytest.fixture(scope="module")
def L():
    import gc
    from eav_amd import _lib
    _lib.load()
    yield _lib
    gc.collect()                 # nothing of this module's device memory outlives it


def dev(a):
    """Host array -> device tensor.  The callers hold it in a local until a Guarded.check (which synchronises)."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def P(t):
    return None if t is None else t.data_ptr()


def guarded(n, slack=0):
    return R.Guarded(n, "cuda", slack)


def same_bits(got, want, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ne = R.bits(got) != R.bits(want)
    assert not ne.any(), f"{what}: {int(ne.sum())} of {ne.size} words differ"


# --------------------------------------------------------------------------------------------------- GEMM
def run_gemm(L, c, form, alpha=1.0, bias=None, gelu=0, want_pre=False, resid=None, prev=None):
    """One eav_gemm_f32 call on the operands of GemmCase c; returns (C, pre) as [Z, M, N] after the guard checks."""
    assert L.plain("eav_gemm_f32_plan", c.M, c.N, c.Z) == form, "the shape no longer takes the tile form under test"
    A, B = dev(c.A), dev(c.B)
    idx = c.LC.index()
    slack = 128 * c.ldc                    # a full tile of rows past the last one stays inside the band
    C = guarded(c.LC.span(), slack)
    if prev is not None:
        C.fill(idx, prev)
    pre = guarded(c.LC.span(), slack) if want_pre else None
    bi = None if bias is None else dev(R.store(R.Layout(1, 1, c.N, c.N), bias))
    ldr = c.N + 5                          # != ldc = N + 3
    rs = None if resid is None else dev(R.store(R.Layout(1, c.M, c.N, ldr), resid))
    (sAb, sAh), (sBb, sBh), (sCb, sCh) = c.strides(c.LA), c.strides(c.LB), c.strides(c.LC)
    L.call("eav_gemm_f32", P(A), P(B), C.ptr(), c.M, c.N, c.K, c.lda, c.ldb, c.ldc, c.tA, c.tB, c.Z, c.H, sAb, sAh, sBb,
           sBh, sCb, sCh, alpha, P(bi), gelu, pre.ptr() if pre else None, P(rs), ldr if rs is not None else 0,
           1 if prev is not None else 0, None)
    what = f"{c.M}x{c.N}x{c.K} z{c.Z} t{c.tA}{c.tB} {c.mode}"
    return C.check(idx, "C " + what), (pre.check(idx, "pre " + what) if pre else None)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tA,tB", R.LAYOUTS)
@pytest.mark.parametrize("K", R.GEMM_BIG_K)
@pytest.mark.parametrize("M,N,Z,H,form", R.GEMM_BIG)
def test_gemm_128_row_tiles(L, M, N, Z, H, form, K, tA, tB, mode):
    c = R.GemmCase(mode, M, N, K, tA, tB, Z, H)
    got, _ = run_gemm(L, c, form, alpha=0.5)
    ref, _, ab = R.gemm_ref(c.a, c.b, 0.5)
    R.compare(mode, got, ref, ab, K, "C")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tA,tB", R.LAYOUTS)
@pytest.mark.parametrize("M,N,K,form", R.GEMM_SMALL)
def test_gemm_small_forms(L, M, N, K, form, tA, tB, mode):
    c = R.GemmCase(mode, M, N, K, tA, tB)
    got, _ = run_gemm(L, c, form, alpha=0.5)
    ref, _, ab = R.gemm_ref(c.a, c.b, 0.5)
    R.compare(mode, got, ref, ab, K, "C")


def check_epilogue(L, c, form, mode, name, alpha, bias, gelu, pre, resid, acc):
    sh = (c.Z, c.M, c.N)
    bi = R.data(mode, R.seed_of("bias", name), (c.N,)) if bias else None
    rs = R.data(mode, R.seed_of("resid", name), sh) if resid else None
    pv = R.data(mode, R.seed_of("prev", name), sh) if acc else None
    got, gpre = run_gemm(L, c, form, alpha, bi, gelu, bool(pre), rs, pv)
    out, z, ab = R.gemm_ref(c.a, c.b, alpha, bi, bool(gelu), rs, pv)
    if pre:
        R.compare(mode, gpre, z, ab, c.K, name + ": pre")
    if gelu:            # the activation itself is not exact in either mode: test_gemm_epilogues' bound at O(1) values
        R.close(got, R.gelu64(z), 1e-5, 2e-5, name + ": gelu")
    else:
        R.compare(mode, got, out, ab, c.K, name)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,alpha,bias,gelu,pre,resid,acc", R.EPILOGUES, ids=[e[0] for e in R.EPILOGUES])
@pytest.mark.parametrize("M,N,K,form", R.EPILOGUE_SHAPES)
def test_gemm_epilogue_options(L, M, N, K, form, name, alpha, bias, gelu, pre, resid, acc, mode):
    c = R.GemmCase(mode, M, N, K, 0, 0, seed=name)
    check_epilogue(L, c, form, mode, name, alpha, bias, gelu, pre, resid, acc)


@pytest.mark.parametrize("mode", MODES)
def test_gemm_epilogue_pre_and_bias_batched(L, mode):
    """`pre` follows ldc and the batch offsets of C; the bias is shared by the slabs."""
    M, N, Z, H, form = R.GEMM_BIG[3]
    c = R.GemmCase(mode, M, N, 37, 0, 1, Z, H, seed="batched pre")
    check_epilogue(L, c, form, mode, "bias_gelu_pre", 1.0, 1, 1, 1, 0, 0)


def test_gemm_refuses_a_batched_residual(L):
    c = R.GemmCase("exact", 8, 8, 4, 0, 0, 2, 1)
    A, B, C, rs = dev(c.A), dev(c.B), guarded(c.LC.span()), dev(np.zeros(64))
    with pytest.raises(L.EavError, match="not batched"):
        L.call("eav_gemm_f32", P(A), P(B), C.ptr(), 8, 8, 4, c.lda, c.ldb, c.ldc, 0, 0, 2, 1, c.LA.sb, 0, c.LB.sb, 0,
               c.LC.sb, 0, 1.0, None, 0, None, P(rs), 8, 0, None)
    C.check(np.zeros(0, np.int64), "refused call")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M,N,K,nz,form,red,tA,tB", [s + l for s in R.SPLITK_CASES for l in R.splitk_layouts(*s[:3])])
def test_gemm_splitk(L, M, N, K, nz, form, red, tA, tB, mode):
    ns = L.plain("eav_gemm_f32_splitk_plan", M, N, K)
    assert L.plain("eav_gemm_f32_splitk_nz", M, N, K) == nz <= ns and R.cdiv(K, R.splitk_slice(K, ns)) == nz
    assert L.plain("eav_gemm_f32_plan", M, N, nz) == form and L.plain("eav_gemm_f32_splitk_reduce", M, N, K) == red
    a, b = R.data(mode, R.seed_of("sk a", M, K), (M, K)), R.data(mode, R.seed_of("sk b", K, N), (K, N), 0.25)
    LA = R.Layout(1, K, M, R.pad4(M) + 4) if tA else R.Layout(1, M, K, R.pad4(K) + 4)
    LB = R.Layout(1, K, N, R.pad4(N) + 4) if tB else R.Layout(1, N, K, R.pad4(K) + 4)
    A, B = dev(R.store(LA, a.T if tA else a)), dev(R.store(LB, b if tB else b.T))
    ws = guarded(ns * M * N, 128 * N)
    outs = []
    for run in range(2):
        C = guarded(M * N, 128 * N)
        L.call("eav_gemm_f32_splitk", P(A), P(B), C.ptr(), ws.ptr(), M, N, K, LA.ld, LB.ld, tA, tB, None)
        outs.append(C.check(np.arange(M * N), f"C (run {run})").reshape(M, N))
        ws.check(np.arange(nz * M * N), "ws: the slabs of the slices that run, nothing beyond them")
    ref, ab = R.splitk_ref(a, b)
    R.compare(mode, outs[0], ref, ab, R.splitk_slice(K, ns), "split-K")
    same_bits(outs[1], outs[0], "second run")


# ------------------------------------------------------------------------------------------------ softmax
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("N", R.SOFTMAX_N)
def test_softmax_fwd_bwd(L, N, pad):
    rows, ld = R.SOFTMAX_ROWS, N + pad
    lay = R.Layout(1, rows, N, ld)
    idx = lay.index()[0]
    s = R.softmax_rows(N)
    S = guarded(lay.span())
    S.fill(idx, s)
    L.call("eav_softmax_fwd", S.ptr(), rows, N, ld, None)
    p = R.softmax_ref(s)
    R.close(S.check(idx, "softmax"), p, 1e-5, 1e-7, f"softmax N={N}")
    p32 = p.astype(np.float32)
    dp = synth.normal(R.seed_of("softmax dp", N), (rows, N))
    Pd = dev(R.store(lay, p32))
    D = guarded(lay.span())
    D.fill(idx, dp)
    L.call("eav_softmax_bwd", P(Pd), D.ptr(), rows, N, ld, None)
    R.close(D.check(idx, "softmax bwd"), R.softmax_bwd_ref(p32, dp), 1e-4, 1e-7, f"softmax bwd N={N}")


def test_softmax_refuses_rows_beyond_2048(L):
    S = guarded(2 * 2049)
    for fn, args in (("eav_softmax_fwd", (S.ptr(),)), ("eav_softmax_bwd", (S.ptr(), S.ptr()))):
        with pytest.raises(L.EavError, match="2048"):
            L.call(fn, *args, 2, 2049, 2049, None)
    S.check(np.zeros(0, np.int64), "refused call")


# ---------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("M,D", R.LN_SHAPES)
def test_layernorm_fwd_bwd(L, M, D):
    x, g, b, dy, old, keep = R.layernorm_inputs(M, D)
    X, G, Bt, DY = dev(x), dev(g), dev(b), dev(dy)
    y, st = guarded(M * D), guarded(2 * M)
    L.call("eav_layernorm_fwd", P(X), P(G), P(Bt), y.ptr(), st.ptr(), st.ptr(M), M, D, R.LN_EPS, None)
    yr, mean, rstd = R.layernorm_fwd_ref(x, g, b, R.LN_EPS)
    gy = y.check(np.arange(M * D), "y").reshape(M, D)
    gst = st.check(np.arange(2 * M), "mean / rstd").reshape(2, M)
    assert np.isfinite(gy).all() and np.isfinite(gst).all()
    R.close(gy[keep], yr[keep], 1e-4, 2e-5, "ln fwd")
    # mean: a sum of D terms and one division; rstd = (var + eps)^-1/2: half the relative error of var (a sum of D
    # non-negative terms, each with the 2 roundings of (x - mean)^2) plus the roundings of the division and the roots
    R.compare("rounded", gst[0][keep], mean[keep], np.abs(R.f64(x)).mean(-1)[keep], D, "mean")
    R.compare("rounded", gst[1][keep], rstd[keep], rstd[keep], D, "rstd")
    # backward from the fp32 rounding of the reference statistics: the kernel's inputs do not depend on the forward kernel
    m32, r32 = mean.astype(np.float32), rstd.astype(np.float32)
    MS, RS = dev(m32), dev(r32)
    npart = L.plain("eav_layernorm_bwd_nparts", M)
    dxr, dg, db, adg, adb = R.layernorm_bwd_ref(dy, x, g, m32, r32)
    # a partial is the sum of 4 waves' chains of at most `chain` rows each (+ 2 additions to combine them, 3 roundings
    # inside a dgamma term): covered by C_EPI
    chain = 16 * R.cdiv(M, 16 * 4 * npart)
    for acc in (0, 1):
        dx, part = guarded(M * D), guarded(npart * 2 * D)       # acc = 0: dx starts as the NaN sentinel
        if acc:
            dx.fill(np.arange(M * D), old)
        L.call("eav_layernorm_bwd", P(DY), P(X), P(G), P(MS), P(RS), dx.ptr(), acc, part.ptr(), M, D, None)
        gdx = dx.check(np.arange(M * D), f"dx (accumulate {acc})").reshape(M, D)
        assert np.isfinite(gdx).all()
        R.close(gdx[keep], (dxr + acc * R.f64(old))[keep], 1e-3, 1e-4, f"ln dx (accumulate {acc})")
        ps = R.f64(part.check(np.arange(npart * 2 * D), "partials")).reshape(npart, 2 * D).sum(0)
        R.compare("rounded", ps[:D], dg, adg, chain, "dgamma")
        R.compare("rounded", ps[D:], db, adb, chain, "dbeta")


@pytest.mark.parametrize("D", [6, 1028])
def test_layernorm_refuses_unsupported_widths(L, D):
    X, G, y, st = dev(np.zeros(2 * D)), dev(np.ones(D)), guarded(2 * D), guarded(4 + 4 * D)
    with pytest.raises(L.EavError, match="D <= 1024"):
        L.call("eav_layernorm_fwd", P(X), P(G), P(G), y.ptr(), st.ptr(), st.ptr(2), 2, D, R.LN_EPS, None)
    with pytest.raises(L.EavError, match="D <= 1024"):
        L.call("eav_layernorm_bwd", P(X), P(X), P(G), st.ptr(), st.ptr(2), y.ptr(), 0, st.ptr(4), 2, D, None)
    y.check(np.zeros(0, np.int64), "refused call")
    st.check(np.zeros(0, np.int64), "refused call")


# ---------------------------------------------------------------------------------- element-wise / row kernels
@pytest.mark.parametrize("n", R.GELU_N)
def test_gelu_bwd(L, n):
    pre, d = R.gelu_inputs(n)
    Pd, D = dev(pre), guarded(n)
    D.fill(np.arange(n), d)
    L.call("eav_gelu_bwd", D.ptr(), P(Pd), n, None)
    R.close(D.check(np.arange(n), "gelu bwd"), R.gelu_bwd_ref(d, pre), 1e-5, 1e-6, "gelu bwd")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M,N,ld", R.COLSUM_SHAPES)
def test_colsum(L, M, N, ld, mode):
    dy = R.data(mode, R.seed_of("colsum", M, N), (M, N))
    DY = dev(R.store(R.Layout(1, M, N, ld), dy, fill=1e30))
    npart = L.plain("eav_colsum_nparts", M)
    part = guarded(npart * N)
    L.call("eav_colsum", P(DY), part.ptr(), M, N, ld, None)
    got = R.f64(part.check(np.arange(npart * N), "partials")).reshape(npart, N).sum(0)
    s, a = R.colsum_ref(dy)
    R.compare(mode, got, s, a, 256, "colsum", c=0)          # a partial: 256 rows, fp32; the partials summed in float64


@pytest.mark.parametrize("name,B,C,H,W,Pp,stride,tr", R.IM2COL_CASES, ids=[c[0] for c in R.IM2COL_CASES])
def test_im2col(L, name, B, C, H, W, Pp, stride, tr):
    x = R.im2col_input(name, B, C, H, W, tr)
    ref = R.im2col_ref(x, Pp, stride, stride, tr)
    X, col = dev(x), guarded(ref.size)
    L.call("eav_im2col", P(X), col.ptr(), B, C, H, W, Pp, stride, stride, tr, None)
    same_bits(col.check(np.arange(ref.size), "col").reshape(ref.shape), ref, "im2col")


@pytest.mark.parametrize("B,ntok,D,nx", R.EMBED_CASES)
def test_embed_finish_and_bwd(L, B, ntok, D, nx):
    h = synth.normal(R.seed_of("embed h", B, ntok, D), (B, ntok, D))
    cls, dist, pos = (synth.normal(R.seed_of("embed", i, D), s) for i, s in enumerate(((D,), (D,), (ntok, D))))
    n = B * ntok * D
    H_, CL, DI, PO = guarded(n), dev(cls), dev(dist), dev(pos)
    H_.fill(np.arange(n), h)
    L.call("eav_embed_finish", H_.ptr(), P(CL), P(DI) if nx == 2 else None, P(PO), B, ntok, D, nx, None)
    ref = R.embed_finish_ref(h, cls, dist, pos, nx).astype(np.float32)
    same_bits(H_.check(np.arange(n), "h").reshape(h.shape), ref, "embed_finish")
    DH = dev(ref)
    dpos, demb = guarded(ntok * D), guarded(B * (ntok - nx) * D)
    L.call("eav_embed_bwd", P(DH), dpos.ptr(), demb.ptr(), B, ntok, D, nx, None)
    s, a, rows = R.embed_bwd_ref(ref, nx)
    same_bits(demb.check(np.arange(rows.size), "demb").reshape(rows.shape), rows, "demb")
    R.compare("rounded", dpos.check(np.arange(ntok * D), "dpos").reshape(ntok, D), s, a, B, "dpos", c=0)


@pytest.mark.parametrize("B,ntok,D,nx", R.TOKEN_CASES)
def test_token_rows_gather_and_scatter(L, B, ntok, D, nx):
    h = synth.normal(R.seed_of("token h", B, ntok, D), (B, ntok, D))
    Hd, rows = dev(h), guarded(B * nx * D)
    L.call("eav_token_rows", P(Hd), rows.ptr(), B, ntok, D, nx, 0, None)
    same_bits(rows.check(np.arange(B * nx * D), "rows").reshape(B * nx, D), R.token_rows_ref(h, None, nx, 0), "gather")
    new = synth.normal(R.seed_of("token rows", B, D), (B * nx, D))
    Hg, Rd = guarded(h.size), dev(new)
    Hg.fill(np.arange(h.size), h)
    L.call("eav_token_rows", Hg.ptr(), P(Rd), B, ntok, D, nx, 1, None)
    same_bits(Hg.check(np.arange(h.size), "h").reshape(h.shape), R.token_rows_ref(h, new, nx, 1), "scatter")
    assert torch.equal(Rd.cpu(), torch.from_numpy(new)), "scatter wrote its source"


@pytest.mark.parametrize("B,D", R.PAIR_CASES)
def test_pair_mean_forward_and_backward(L, B, D):
    seq = synth.normal(R.seed_of("pair", B, D), (2 * B, D))
    Sd, pooled = dev(seq), guarded(B * D)
    L.call("eav_pair_mean", P(Sd), pooled.ptr(), B, D, 0, None)
    got, ref = pooled.check(np.arange(B * D), "pooled").reshape(B, D), R.pair_mean_ref(seq)
    assert (np.abs(R.f64(got) - ref) <= np.spacing(np.abs(ref.astype(np.float32)))).all(), "pair mean beyond 1 ulp"
    dp = synth.normal(R.seed_of("pair d", B, D), (B, D))
    Pd, dseq = dev(dp), guarded(2 * B * D)
    L.call("eav_pair_mean", dseq.ptr(), P(Pd), B, D, 1, None)
    same_bits(dseq.check(np.arange(2 * B * D), "dseq").reshape(2 * B, D), R.pair_mean_bwd_ref(dp).astype(np.float32),
              "pair mean backward")
