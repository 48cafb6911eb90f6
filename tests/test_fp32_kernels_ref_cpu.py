"""The float64 references of tests/fp32_kernels_ref.py against independent statements of the same operations
(torch.nn.functional and autograd in double), the guarded allocator on the host, the tile forms the GPU cases are meant
to take (through the plan queries of the library, which need no device), and, for the input sets of
test_fp32_encoder_kernels_gpu.py, that the reference is finite and that its own fp32 rounding - the best any kernel can
do - stays within the bounds the GPU test applies."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from eav_amd import synth
from tests import fp32_kernels_ref as R


@pytest.fixture(scope="module")
def lib():
    from eav_amd import _lib
    _lib.load()
    return _lib


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(R.f64(a)))


def same(a, b, tol=1e-12):
    a, b = R.f64(a), R.f64(b)
    assert a.shape == b.shape
    assert np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max())


# ------------------------------------------------------------------------------------- references, pinned
def test_gemm_reference_matches_linear_and_autograd():
    M, N, K = 9, 7, 5
    a, b = synth.normal(1, (2, M, K)), synth.normal(2, (2, K, N))
    bias, resid, prev = synth.normal(3, (N,)), synth.normal(4, (2, M, N)), synth.normal(5, (2, M, N))
    out, pre, ab = R.gemm_ref(a, b, 0.5, bias, True, resid, prev)
    z = 0.5 * torch.matmul(t64(a), t64(b)) + t64(bias)
    same(pre, z.numpy())
    same(out, (F.gelu(z) + t64(resid) + t64(prev)).numpy())
    same(ab, (0.5 * torch.matmul(t64(a).abs(), t64(b).abs()) + t64(bias).abs() + t64(resid).abs() + t64(prev).abs()).numpy())
    # nn.Linear forward (A [M,K], B stored [N,K]) and its two gradients are the (0,0), (0,1) and (1,1) layouts
    x, w = t64(a[0]).requires_grad_(True), t64(b[0].T.copy()).requires_grad_(True)
    y = F.linear(x, w)
    same(R.gemm_ref(a[:1], b[:1])[0][0], y.detach().numpy())
    dy = synth.normal(6, (M, N))
    y.backward(t64(dy))
    same(R.gemm_ref(dy[None], b[0].T[None])[0][0], x.grad.numpy())            # dx = dy . W
    same(R.splitk_ref(dy.T, a[0])[0], w.grad.numpy())                        # dW = dy^T . x
    assert R.splitk_slice(16200, 64) == 256 and R.splitk_slice(4100, 17) == 256 and R.splitk_slice(700, 3) == 240


def test_gelu_and_its_derivative():
    z = t64(np.concatenate([synth.normal(7, (500,), 0, 3.0), [0.0, 12.0, -12.0, 1e-40]])).requires_grad_(True)
    g = F.gelu(z)
    same(R.gelu64(z.detach().numpy()), g.detach().numpy())
    g.backward(torch.ones_like(g))
    same(R.gelu_grad64(z.detach().numpy()), z.grad.numpy())
    d = synth.normal(8, (504,))
    same(R.gelu_bwd_ref(d, z.detach().numpy()), (t64(d) * z.grad).numpy())


def test_softmax_references():
    for N in (1, 65, 257):
        s = R.softmax_rows(N)
        st = t64(s).requires_grad_(True)
        p = torch.softmax(st, -1)
        same(R.softmax_ref(s), p.detach().numpy())
        dp = synth.normal(9, s.shape)
        p.backward(t64(dp))
        same(R.softmax_bwd_ref(p.detach().numpy(), dp), st.grad.numpy())


def test_layernorm_references():
    for M, D in ((5, 8), (7, 252)):
        x, g, b, dy, old, keep = R.layernorm_inputs(M, D)
        x = x.copy()
        x[1] = synth.normal(10, (D,))             # (autograd through a zero-variance row is not a reference of anything)
        xt, gt, bt = (t64(v).requires_grad_(True) for v in (x, g, b))
        y = F.layer_norm(xt, (D,), gt, bt, 1e-5)
        yr, mean, rstd = R.layernorm_fwd_ref(x, g, b, 1e-5)
        same(yr, y.detach().numpy())
        same(mean, R.f64(x).mean(-1))
        same(rstd, 1.0 / np.sqrt(R.f64(x).var(-1) + 1e-5))
        y.backward(t64(dy))
        dx, dg, db, adg, adb = R.layernorm_bwd_ref(dy, x, g, mean, rstd)
        same(dx, xt.grad.numpy(), 1e-10)
        same(dg, gt.grad.numpy(), 1e-10)
        same(db, bt.grad.numpy())
        assert (adg >= np.abs(dg) - 1e-12).all() and (adb >= np.abs(db) - 1e-12).all()


def test_colsum_im2col_references():
    dy = synth.normal(11, (37, 9))
    s, a = R.colsum_ref(dy)
    same(s, t64(dy).sum(0).numpy())
    same(a, t64(dy).abs().sum(0).numpy())
    for name, B, C, H, W, P, stride, tr in R.IM2COL_CASES[2:]:
        x = R.im2col_input(name, B, C, H, W, tr)
        img = torch.from_numpy(x).unsqueeze(1).transpose(2, 3) if tr else torch.from_numpy(x)
        ref = F.unfold(img, P, stride=stride).transpose(1, 2).reshape(-1, C * P * P)
        assert np.array_equal(R.im2col_ref(x, P, stride, stride, tr), ref.numpy())
    x = synth.normal(12, (2, 3, 32, 48))          # different strides along the two axes
    ref = F.unfold(torch.from_numpy(x), 16, stride=(8, 16)).transpose(1, 2).reshape(-1, 768)
    assert np.array_equal(R.im2col_ref(x, 16, 8, 16, 0), ref.numpy())


def test_embedding_token_rows_pair_mean_references():
    B, ntok, D = 3, 7, 8
    for nx in (1, 2):
        patches = t64(synth.normal(13, (B, ntok - nx, D))).requires_grad_(True)
        cls, dist, pos = (t64(synth.normal(14 + i, s)).requires_grad_(True) for i, s in enumerate(((D,), (D,), (ntok, D))))
        toks = [cls.expand(B, 1, D)] + ([dist.expand(B, 1, D)] if nx == 2 else [])
        h = torch.cat(toks + [patches], 1) + pos               # HF embeddings: cat(cls, [dist,] patches) + position
        h0 = np.zeros((B, ntok, D))
        h0[:, nx:] = patches.detach().numpy()
        same(R.embed_finish_ref(h0, cls.detach().numpy(), dist.detach().numpy(), pos.detach().numpy(), nx), h.detach().numpy())
        dh = synth.normal(17, (B, ntok, D))
        h.backward(t64(dh))
        dpos, apos, demb = R.embed_bwd_ref(dh, nx)
        same(dpos, pos.grad.numpy())
        same(demb, patches.grad.reshape(-1, D).numpy())
        assert (apos >= np.abs(dpos)).all()
        # token rows: gather, then scatter of other rows into the same places
        hh = h.detach().numpy()
        rows = R.token_rows_ref(hh, None, nx, 0)
        assert np.array_equal(rows, hh[:, :nx].reshape(B * nx, D))
        new = synth.normal(18, rows.shape).astype(np.float64)
        sc = R.token_rows_ref(hh, new, nx, 1)
        assert np.array_equal(sc[:, nx:], hh[:, nx:]) and np.array_equal(R.token_rows_ref(sc, None, nx, 0), new)
    seq = t64(synth.normal(19, (2 * B, 7))).requires_grad_(True)
    pooled = seq.view(B, 2, 7).mean(1)                        # HF AST: (cls + dist) / 2
    same(R.pair_mean_ref(seq.detach().numpy()), pooled.detach().numpy())
    dp = synth.normal(20, (B, 7))
    pooled.backward(t64(dp))
    same(R.pair_mean_bwd_ref(dp), seq.grad.numpy())


# ------------------------------------------------------------------------------------- allocator, layouts
def test_guarded_allocator_reports_stray_and_missing_writes():
    lay = R.Layout(4, 5, 3, 2 * 4 + 2, 2, 5 * 10 + 3, 4)
    assert lay.distinct()
    idx = lay.index()
    g = R.Guarded(lay.span(), "cpu", slack=7)
    assert g.buf.numel() == 2 * R.GUARD + lay.span() + 7 and g.buf.view(torch.int32).eq(R.SENT).all()
    with pytest.raises(AssertionError, match="never written"):
        g.check(idx, "empty")
    vals = synth.normal(21, idx.shape)
    g.fill(idx, vals)
    assert np.array_equal(R.bits(g.check(idx, "full")), R.bits(vals))
    for off in (-1, 3, int(idx.max()) + 1, lay.span() + 7 + R.GUARD - 1):   # band before, a pad column, bands after
        g.buf[R.GUARD + off] = 1.0
        with pytest.raises(AssertionError, match="outside the output"):
            g.check(idx, "stray")
        g.buf.view(torch.int32)[R.GUARD + off] = R.SENT
    g.buf.view(torch.int32)[R.GUARD + 3] = 0x7FC00000           # another NaN is not the sentinel: compared bit for bit
    with pytest.raises(AssertionError, match="outside the output"):
        g.check(idx, "nan")
    buf = R.store(lay, vals)
    assert np.array_equal(buf[idx], vals) and (np.delete(buf, idx.ravel()) == np.float32(R.BIG)).all()


def test_compare_modes():
    w = np.array([1.0, 2.0, 3.0])
    R.compare("exact", w.astype(np.float32), w, None, 3, "ok")
    with pytest.raises(AssertionError, match="bit-exact"):
        R.compare("exact", np.float32([1, 2, 3.0000002]), w, None, 3, "off by an ulp")
    R.compare("rounded", w * (1 + 14 * R.U), w, w, 3, "inside")
    for bad in (w * (1 + 16 * R.U), np.array([1.0, np.nan, 3.0])):
        with pytest.raises(AssertionError, match="beyond"):
            R.compare("rounded", bad, w, w, 3, "outside")


@pytest.mark.parametrize("M,N,Z,H,form", R.GEMM_BIG)
def test_gemm_operand_layouts(M, N, Z, H, form):
    for tA, tB in R.LAYOUTS:
        c = R.GemmCase("exact", M, N, 37, tA, tB, Z, H)
        for lay in (c.LA, c.LB, c.LC):
            assert lay.ld > lay.C and (Z == 1 or lay.distinct())
        for lay in (c.LA, c.LB):
            assert lay.ld % 4 == 0 and lay.sb % 4 == 0 and lay.sh % 4 == 0
        a = c.A[c.LA.index()]
        assert np.array_equal(a.transpose(0, 2, 1) if tA else a, c.a)
        b = c.B[c.LB.index()]
        assert np.array_equal(b if tB else b.transpose(0, 2, 1), c.b)
        assert (np.delete(c.A, c.LA.index().ravel()) == np.float32(R.BIG)).all()


# ------------------------------------------------------------------------------------- tile forms
def test_case_lists_take_the_forms_they_name(lib):
    plan = lambda *a: lib.plain("eav_gemm_f32_plan", *a)  # noqa: E731
    for M, N, Z, H, form in R.GEMM_BIG:
        assert plan(M, N, Z) == form, (M, N, Z)
        assert form // 1000 == 128
        # close to the threshold: two row tiles (or one image) fewer fall back to 64-row tiles
        assert plan(M - 256, N, Z) // 1000 == 64 if Z == 1 else plan(M, N, Z - 1) // 1000 == 64
    for M, N, K, form in R.GEMM_SMALL + R.EPILOGUE_SHAPES:
        assert plan(M, N, 1) == form, (M, N)
    assert R.gemm_instances() == {(bm, bn, tA, tB) for bm in (64, 128) for bn in (64, 128) for tA, tB in R.LAYOUTS}
    reduces = set()
    for M, N, K, nz, form, red in R.SPLITK_CASES:
        ns = lib.plain("eav_gemm_f32_splitk_plan", M, N, K)
        assert lib.plain("eav_gemm_f32_splitk_nz", M, N, K) == nz == R.cdiv(K, R.splitk_slice(K, ns)) <= ns
        assert plan(M, N, nz) == form and lib.plain("eav_gemm_f32_splitk_reduce", M, N, K) == red
        assert (red == 2) == (nz >= 16 and M * N <= 1 << 18)
        reduces.add(red)
    assert reduces == {1, 2}
    assert 16200 % 256 == 72 and 72 % 16 == 8 and 17 % 8 != 0
    assert lib.plain("eav_gemm_f32_splitk_reduce", 8, 8, 64) == 0 and lib.plain("eav_gemm_f32_splitk_nz", 8, 8, 64) == 1
    assert plan(0, 5, 1) == 0
    # the query is the launcher's own rule: the documented thresholds
    assert plan(9712, 3072, 1) == 128128 and plan(9712, 768, 1) == 64128 and plan(40, 160, 64) == 64128
    assert plan(65, 64, 10000) == 128064 and plan(64, 64, 10000) == 64064 and plan(65, 65, 10000) == 128128
    assert {R.softmax_instance(n) for n in R.SOFTMAX_N} == {4, 20, 32}
    assert [R.softmax_instance(n) for n in (256, 257, 1280, 1281)] == [4, 20, 20, 32]
    assert lib.plain("eav_layernorm_bwd_nparts", 32789) == 512 and 4 * 512 * 16 == 32768 and 32789 - 32784 == 5


# ------------------------------------------------------------------------------------- input sets and bounds
def _best_case(mode, ref, ab, n, what, c=R.C_EPI):
    """The reference is finite and its own fp32 rounding passes the comparison the GPU test applies."""
    assert np.isfinite(ref).all() and np.isfinite(ab).all(), what
    assert (ab >= np.abs(ref) * (1 - 1e-12)).all(), what
    R.compare(mode, ref.astype(np.float32), ref, ab, n, what, c)


@pytest.mark.parametrize("mode", ["exact", "rounded"])
def test_gemm_input_sets(mode):
    for M, N, Z, H, form in R.GEMM_BIG:
        for K in R.GEMM_BIG_K:
            c = R.GemmCase(mode, M, N, K, 0, 0, Z, H)
            ref, _, ab = R.gemm_ref(c.a, c.b, 0.5)
            _best_case(mode, ref, ab, K, (M, N, K))
            # a plain fp32 product (another summation order) meets the same comparison
            R.compare(mode, 0.5 * np.matmul(c.a, c.b), ref, ab, K, (M, N, K, "sgemm"))
    for M, N, K, form in R.GEMM_SMALL:
        c = R.GemmCase(mode, M, N, K, 1, 0)
        ref, _, ab = R.gemm_ref(c.a, c.b, 0.5)
        _best_case(mode, ref, ab, K, (M, N, K))
    M, N, K, _ = R.EPILOGUE_SHAPES[-1]
    for name, alpha, bias, gelu, pre, resid, acc in R.EPILOGUES:
        c = R.GemmCase(mode, M, N, K, 0, 0, seed=name)
        bi = R.data(mode, 1, (N,)) if bias else None
        rs = R.data(mode, 2, (1, M, N)) if resid else None
        pv = R.data(mode, 3, (1, M, N)) if acc else None
        out, z, ab = R.gemm_ref(c.a, c.b, alpha, bi, gelu, rs, pv)
        assert np.isfinite(out).all()
        if not gelu:
            _best_case(mode, out, ab, K, name)
        else:
            R.close(out.astype(np.float32), R.gelu64(z), 1e-5, 2e-5, name)
    for M, N, K, nz, form, red in R.SPLITK_CASES[1:]:
        a, b = R.data(mode, 4, (M, K)), R.data(mode, 5, (K, N))
        ref, ab = R.splitk_ref(a, b)
        _best_case(mode, ref, ab, R.splitk_slice(K, nz), (M, N, K))
        assert np.abs(ref).max() < 2 ** 24


def test_exact_mode_stays_below_2_24():
    """|sum| <= 16 K for operands in [-4, 4]: the longest contraction (16 200) leaves every partial sum an fp32 integer."""
    assert 16 * 16200 + 8 < 2 ** 24
    a = R.ints(1, (100000,))
    assert a.min() == -4 and a.max() == 4 and (a == np.round(a)).all()


def test_row_kernel_input_sets():
    for N in R.SOFTMAX_N:
        s = R.softmax_rows(N)
        assert s.shape == (R.SOFTMAX_ROWS, N) and np.argmax(s[5]) == N - 1 and (s[4] == s[4, 0]).all()
        assert N == 1 or (s[3].max() == 80 and s[3].min() == -80)
        p = R.softmax_ref(s)
        assert np.isfinite(p).all() and np.abs(p.sum(-1) - 1).max() < 1e-12
        R.close(p.astype(np.float32), p, 1e-5, 1e-7, N)
        ds = R.softmax_bwd_ref(p.astype(np.float32), synth.normal(R.seed_of("softmax dp", N), s.shape))
        assert np.isfinite(ds).all()
        R.close(ds.astype(np.float32), ds, 1e-4, 1e-7, N)
    for M, D in R.LN_SHAPES:
        x, g, b, dy, old, keep = R.layernorm_inputs(M, D)
        y, mean, rstd = R.layernorm_fwd_ref(x, g, b, R.LN_EPS)
        assert np.isfinite(y).all() and np.isfinite(rstd).all()
        m32, r32 = mean.astype(np.float32), rstd.astype(np.float32)
        dx, dg, db, adg, adb = R.layernorm_bwd_ref(dy, x, g, m32, r32)
        assert np.isfinite(dx).all()
        R.close(y.astype(np.float32)[keep], y[keep], 1e-4, 2e-5, (M, D))
        R.close((dx + old).astype(np.float32)[keep], (dx + old)[keep], 1e-3, 1e-4, (M, D))
        _best_case("rounded", dg, adg, M, (M, D, "dgamma"))
        _best_case("rounded", db, adb, M, (M, D, "dbeta"))
    for n in R.GELU_N[:2]:
        pre, d = R.gelu_inputs(n)
        ref = R.gelu_bwd_ref(d, pre)
        assert np.isfinite(ref).all() and {0.0, 12.0, -12.0} <= set(pre.tolist()) and 0 < pre[3] < 1.2e-38
        R.close(ref.astype(np.float32), ref, 1e-5, 1e-6, n)
    assert R.GELU_N[2] // 4 > 4096 * 256 and R.GELU_N[2] // 4 < 2 * 4096 * 256
    for M, N, ld in R.COLSUM_SHAPES:
        assert ld >= N
        for mode in ("exact", "rounded"):
            s, a = R.colsum_ref(R.data(mode, R.seed_of("colsum", M, N), (M, N)))
            _best_case(mode, s, a, 256, (M, N), 0)


def test_looped_kernels_make_a_second_pass():
    """grid_for() caps the grid at 4096 blocks of 256: the sizes that give some thread a second item."""
    cap = 4096 * 256
    name, B, C, H, W, P, s, tr = R.IM2COL_CASES[0]
    assert B * ((H - P) // s + 1) * ((W - P) // s + 1) * C * P * P > cap
    name, B, C, H, W, P, s, tr = R.IM2COL_CASES[1]
    assert B * ((H - P) // s + 1) * ((W - P) // s + 1) * C * P * P > cap
    for name, B, C, H, W, P, s, tr in R.IM2COL_CASES[2:]:
        assert (H - P) % s != 0 and (W - P) % s != 0
    B, ntok, D, nx = R.EMBED_CASES[2]
    assert B * ntok * D // 4 > cap
    B, ntok, D, nx = R.EMBED_CASES[3]
    assert ntok * D // 4 > cap
    B, ntok, D, nx = R.TOKEN_CASES[-1]
    assert B * nx * D // 4 > cap
    B, D = R.PAIR_CASES[-1]
    assert B * D > cap and D % 4 != 0
