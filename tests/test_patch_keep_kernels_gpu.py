"""The five kernels of csrc/patch_keep.hip through the C ABI against the numpy restatements of tests/patch_keep_ref.py:
the plan and its inverse by integer equality (hash keys at every grid size the encoder can meet, explicit keys with ties
planted at the K-th place), the three gather kernels bit for bit against their plain twins' gathered outputs, the position
gradient against float64.  Every output sits between sentinel bands that are compared after the launch."""
import numpy as np
import pytest
import torch

from eav_amd import synth
from tests import patch_keep_ref as R

pytestmark = pytest.mark.gpu

BAND = 256


@pytest.fixture(scope="module")
def L():
    import gc
    from eav_amd import _lib
    _lib.load()
    yield _lib
    gc.collect()


class Banded:
    """A contiguous device tensor of `shape` between two sentinel bands (NaN / -7777)."""

    def __init__(self, shape, dtype=torch.float32):
        n = int(np.prod(shape))
        self.fill = float("nan") if dtype == torch.float32 else -7777
        self.whole = torch.full((n + 2 * BAND,), self.fill, dtype=dtype, device="cuda")
        self.t = self.whole[BAND:BAND + n].view(*shape)
        assert self.t.data_ptr() % 16 == 0

    def ptr(self):
        return self.t.data_ptr()

    def host(self, what):
        torch.cuda.synchronize()
        w = self.whole.cpu().numpy()
        bands = np.concatenate([w[:BAND], w[-BAND:]])
        ok = np.isnan(bands).all() if self.whole.dtype == torch.float32 else (bands == self.fill).all()
        assert ok, what + ": wrote outside its output"
        return self.t.cpu().numpy()


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def counter(v):
    return torch.tensor(int(v), dtype=torch.int64, device="cuda")


def run_plan(L, B, P, K, seed, cnt=None, keys=None):
    keep, inv = Banded((B, K), torch.int32), Banded((B, P), torch.int32)
    c = None if cnt is None else counter(cnt)
    k = None if keys is None else torch.from_numpy(np.ascontiguousarray(keys, np.uint32).view(np.int32)).cuda()
    L.call("eav_patch_keep_plan", keep.ptr(), inv.ptr(), B, P, K, seed, None if c is None else c.data_ptr(),
           None if k is None else k.data_ptr(), None)
    what = f"plan B={B} P={P} K={K}"
    return keep.host(what + " keep"), inv.host(what + " inv")


# ============================================================================================ plan
@pytest.mark.parametrize("cnt", R.PLAN_COUNTERS)
@pytest.mark.parametrize("B,P,K", R.PLAN_CASES)
def test_plan_equals_the_restatement(L, B, P, K, cnt):
    seed = R.plan_seed(4242 + P)
    keep, inv = run_plan(L, B, P, K, seed, cnt)
    want_keep, want_inv = R.plan(B, P, K, seed, cnt)
    assert np.array_equal(keep, want_keep) and np.array_equal(inv, want_inv)
    again, _ = run_plan(L, B, P, K, seed, cnt)
    assert np.array_equal(keep, again)                                  # the same bits on every run
    if K < P and P > 2:
        other, _ = run_plan(L, B, P, K, seed, cnt + 1)
        assert not np.array_equal(keep, other)                          # another counter, another subset
    # no counter: the seed itself
    keep0, _ = run_plan(L, B, P, K, seed)
    assert np.array_equal(keep0, R.plan(B, P, K, seed)[0])


@pytest.mark.parametrize("P,K", [(3, 1), (10, 4), (300, 150), (1212, 606), (2046, 1023), (2046, 2044)])
def test_plan_breaks_ties_by_the_patch_index(L, P, K):
    for name, keys, want in R.tie_cases(P, K):
        keys3 = np.concatenate([keys, keys[:, ::-1], keys], 0)          # three samples: the middle one sees the reverse
        keep, inv = run_plan(L, 3, P, K, 0, keys=keys3)
        rk, ri = R.plan(3, P, K, 0, keys=keys3)
        assert np.array_equal(keep[0], want) and np.array_equal(keep[2], want), (name, P, K)
        assert np.array_equal(keep, rk) and np.array_equal(inv, ri), (name, P, K)
    keys = np.array([[0xFFFFFFFF, 0, 0xFFFFFFFF, 1]], np.uint32)          # the largest key is a key like any other
    assert np.array_equal(run_plan(L, 1, 4, 3, 0, keys=keys)[0], [[0, 1, 3]])


@pytest.mark.parametrize("B,P,K", R.PLAN_CASES)
def test_invert_equals_the_plans_inverse(L, B, P, K):
    keep, inv = R.plan(B, P, K, R.plan_seed(7), 9)
    out = Banded((B, P), torch.int32)
    kd = dev(keep, np.int32)
    L.call("eav_patch_keep_invert", kd.data_ptr(), out.ptr(), B, P, K, None)
    assert np.array_equal(out.host(f"invert {B} {P} {K}"), inv)


def test_plan_refuses_bad_sizes(L):
    k = torch.zeros(8, dtype=torch.int32, device="cuda")
    for B, P, K in ((0, 4, 2), (1, 4, 0), (1, 4, 5), (1, 2048, 4)):
        with pytest.raises(L.EavError):
            L.call("eav_patch_keep_plan", k.data_ptr(), k.data_ptr(), B, P, K, 0, None, None, None)
        with pytest.raises(L.EavError):
            L.call("eav_patch_keep_invert", k.data_ptr(), k.data_ptr(), B, P, K, None)


# ============================================================================================ gather kernels
def tables(B, P, seed):
    """Keep tables of a P-patch grid: K = 1 (first / last patch), a half with first and last forced in, K = P."""
    out = [np.tile([[0]], (B, 1)), np.tile([[P - 1]], (B, 1)), np.tile(np.arange(P), (B, 1))]
    if P > 2:
        K = max(2, P // 2)
        half = R.plan(B, P, K, seed, 1)[0]
        half[0, 0], half[0, -1] = 0, P - 1                       # (ascending and unique still: they are the extremes)
        out.append(half)
    return [np.ascontiguousarray(t, np.int32) for t in out]


# (B, C, H, W, patch, stride, transposed): the AST layout, 36 x 40 input in a 3 x 3 grid of overlapping patches, and ViT's 2 x 2
IM2COL = [(2, 1, 36, 40, 16, 10, 1), (2, 3, 32, 32, 16, 16, 0)]


@pytest.mark.parametrize("B,C,H,W,Pp,stride,tr", IM2COL)
def test_im2col_keep_gathers_im2cols_rows(L, B, C, H, W, Pp, stride, tr):
    ny, nx = (H - Pp) // stride + 1, (W - Pp) // stride + 1
    P, KP = ny * nx, C * Pp * Pp
    x = dev(synth.normal(500 + C, (B, W, H) if tr else (B, C, H, W)))
    full = Banded((B * P, KP))
    L.call("eav_im2col", x.data_ptr(), full.ptr(), B, C, H, W, Pp, stride, stride, tr, None)
    full_h = full.host("im2col").reshape(B, P, KP)
    for keep in tables(B, P, 11):
        K = keep.shape[1]
        col = Banded((B * K, KP))
        kd = dev(keep, np.int32)
        L.call("eav_im2col_keep", x.data_ptr(), col.ptr(), kd.data_ptr(), B, C, H, W, Pp, stride, stride, tr, K, None)
        got = col.host(f"im2col_keep K={K}").reshape(B, K, KP)
        assert np.array_equal(bits(got), bits(R.gather_rows(full_h, keep))), (K, tr)
        if K == P:
            assert np.array_equal(bits(got), bits(full_h))                # keep = arange: the plain twin's bits


@pytest.mark.parametrize("nextra", [1, 2])
@pytest.mark.parametrize("D", [64, 772])                                    # 772: 193 float4 lanes, no multiple of the block
def test_embed_finish_keep_gathers_embed_finish(L, D, nextra):
    B, P = 3, 9
    proj = synth.normal(600 + D, (B, P, D))                               # the projected patches of the full grid
    cls, dist, pos = synth.normal(601, (D,)), synth.normal(602, (D,)), synth.normal(603 + D, (nextra + P, D))
    pos[nextra + 4, 1] = -0.0
    cd, dd, pd = dev(cls), dev(dist), dev(pos)
    hfull = Banded((B, nextra + P, D))
    hfull.t[:, nextra:] = dev(proj)
    L.call("eav_embed_finish", hfull.ptr(), cd.data_ptr(), dd.data_ptr() if nextra == 2 else None, pd.data_ptr(), B,
           nextra + P, D, nextra, None)
    full_h = hfull.host("embed_finish")
    for keep in tables(B, P, 12):
        K = keep.shape[1]
        h = Banded((B, nextra + K, D))
        h.t[:, nextra:] = dev(R.gather_rows(proj, keep))
        kd = dev(keep, np.int32)
        L.call("eav_embed_finish_keep", h.ptr(), cd.data_ptr(), dd.data_ptr() if nextra == 2 else None, pd.data_ptr(),
               kd.data_ptr(), B, K, D, nextra, None)
        got = h.host(f"embed_finish_keep K={K}")
        want = np.concatenate([full_h[:, :nextra], R.gather_rows(full_h[:, nextra:], keep)], 1)
        assert np.array_equal(bits(got), bits(want)), (K, D, nextra)
        ref = R.embed_finish_keep_ref(np.concatenate([np.zeros((B, nextra, D), np.float32), R.gather_rows(proj, keep)], 1),
                                      cls, dist, pos, keep, nextra)
        assert np.array_equal(got.astype(np.float64), ref.astype(np.float32).astype(np.float64))     # one rounded add
        if K == P:
            assert np.array_equal(bits(got), bits(full_h))


@pytest.mark.parametrize("nextra", [1, 2])
@pytest.mark.parametrize("D", [64, 772])
@pytest.mark.parametrize("B", [1, 3])
def test_embed_bwd_keep_against_float64(L, B, D, nextra):
    """Per element within B 2^-24 sum|dh| of its terms; a position every sample kept, one nobody kept (no set bit), every
    element of both outputs written, two runs bit-equal."""
    P, K = 9, 4
    keep = R.plan(B, P, K, R.plan_seed(13), 2)[0]
    everyone, nobody = 3, 6
    for b in range(B):
        row = [p for p in keep[b] if p not in (everyone, nobody)][:K - 1] + [everyone]
        keep[b] = sorted(row + [p for p in range(P) if p not in row and p != nobody][:K - len(row)])
    inv = R.invert(keep, P)
    assert (inv[:, everyone] >= 0).all() and (inv[:, nobody] < 0).all()
    dh = synth.normal(700 + D + B, (B, nextra + K, D))
    dh[0, nextra, 0] = -0.0
    dhd, invd = dev(dh), dev(inv, np.int32)
    runs = []
    for _ in range(2):
        dpos, demb = Banded((nextra + P, D)), Banded((B * K, D))
        L.call("eav_embed_bwd_keep", dhd.data_ptr(), dpos.ptr(), demb.ptr(), invd.data_ptr(), B, P, K, D, nextra, None)
        runs.append((dpos.host("dpos"), demb.host("demb")))
    (gpos, gemb), (gpos2, gemb2) = runs
    assert np.isfinite(gpos).all() and np.isfinite(gemb).all(), "an output element was not written"
    assert np.array_equal(bits(gpos), bits(gpos2)) and np.array_equal(bits(gemb), bits(gemb2))
    ref, mag, emb = R.embed_bwd_keep_ref(dh, inv, nextra)
    err = np.abs(gpos.astype(np.float64) - ref)
    assert (err <= B * 2.0 ** -24 * mag).all(), float((err - B * 2.0 ** -24 * mag).max())
    assert not bits(gpos[nextra + nobody]).any()                           # +0.0, every bit
    assert np.array_equal(bits(gemb), bits(emb.astype(np.float32)))
    # the plain twin with keep = arange
    full = synth.normal(710 + D + B, (B, nextra + P, D))
    fd, ident = dev(full), dev(np.tile(np.arange(P), (B, 1)), np.int32)
    a, b = (Banded((nextra + P, D)), Banded((B * P, D))), (Banded((nextra + P, D)), Banded((B * P, D)))
    L.call("eav_embed_bwd", fd.data_ptr(), a[0].ptr(), a[1].ptr(), B, nextra + P, D, nextra, None)
    L.call("eav_embed_bwd_keep", fd.data_ptr(), b[0].ptr(), b[1].ptr(), ident.data_ptr(), B, P, P, D, nextra, None)
    for u, v, what in zip(a, b, ("dpos", "demb")):
        assert np.array_equal(bits(u.host(what)), bits(v.host(what))), what
