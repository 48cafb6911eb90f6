"""Per-kernel parity of the video CNN kernels (csrc/video_cnn.hip, through the C ABI) against float64 torch.

Conv cases run in two data modes.  "exact": small integers, so that every fp32 product and partial sum is exact in any
order; the kernel must equal the float64 result bit for bit.  "rounded": synth normal data, held to gamma_n * sum|terms|
with n the number of terms of that output's sum.  MaxPool and the head pools carry planted ties and NaNs.

Every output is filled with a NaN sentinel and carries a guard band past its end: all of it must be overwritten, the
guard band must be untouched."""
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from eav_amd import synth

pytestmark = pytest.mark.gpu

SENT = 0x7FC0DEAD
GUARD = 4096
U = 2.0 ** -24


@pytest.fixture(scope="module", autouse=True)
def L():
    from eav_amd import _lib
    _lib.load()
    return _lib


_KEEP = []


def dev(a):
    t = (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).contiguous().cuda()
    _KEEP.append(t)
    if len(_KEEP) > 64:
        torch.cuda.synchronize()
        del _KEEP[:32]
    return t


def P(t):
    return None if t is None else t.data_ptr()


def st():
    return torch.cuda.current_stream().cuda_stream


def sentinel_buf(n, dtype=torch.float32):
    if dtype == torch.uint8:
        return dev(torch.full((n + GUARD,), 0xFF, dtype=torch.uint8))
    return dev(torch.full((n + GUARD,), SENT, dtype=torch.int32)).view(torch.float32)


def take(buf, n, shape, what):
    torch.cuda.synchronize()
    h = buf.cpu()
    bits = h if h.dtype == torch.uint8 else h.view(torch.int32)
    s = 0xFF if h.dtype == torch.uint8 else SENT
    unwritten = int((bits[:n] == s).sum())
    assert unwritten == 0, f"{what}: {unwritten} of {n} elements never written"
    assert (bits[n:] == s).all(), f"{what}: guard band written past the end"
    return h[:n].view(shape)


def seed_of(*case):
    return zlib.crc32(repr(case).encode())


def ints(seed, shape, lo, hi):
    n = int(np.prod(shape))
    return torch.from_numpy((lo + (synth.splitmix64(seed, n) % np.uint64(hi - lo + 1)).astype(np.int64))
                            .astype(np.float32).reshape(shape))


def data(mode, seed, shape):
    return ints(seed, shape, -3, 3) if mode == "exact" else torch.from_numpy(synth.normal(seed, shape, 0.0, 1.0))


def gamma(n):
    return n * U / (1 - n * U)


def compare(mode, got, want64, absref64, nterms, what):
    if mode == "exact":
        assert torch.equal(got.double(), want64), f"{what}: not bit-exact ({float((got.double() - want64).abs().max())})"
    else:
        err = (got.double() - want64).abs()
        bound = gamma(nterms + 2) * absref64 + 1e-30
        assert bool((err <= bound).all()), f"{what}: error {float(err.max()):.3e} beyond gamma_n sum|terms|"


# ResNet-50's non-GEMM conv geometries (Ci, Co, k, s, p) at reduced maps, plus ragged channels and odd sizes
GEOMS = [
    ("stem7x7s2", 3, 64, 7, 2, 3, 2, 30, 30),
    ("l1_3x3s1", 64, 64, 3, 1, 1, 2, 14, 14),
    ("l2_3x3s2", 128, 128, 3, 2, 1, 2, 14, 14),
    ("l2_3x3s1", 128, 128, 3, 1, 1, 1, 7, 7),
    ("l3_3x3s2", 256, 256, 3, 2, 1, 1, 8, 8),
    ("l3_3x3s1", 256, 256, 3, 1, 1, 2, 6, 6),
    ("l4_3x3s2", 512, 512, 3, 2, 1, 1, 7, 7),
    ("l4_3x3s1", 512, 512, 3, 1, 1, 2, 4, 4),
    ("ds2_1x1s2", 256, 512, 1, 2, 0, 2, 9, 9),
    ("ds3_1x1s2", 512, 1024, 1, 2, 0, 1, 7, 7),
    ("ds4_1x1s2", 1024, 2048, 1, 2, 0, 1, 5, 5),
    ("ragged_c", 24, 40, 3, 2, 1, 3, 11, 9),
    ("ragged_odd", 5, 7, 3, 2, 1, 1, 13, 7),
    ("b1_odd", 64, 72, 3, 2, 1, 1, 7, 5),
]


@pytest.mark.parametrize("mode", ["exact", "rounded"])
@pytest.mark.parametrize("geom", GEOMS, ids=[g[0] for g in GEOMS])
def test_conv_entry_points(geom, mode, L):
    name, Ci, Co, k, s, p, B, H, W = geom
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    sd = seed_of(geom, mode)
    x = data(mode, sd, (B, Ci, H, W))
    w = data(mode, sd + 1, (Co, Ci, k, k))
    dy = data(mode, sd + 2, (B, Co, OH, OW))
    x64, w64, dy64 = x.double().requires_grad_(True), w.double().requires_grad_(True), dy.double()
    y64 = F.conv2d(x64, w64, stride=s, padding=p)
    y64.backward(dy64)
    ya = F.conv2d(x.double().abs(), w.double().abs(), stride=s, padding=p)
    nchw = 1 if Ci == 3 else 0
    xd = dev(x if nchw else x.permute(0, 2, 3, 1))
    wd = dev(w)
    wf = sentinel_buf(w.numel())
    L.call("eav_video_conv_relayout", P(wd), P(wf), None, Co, Ci, k * k, st())
    wf_h = take(wf, w.numel(), (Co, k, k, Ci), "wf")
    assert torch.equal(wf_h, w.permute(0, 2, 3, 1))
    out = sentinel_buf(B * OH * OW * Co)
    L.call("eav_video_conv_fwd", P(xd), P(wf), P(out), B, Ci, H, W, Co, k, k, s, p, OH, OW, nchw, st())
    got = take(out, B * OH * OW * Co, (B, OH, OW, Co), "fwd").permute(0, 3, 1, 2)
    compare(mode, got, y64.detach(), ya, Ci * k * k, f"{name} fwd")

    # data gradient (NHWC input only) with the residual `add` operand
    if not nchw:
        wdg = sentinel_buf(w.numel())
        L.call("eav_video_conv_relayout", P(wd), None, P(wdg), Co, Ci, k * k, st())
        add = data(mode, sd + 3, (B, H, W, Ci))
        dyd = dev(dy.permute(0, 2, 3, 1))
        din = sentinel_buf(B * H * W * Ci)
        L.call("eav_video_conv_dgrad", P(dyd), P(wdg), P(dev(add)), P(din), B, Ci, H, W, Co, k, k, s, p, OH, OW, st())
        got = take(din, B * H * W * Ci, (B, H, W, Ci), "dgrad").permute(0, 3, 1, 2)
        want = x64.grad + add.double().permute(0, 3, 1, 2)
        xa = torch.nn.grad.conv2d_input(x.shape, w.double().abs(), dy64.abs(), stride=s, padding=p) + \
            add.double().abs().permute(0, 3, 1, 2)
        compare(mode, got, want, xa, Co * k * k + 1, f"{name} dgrad")

    # weight gradient: partials + the fixed-order reduction
    M = B * OH * OW
    n = L.plain("eav_video_wgrad_nparts", Co, Ci, k * k, M)
    part = sentinel_buf(n * Co * Ci * k * k)
    dyd = dev(dy.permute(0, 2, 3, 1))
    L.call("eav_video_conv_wgrad", P(dyd), P(xd), P(part), B, Ci, H, W, Co, k, k, s, p, OH, OW, nchw, n, st())
    take(part, n * Co * Ci * k * k, (n, Co, Ci, k, k), "wgrad partials")      # every [part][co][ci][tap] written
    gw = sentinel_buf(Co * Ci * k * k)
    L.call("eav_reduce_partials", P(part), n, Co * Ci * k * k, Co * Ci * k * k, 1.0, P(gw), st())
    got = take(gw, Co * Ci * k * k, (Co, Ci, k, k), "wgrad")
    wa = torch.nn.grad.conv2d_weight(x.double().abs(), w.shape, dy64.abs(), stride=s, padding=p)
    compare(mode, got, w64.grad, wa, M + n, f"{name} wgrad (nparts {n})")


def test_wgrad_many_parts_chunk_loop(L):
    """A small output-channel count with many output pixels: every part loops over several 32-pixel chunks."""
    B, Ci, Co, H, W = 4, 64, 64, 40, 40
    M = B * H * W
    n = L.plain("eav_video_wgrad_nparts", Co, Ci, 9, M)
    assert 1 < n < (M + 31) // 32, n
    x, dy = ints(1, (B, Ci, H, W), -2, 2), ints(2, (B, Co, H, W), -2, 2)
    part = sentinel_buf(n * Co * Ci * 9)
    L.call("eav_video_conv_wgrad", P(dev(dy.permute(0, 2, 3, 1))), P(dev(x.permute(0, 2, 3, 1))), P(part), B, Ci, H, W,
           Co, 3, 3, 1, 1, H, W, 0, n, st())
    take(part, n * Co * Ci * 9, (n, Co, Ci, 9), "wgrad partials")
    gw = sentinel_buf(Co * Ci * 9)
    L.call("eav_reduce_partials", P(part), n, Co * Ci * 9, Co * Ci * 9, 1.0, P(gw), st())
    got = take(gw, Co * Ci * 9, (Co, Ci, 3, 3), "wgrad")
    want = torch.nn.grad.conv2d_weight(x.double(), (Co, Ci, 3, 3), dy.double(), stride=1, padding=1)
    assert torch.equal(got.double(), want)


@pytest.mark.parametrize("C,M", [(2048, 98), (2048, 700), (64, 1000), (100, 300)])
def test_bn_stats_apply_bwd(C, M, L):
    x = torch.from_numpy(synth.normal(C + M, (M, C), 0.3, 1.0))
    res = torch.from_numpy(synth.normal(C + M + 1, (M, C), 0.0, 1.0))
    dy = torch.from_numpy(synth.normal(C + M + 2, (M, C), 0.0, 1.0))
    npart = L.plain("eav_video_bn_nparts", M)
    part = sentinel_buf(npart * 2 * C)
    xd = dev(x)
    L.call("eav_video_bn_stats", P(xd), P(part), M, C, st())
    pt = take(part, npart * 2 * C, (npart, 2, C), "stats").double()
    s64, q64 = x.double().sum(0), (x.double() ** 2).sum(0)
    # the (rounded sum, remainder) row pairs carry the fp64 chunk sums: far below fp32 resolution
    assert torch.allclose(pt[:, 0].sum(0), s64, rtol=1e-12, atol=1e-9)
    assert torch.allclose(pt[:, 1].sum(0), q64, rtol=1e-12, atol=1e-9)
    # apply with a BatchNorm'd residual and ReLU
    sc, sh = synth.uniform(1, (C,), 0.5, 1.5), synth.uniform(2, (C,), -0.5, 0.5)
    rsc, rsh = synth.uniform(3, (C,), 0.5, 1.5), synth.uniform(4, (C,), -0.5, 0.5)
    out = sentinel_buf(M * C)
    L.call("eav_video_bn_apply", P(xd), P(dev(sc)), P(dev(sh)), P(dev(res)), P(dev(rsc)), P(dev(rsh)), P(out), M, C, 1,
           st())
    got = take(out, M * C, (M, C), "apply")
    want = torch.relu(x * torch.from_numpy(sc) + torch.from_numpy(sh) + (res * torch.from_numpy(rsc) +
                                                                         torch.from_numpy(rsh)))
    assert torch.allclose(got, want, rtol=1e-6, atol=1e-6)
    # backward sums with the ReLU' gate from the stored output (zeros and a NaN output planted)
    y = got.clone()
    y[0, :3] = 0.0
    y[1, 0] = float("nan")
    mean, invstd = x.double().mean(0).float(), (1.0 / torch.sqrt(x.double().var(0, unbiased=False) + 1e-5)).float()
    bn = dev(torch.cat([mean, invstd, torch.zeros(4 * C)]))
    g = sentinel_buf(M * C)
    part2 = sentinel_buf(npart * 2 * C)
    L.call("eav_video_bn_bwd", P(dev(dy)), P(dev(y)), P(xd), P(bn), P(g), P(part2), M, C, st())
    gg = take(g, M * C, (M, C), "g")
    gate = ~(y <= 0)
    assert torch.equal(gg, torch.where(gate, dy, torch.zeros_like(dy)))
    p2 = take(part2, npart * 2 * C, (npart, 2, C), "bwd sums").double().sum(0)
    xh = (x.double() - mean.double()) * invstd.double()
    assert torch.allclose(p2[0], gg.double().sum(0), rtol=1e-5, atol=1e-4)
    assert torch.allclose(p2[1], (gg.double() * xh).sum(0), rtol=1e-5, atol=1e-3)


def maxpool_ref(x):
    """torch's CPU max_pool2d(3, 2, 1) with indices, as window indices kh * 3 + kw."""
    B, C, H, W = x.shape
    out, idx = F.max_pool2d(x, 3, 2, 1, return_indices=True)
    OH, OW = out.shape[2:]
    ih, iw = idx // W, idx % W
    oh = torch.arange(OH).view(1, 1, OH, 1)
    ow = torch.arange(OW).view(1, 1, 1, OW)
    return out, (ih - (2 * oh - 1)) * 3 + (iw - (2 * ow - 1))


@pytest.mark.parametrize("B,C,H,W", [(2, 64, 14, 14), (1, 64, 9, 7), (3, 16, 5, 6)])
def test_maxpool_ties_nan_and_gather_backward(B, C, H, W, L):
    x = ints(B * 100 + H, (B, C, H, W), -2, 2)          # many ties
    x[0, 0, 1, 1] = float("nan")
    x[0, 1, 2, 2] = float("nan")
    x[0, 1, 2, 3] = float("nan")
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out_w, idx_w = maxpool_ref(x)
    xd = dev(x.permute(0, 2, 3, 1))
    out = sentinel_buf(B * OH * OW * C)
    idx = sentinel_buf(B * OH * OW * C, torch.uint8)
    L.call("eav_video_maxpool_fwd", P(xd), P(out), P(idx), B, H, W, C, OH, OW, 3, 2, 1, st())
    got = take(out, B * OH * OW * C, (B, OH, OW, C), "pool").permute(0, 3, 1, 2)
    gi = take(idx, B * OH * OW * C, (B, OH, OW, C), "argmax").permute(0, 3, 1, 2).long()
    assert torch.equal(torch.isnan(got), torch.isnan(out_w))
    assert torch.equal(torch.nan_to_num(got), torch.nan_to_num(out_w))
    assert torch.equal(gi, idx_w)
    # backward: a gather in window order equals torch's scatter (integer gradients: exact)
    dout = ints(7, (B, C, OH, OW), -3, 3)
    xr = x.clone().requires_grad_(True)
    F.max_pool2d(xr, 3, 2, 1).backward(dout)
    dx = sentinel_buf(B * H * W * C)
    L.call("eav_video_maxpool_bwd", P(dev(dout.permute(0, 2, 3, 1))), P(idx), P(dx), B, H, W, C, OH, OW, 3, 2, 1, st())
    assert torch.equal(take(dx, B * H * W * C, (B, H, W, C), "pool bwd").permute(0, 3, 1, 2), xr.grad)


@pytest.mark.parametrize("B,HW,C", [(2, 49, 2048), (3, 4, 64), (1, 1, 8)])
def test_head_pools_and_backward(B, HW, C, L):
    y = ints(B + HW, (B, HW, C), -2, 2)
    y[0, 3 % HW, 0] = float("nan")
    yd = dev(y)
    pooled = sentinel_buf(2 * B * C)
    idx = sentinel_buf(B * C, torch.uint8)
    L.call("eav_video_head_pool", P(yd), P(pooled), P(idx), B, HW, C, st())
    pg = take(pooled, 2 * B * C, (2, B, C), "pooled")
    ig = take(idx, B * C, (B, C), "argmax").long()
    yc = y.permute(0, 2, 1).reshape(B, C, HW, 1)
    mx, mi = F.adaptive_max_pool2d(yc, 1, return_indices=True)
    assert torch.equal(ig, mi.view(B, C))
    assert torch.equal(torch.nan_to_num(pg[1]), torch.nan_to_num(mx.view(B, C)))
    avg = y.double().mean(1)
    fin = torch.isfinite(avg)
    assert torch.allclose(pg[0].double()[fin], avg[fin], rtol=1e-6, atol=1e-6)
    # scale-pool and the two backward kernels against autograd in float64 (finite data)
    y = torch.from_numpy(synth.normal(5, (B, HW, C), 0.0, 1.0))
    A = torch.from_numpy(synth.normal(6, (2, B, C), 0.0, 1.0))
    dz = torch.from_numpy(synth.normal(7, (B, C), 0.0, 1.0))
    dP = torch.from_numpy(synth.normal(8, (2, B, C), 0.0, 1.0))
    yd = dev(y)
    L.call("eav_video_head_pool", P(yd), P(pooled), P(idx), B, HW, C, st())
    attn, z = sentinel_buf(B * C), sentinel_buf(B * C)
    L.call("eav_video_head_scale_pool", P(yd), P(dev(A)), P(attn), P(z), B, HW, C, st())
    y64 = y.double().requires_grad_(True)
    a64 = (A[0] + A[1]).double().requires_grad_(True)
    z64 = (y64 * a64.unsqueeze(1)).mean(1)
    assert torch.allclose(take(attn, B * C, (B, C), "attn").double(), a64.detach(), rtol=0, atol=0)
    assert torch.allclose(take(z, B * C, (B, C), "z").double(), z64.detach(), rtol=1e-5, atol=1e-6)
    dA = sentinel_buf(2 * B * C)
    L.call("eav_video_head_attn_bwd", P(yd), P(dev(dz)), P(dA), B, HW, C, st())
    ga, = torch.autograd.grad(z64, [a64], dz.double(), retain_graph=True)
    dAg = take(dA, 2 * B * C, (2, B, C), "dA").double()
    assert torch.allclose(dAg[0], ga, rtol=1e-5, atol=1e-6) and torch.equal(dAg[0], dAg[1])
    dy = sentinel_buf(B * HW * C)
    L.call("eav_video_head_feat_bwd", P(dev(dz)), P(attn), P(dev(dP)), P(idx), P(dy), B, HW, C, st())
    avg64 = y64.mean(1)
    mx64 = y64.max(1).values
    total = (z64 * dz.double()).sum() + (avg64 * dP[0].double()).sum() + (mx64 * dP[1].double()).sum()
    gy, = torch.autograd.grad(total, [y64])
    assert torch.allclose(take(dy, B * HW * C, (B, HW, C), "dy").double(), gy, rtol=1e-5, atol=1e-6)
