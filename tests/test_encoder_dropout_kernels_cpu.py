"""The host side of tests/test_encoder_dropout_kernels_gpu.py without a GPU: the numpy restatement of the dropout generator
(statistics, seed / counter algebra), the float64 attention reference against a direct restatement, and the case lists
against the dispatch constants read out of the kernel sources."""
import os
import re

import numpy as np
import pytest
import torch

from tests import encoder_dropout_kernel_ref as R
from tests.test_transformer_kernels_gpu import _attn_ref

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eav_amd", "csrc")
N20 = 1 << 20


def _frac_bound(p, n):
    return 5.0 * np.sqrt(p * (1.0 - p) / n)


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_hash_keep_statistics(p):
    """|kept / n - (1 - p)| <= 5 sqrt(p (1 - p) / n) at n = 2^20; two counters, and two seeds, differ in a fraction within
    the same bound of 2 p (1 - p)."""
    seed = 0x1234 << 40
    a = R.hash_keep(seed, N20, p)
    assert a.dtype == np.uint8 and a.shape == (N20,) and set(np.unique(a)) <= {0, 1}
    assert abs(a.mean() - (1.0 - p)) <= _frac_bound(p, N20)
    for what, b in (("counter", R.hash_keep(seed, N20, p, counter=1)), ("seed", R.hash_keep(seed + (1 << 40), N20, p))):
        assert abs((a != b).mean() - 2 * p * (1 - p)) <= _frac_bound(p, N20), what


def test_hash_keep_counter_is_a_seed_offset_and_p0_keeps_everything():
    for seed, c in ((7, 3), (0x5 << 40, 5), ((1 << 64) - 3, 4)):       # (the last: seed + 2 c wraps modulo 2^64)
        assert np.array_equal(R.hash_keep(seed, 4099, 0.3, counter=c), R.hash_keep(seed + 2 * c, 4099, 0.3))
    assert np.array_equal(R.hash_keep(9, 4099, 0.3, counter=0), R.hash_keep(9, 4099, 0.3))
    assert R.hash_keep(11, N20, 0.0).all()


def test_hash_keep_matches_a_scalar_restatement():
    """The vectorised uint64 arithmetic against Python integers reduced modulo 2^64, element by element."""
    seed, p = (3 << 40) + 17, 0.5
    got = R.hash_keep(seed, 257, p, counter=2)
    for idx in range(257):
        z = (seed + 4 + (idx + 1) * 0x9E3779B97F4A7C15) & R.M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & R.M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & R.M64
        z ^= z >> 31
        assert got[idx] == (np.float32(z >> 40) * np.float32(2.0 ** -24) >= np.float32(p)), idx


def test_scale32_and_the_split_exponent():
    assert R.scale32(0.5) == 2.0 and R.scale32(0.75) == 4.0
    assert R.scale32(0.1) == float(np.float32(1.0) / np.float32(np.float32(1.0) - np.float32(0.1)))
    assert [R.sp_exponent(p) for p in R.SP_P] == [1, 1, 2, 2, 4]


def test_attention_ref_equals_a_direct_restatement():
    """(B, H, N) = (2, 2, 5) in float64: O, lse and the three gradients written out per (image, head) with the softmax
    Jacobian by hand - no autograd, no batched products."""
    B, H, N, p = 2, 2, 5, 0.3
    D = H * 64
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(B * N, 3 * D, generator=g, dtype=torch.float64)
    dO = torch.randn(B * N, D, generator=g, dtype=torch.float64)
    mask = R.planted_mask(5, B, H, N, p)
    assert not mask[0, 0, 0].any() and not mask[0, 0, :, 2].any() and not mask[-1, -1, -1].any()
    assert mask[0, 0, 1, [0, 1, 3, 4]].all()
    out, dqkv, lse = R.attention_ref(qkv, dO, mask, B, H, N, p)
    s32 = R.scale32(p)
    for b in range(B):
        for h in range(H):
            rows = slice(b * N, (b + 1) * N)
            q, k, v = (qkv[rows, i * D + 64 * h:i * D + 64 * h + 64] for i in range(3))
            do = dO[rows, 64 * h:64 * h + 64]
            S = q @ k.t() / 8.0
            P = torch.exp(S - S.max(1, keepdim=True).values)
            P = P / P.sum(1, keepdim=True)
            Mk = torch.from_numpy(mask[b, h].astype(np.float64)) * s32
            Pd = P * Mk
            O = Pd @ v
            dPd = (do @ v.t()) * Mk
            dS = P * (dPd - (P * dPd).sum(1, keepdim=True))
            want = {"O": (out[rows, 64 * h:64 * h + 64], O), "dQ": (dqkv[rows, 64 * h:64 * h + 64], dS @ k / 8.0),
                    "dK": (dqkv[rows, D + 64 * h:D + 64 * h + 64], dS.t() @ q / 8.0),
                    "dV": (dqkv[rows, 2 * D + 64 * h:2 * D + 64 * h + 64], Pd.t() @ do),
                    "lse": (lse[b * H + h], torch.log(torch.exp(S).sum(1)))}
            for name, (got, ref) in want.items():
                assert (got - ref).abs().max().item() <= 1e-13 * max(1.0, ref.abs().max().item()), (b, h, name)
    assert (out[0, :64] == 0).all() and (dqkv[0, :64] == 0).all()              # the fully dropped query row
    assert (dqkv[2, 2 * D:2 * D + 64] == 0).all()                              # dV of the fully dropped key column


def test_attention_ref_without_dropout_is_the_undropped_reference():
    """An all-ones mask at p = 0 (scale 1): the forward of test_transformer_kernels_gpu._attn_ref, bit for bit up to the
    order of its float64 sums."""
    B, H, N = 2, 3, 7
    D = H * 64
    g = torch.Generator().manual_seed(4)
    qkv = torch.randn(B * N, 3 * D, generator=g)
    dO = torch.randn(B * N, D, generator=g)
    out, _, lse = R.attention_ref(qkv, dO, np.ones((B, H, N, N), np.uint8), B, H, N, 0.0)
    q, k, v, s = _attn_ref(qkv.numpy(), B, H, N, 64)
    ref = (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(B * N, D)
    assert (out - ref).abs().max().item() <= 1e-14 * ref.abs().max().item()
    assert (lse.view(B, H, N) - torch.logsumexp(s, -1)).abs().max().item() <= 1e-13
    out32, g32, lse32 = R.attention_ref(qkv, dO, np.ones((B, H, N, N), np.uint8), B, H, N, 0.0, dtype=torch.float32)
    assert out32.dtype == g32.dtype == lse32.dtype == torch.float32
    assert (out32.double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()


def test_softmax_dropout_ref_is_the_jacobian_of_its_forward():
    g = torch.Generator().manual_seed(6)
    s = torch.randn(3, 9, generator=g, dtype=torch.float64).requires_grad_(True)
    dP = torch.randn(3, 9, generator=g, dtype=torch.float64)
    mask = R.hash_keep(8, 27, 0.4).reshape(3, 9)
    P, Pd, dS, mag = R.softmax_dropout_ref(s.detach(), dP, mask, 0.4)
    pd = torch.softmax(s, -1) * torch.from_numpy(mask.astype(np.float64)) * R.scale32(0.4)
    pd.backward(dP)
    assert torch.equal(Pd, pd.detach()) and (dS - s.grad).abs().max().item() <= 1e-15
    assert (mag >= dS.abs() - 1e-18).all()


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const(text, pattern):
    m = re.search(pattern, text)
    assert m, pattern
    return int(m.group(1))


def test_case_lists_reach_every_dispatch_branch():
    """The constants the launchers dispatch on, read out of the sources, against the case lists of the GPU tests."""
    attn, sp, tfd = _src("attention.hip"), _src("attention_sp.hip"), _src("tf_dropout.hip")
    TQ = _const(attn, r"constexpr int TQ = (\d+);")
    nw4 = _const(sp, r"int g_nw4_above = (\d+);")
    assert (TQ, nw4) == (128, 128)
    npl = [int(x) for x in re.findall(r"if \(N <= (\d+)\)\s+hipLaunchKernelGGL\(softmax_dropout_fwd_kernel", tfd)]
    assert npl == [256, 1280] and npl == [int(x) for x in
                                          re.findall(r"if \(N <= (\d+)\)\s+hipLaunchKernelGGL\(softmax_dropout_bwd_kernel", tfd)]
    nmax = _const(tfd, r"N <= (\d+) && EAV_DROP_ARGS_OK")
    assert nmax == 2048
    m = re.search(r"cdiv64\(n, (\d+)\) < (\d+) \? cdiv64\(n, \1\) : \2", tfd)
    assert m and int(m.group(1)) * int(m.group(2)) == R.EW_CAP

    for cases in (R.ATTN_CASES, R.SP_CASES):
        ns = {n for _, _, n in cases}
        assert any(n <= 32 for n in ns)                                     # one ragged key tile
        assert any(n % 32 == 0 and n % TQ for n in ns) and TQ in ns         # no ragged tile: multiples of 32 and of 128
        assert {TQ, TQ + 1, 1214} <= ns                                     # either side of the workgroup; the workload
        assert any(n % 32 and n > TQ for n in ns)
        assert max(b * h for b, h, _ in cases) > 4                          # the (b H + h) term beyond the reduced model
        assert any(h > 1 and b > 1 for b, h, _ in cases)
    assert {1, 32, 33} <= {n for _, _, n in R.ATTN_CASES}
    # split kernels: N <= g_nw4_above takes the 2-wave forward, above it the 4-wave one; the workgroup map has full groups
    # of 8 image-heads and a remainder
    ns = {n for _, _, n in R.SP_CASES}
    assert nw4 in ns and nw4 + 1 in ns
    bh = {b * h for b, h, _ in R.SP_CASES}
    assert any(x > 8 and x % 8 for x in bh) and any(x >= 8 and x % 8 == 0 for x in bh) and any(x < 8 for x in bh)
    assert {R.sp_exponent(p) for p in R.SP_P} == {1, 2, 4} and 0.5 in R.SP_P
    assert R.SP_SPIKE[:3] in R.SP_CASES
    # softmax: both sides of every NPL switch point, the largest N, a partial 64-lane step, a partial block of four rows
    for edge in npl:
        assert edge in R.SOFTMAX_N and edge + 1 in R.SOFTMAX_N
    assert nmax in R.SOFTMAX_N and 1 in R.SOFTMAX_N and {63, 64, 65} <= set(R.SOFTMAX_N)
    assert any(r % 4 for r in R.SOFTMAX_ROWS) and any(r % 4 == 0 for r in R.SOFTMAX_ROWS)
    # element-wise kernels: below one block, a ragged last block, and past the block cap (the grid-stride loop)
    assert max(R.MASK_N) > R.EW_CAP and min(R.MASK_N) == 1 and any(n % 256 for n in R.MASK_N if n > 1)
    assert max(R.ADD_N) // 4 > R.EW_CAP and all(n % 4 == 0 for n in R.ADD_N) and any((n // 4) % 256 for n in R.ADD_N)
