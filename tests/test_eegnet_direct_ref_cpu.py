"""The float64 references of tests/eegnet_direct_ref.py against independent statements of the same operations (torch.nn
.functional and autograd in double on small shapes), the exactness condition of every exact-mode case, and the positions of
the case lists relative to the documented launch thresholds.  No device needed."""
import pytest
import torch
import torch.nn.functional as F

from tests import eegnet_direct_ref as R
from tests.kernel_check import assert_exact, normal

EPS = 1e-5


def near(a, b, what, tol=1e-11):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float((a - b).abs().max())
    assert err <= tol * max(1.0, float(b.abs().max())), f"{what}: {err:.3e}"


def rnd(seed, *shape):
    return normal(seed, shape).double()


def batch_bn(y, gamma, beta, dims):
    """Training-mode BatchNorm written out (biased variance), differentiable; returns (out, mean, invstd)."""
    mean = y.mean(dims, keepdim=True)
    invstd = 1.0 / torch.sqrt(((y - mean) ** 2).mean(dims, keepdim=True) + EPS)
    shape = [1, -1] + [1] * (y.dim() - 2)
    return (y - mean) * invstd * gamma.view(shape) + beta.view(shape), mean.flatten(), invstd.flatten()


@pytest.mark.parametrize("K", [1, 6, 7, 16])
def test_fir_forward_and_weight_gradient_against_conv2d_autograd(K):
    B, C, S = 2, 3, 19
    x, w = rnd(1, B, C, S), rnd(2, 8, K).requires_grad_(True)
    y = F.conv2d(x.unsqueeze(1), w.view(8, 1, 1, K), padding="same")
    r = R.fir_fwd_ref(x, w.detach())
    near(r["y"], y.detach(), "y1")
    near(r["s"], y.detach().sum((0, 2, 3)), "sum")
    near(r["q"], (y.detach() ** 2).sum((0, 2, 3)), "sum of squares")
    gamma, beta, G = rnd(3, 8) + 2.0, rnd(4, 8), rnd(5, B, 8, C, S)
    # train: BatchNorm on the batch statistics, its backward by autograd
    out, mean, invstd = batch_bn(y, gamma, beta, (0, 2, 3))
    (dW,) = torch.autograd.grad((out * G).sum(), w, retain_graph=True)
    xhat = (y.detach() - mean.view(1, 8, 1, 1)) * invstd.view(1, 8, 1, 1)
    bn = torch.stack([mean, invstd, gamma * invstd, beta, G.mean((0, 2, 3)), (G * xhat).mean((0, 2, 3))]).detach()
    near(R.fir_wgrad_ref(x, y.detach(), G, bn, K, True)["dW"], dW, "dW1 (train)", 1e-10)
    # eval: constants
    bn = torch.stack([rnd(6, 8), rnd(7, 8).abs() + 0.5, rnd(8, 8), rnd(9, 8), rnd(10, 8), rnd(11, 8)])
    out = (y - bn[0].view(1, 8, 1, 1)) * bn[2].view(1, 8, 1, 1)
    (dW,) = torch.autograd.grad((out * G).sum(), w)
    near(R.fir_wgrad_ref(x, None, G, bn, K, False)["dW"], dW, "dW1 (eval)", 1e-10)


@pytest.mark.parametrize("S,K", [(19, 7), (40, 300), (333, 64)])
def test_fft_correlation_is_the_direct_sum(S, K):
    dy, x = rnd(1, 2, 8, 3, S), rnd(2, 2, 3, S)
    near(R.corr_fft(dy, x, K), R.corr_direct(dy, x, K), "corr_fft", 1e-12)


def test_block1_inference_against_the_module_chain():
    B, C, S, K = 2, 5, 24, 9
    _, _, w1, bn1, w2, bn2 = R.block1_inputs("rounded", B, C, S, K)
    x = rnd(1, B, C, S)
    y = F.conv2d(x.unsqueeze(1), w1.double().view(8, 1, 1, K), padding="same")
    a1 = F.elu(y * bn1[2].double().view(1, 8, 1, 1) + bn1[3].double().view(1, 8, 1, 1))
    z = F.conv2d(a1, w2.double().view(64, 1, C, 1), groups=8).squeeze(2)
    a2 = F.elu(z * bn2[2].double().view(1, 64, 1) + bn2[3].double().view(1, 64, 1))
    r = R.block1_infer_ref(x, w1, bn1, w2, bn2)
    near(r["p"], F.avg_pool1d(a2, 4), "p2")
    assert float(r["bound"].min()) > 0


@pytest.mark.parametrize("S", [24, 1030])
def test_depthwise_forward_and_backward_against_autograd(S):
    B, C = 2, 5
    _, bn1, w2, bn2, _ = R.dw_inputs("rounded", B, C, S)
    y1, dz = rnd(1, B, 8, C, S), rnd(2, B, 64, S)
    w = w2.double().requires_grad_(True)
    o = (y1 * bn1[2].double().view(1, 8, 1, 1) + bn1[3].double().view(1, 8, 1, 1)).requires_grad_(True)
    z = F.conv2d(F.elu(o), w.view(64, 1, C, 1), groups=8).squeeze(2)
    r = R.dw_fwd_ref(y1, bn1, w2, bn2 if S % 4 == 0 else None)
    near(r["z"], z.detach(), "z")
    near(r["s"].sum(1), z.detach().sum(2), "sum z")
    near(r["q"].sum(1), (z.detach() ** 2).sum(2), "sum z^2")
    if S % 4 == 0:
        near(r["p"], F.avg_pool1d(F.elu(z.detach() * bn2[2].double().view(1, 64, 1) + bn2[3].double().view(1, 64, 1)), 4), "p2")
    g, dW = torch.autograd.grad((z * dz).sum(), (o, w))
    rb = R.dw_bwd_ref(y1, dz, None, bn1, w2)
    near(rb["g1"], g, "g1")
    near(rb["dW"].sum((0, 1)).view(64, C), dW, "dW2")
    xhat = (y1 - bn1[0].double().view(1, 8, 1, 1)) * bn1[1].double().view(1, 8, 1, 1)
    near(rb["st"].sum((0, 1)), torch.cat([g.sum((0, 2, 3)), (g * xhat).sum((0, 2, 3))]), "sum g1, sum g1 xhat")
    assert rb["st"].shape == (B, R.cdiv(S, 1024), 16) and rb["dW"].shape == (B, R.cdiv(S, 1024), 64 * C)


@pytest.mark.parametrize("T,P,drop", [(24, 4, 0.0), (27, 8, 0.5), (44, 8, -0.5), (17, 4, 0.5)])
def test_pool_passes_against_autograd_of_batchnorm_elu_avgpool_dropout(T, P, drop):
    B = 3
    _, bn, dp, mask = R.pool_inputs("rounded", B, T, P, drop)
    u = rnd(1, B, 64, T).requires_grad_(True)
    dp, To = dp.double(), T // P
    mult = R.pool_mult(mask, drop, (B, 64, To))
    gamma, beta = rnd(2, 64) + 2.0, rnd(3, 64)
    bnout, mean, invstd = batch_bn(u, gamma, beta, (0, 2))
    bnout.retain_grad()
    out = F.avg_pool1d(F.elu(bnout), P) * mult
    (out * dp).sum().backward()
    bn = torch.stack([mean, invstd, gamma * invstd, beta - mean * gamma * invstd, bn[4].double(), bn[5].double()]).detach()
    near(R.pool_fwd_ref(u.detach(), bn, P, mult)["out"], out.detach(), "pool out")
    r = R.pool_bwd_ref(dp, u.detach(), bn, P, mult)
    near(r["g"], bnout.grad, "g")
    sums = R.pool_sums(r, 1)
    count = B * T
    bn[4], bn[5] = sums["s"].sum(0) / count, sums["q"].sum(0) / count         # what eav_bn_bwd_finalize leaves
    near(R.pool_bwd_ref(dp, u.detach(), bn, P, mult)["du"], u.grad, "du (train)", 1e-10)
    near(R.pool_bwd_ref(dp, u.detach(), bn, P, mult, train=False)["du"], bn[2].view(1, 64, 1) * bnout.grad, "du (eval)")


def test_fused_depthwise_backward_against_autograd_of_the_chain():
    B, C, S = 2, 4, 22
    _, _, dp2, bn2, bn1, w2, mask = R.dw_fused_inputs("rounded", B, C, S, 0.5)
    y1 = rnd(1, B, 8, C, S)
    mult = R.pool_mult(mask, 0.5, dp2.shape)
    w = w2.double().requires_grad_(True)
    o = (y1 * bn1[2].double().view(1, 8, 1, 1) + bn1[3].double().view(1, 8, 1, 1)).requires_grad_(True)
    z = F.conv2d(F.elu(o), w.view(64, 1, C, 1), groups=8).squeeze(2)
    p = F.avg_pool1d(F.elu(z * bn2[2].double().view(1, 64, 1) + bn2[3].double().view(1, 64, 1)), 4) * mult
    g, dW = torch.autograd.grad((p * dp2.double()).sum(), (o, w))
    r = R.dw_bwd_fused_ref(y1, z.detach(), dp2, bn2, bn1, w2, mult, train=False)
    near(r["g1"], g, "g1")
    near(r["dW"].sum((0, 1)).view(64, C), dW, "dW2")
    pr = R.pool_bwd_ref(dp2, z.detach(), bn2, 4, mult, train=False)
    near(r["p2"].sum((0, 1)), torch.cat([pr["g"].sum((0, 2)), (pr["g"] * pr["uhat"]).sum((0, 2))]), "depthwiseBN sums")
    rt = R.dw_bwd_fused_ref(y1, z.detach(), dp2, bn2, bn1, w2, mult, train=True)
    near(rt["g1"], R.dw_bwd_ref(y1, R.pool_bwd_ref(dp2, z.detach(), bn2, 4, mult)["du"], None, bn1, w2)["g1"], "g1 (train)")
    assert not torch.equal(rt["g1"], r["g1"])


@pytest.mark.parametrize("B,T", [(2, 21), (1, 5)])
def test_conv64_against_conv2d_autograd(B, T):
    x = rnd(1, B, 64, T).requires_grad_(True)
    w = rnd(2, 64, 64, 16).requires_grad_(True)
    du = rnd(3, B, 64, T)
    out = F.conv2d(x.unsqueeze(2), w.view(64, 64, 1, 16), padding="same").squeeze(2)
    dx, dW = torch.autograd.grad((out * du).sum(), (x, w))
    r = R.conv64_fwd_ref(x.detach(), w.detach())
    near(r["out"], out.detach(), "out")
    near(r["s"], out.detach().sum((0, 2)), "sum")
    near(r["q"], (out.detach() ** 2).sum((0, 2)), "sum of squares")
    near(R.conv64_dgrad_ref(du, w.detach())["out"], dx, "dx")
    near(R.conv64_wgrad_ref(du, x.detach())["dW"], dW, "dW")
    wf, wb = R.conv64_prep_ref(w.detach())
    for o, i, k in [(0, 0, 0), (63, 1, 15), (5, 62, 3), (17, 33, 8)]:
        assert wf[i * 16 + k, o] == w[o, i, k] and wb[o * 16 + (15 - k), i] == w[o, i, k]


# ------------------------------------------------------------------------------------ exactness of the exact-mode cases
def check_exact(r, what, pre=True):
    for bound, quantum, name in r["exact"]:
        assert_exact(bound, quantum, f"{what} {name}")
    if pre:
        assert r["min_pre"] >= 0.0, f"{what}: a pre-activation of {r['min_pre']} (ELU must be the identity)"


@pytest.mark.parametrize("case", R.FIR_FWD_CASES)
def test_exact_fir_forward_cases(case):
    B, C, S, K = case
    xs, idx, w = R.fir_inputs("exact", B, C, S, K)
    assert w[:, 0].abs().min() > 0 and w[:, K - 1].abs().min() > 0          # both ends of the window carry weight
    check_exact(R.fir_fwd_ref(xs[idx], w), f"fir_fwd {case}", pre=False)


@pytest.mark.parametrize("case", R.FIR_WGRAD_CASES)
def test_exact_fir_weight_gradient_cases(case):
    B, C, S, K = case
    xs, idx, y1, g1, bn = R.fir_wgrad_inputs("exact", B, C, S, K)
    r = R.fir_wgrad_ref(xs[idx], y1, g1, bn, K, True, "exact")
    check_exact(r, f"fir_wgrad {case}", pre=False)
    dy, _, _ = R.bn_fold(y1, g1, bn, True)
    assert torch.equal(dy, dy.round()) and torch.equal(r["dW"], r["dW"].round())


@pytest.mark.parametrize("case", R.INFER_CASES)
def test_exact_block1_inference_cases(case):
    B, C, S, K = case
    xs, idx, w1, bn1, w2, bn2 = R.block1_inputs("exact", B, C, S, K)
    check_exact(R.block1_infer_ref(xs[idx], w1, bn1, w2, bn2), f"block1_infer {case}")


@pytest.mark.parametrize("case", R.DW_CASES)
def test_exact_depthwise_cases(case):
    B, C, S = case
    y1, bn1, w2, bn2, dz = R.dw_inputs("exact", B, C, S)
    check_exact(R.dw_fwd_ref(y1, bn1, w2, bn2 if S % 4 == 0 else None), f"dw_fwd {case}")
    check_exact(R.dw_bwd_ref(y1, dz, None, bn1, w2), f"dw_bwd {case}")


@pytest.mark.parametrize("case", R.DW_FUSED_CASES)
def test_exact_fused_depthwise_backward_cases(case):
    B, C, S, drop = case
    y1, z, dp2, bn2, bn1, w2, mask = R.dw_fused_inputs("exact", B, C, S, drop)
    mult = R.pool_mult(mask, drop, dp2.shape)
    for train in (True, False):
        check_exact(R.dw_bwd_fused_ref(y1, z, dp2, bn2, bn1, w2, mult, train), f"dw_bwd_fused {case} train={train}")


@pytest.mark.parametrize("case", R.POOL_CASES)
def test_exact_pool_cases(case):
    B, T, P, drop = case
    u, bn, dp, mask = R.pool_inputs("exact", B, T, P, drop)
    mult = R.pool_mult(mask, drop, dp.shape)
    check_exact(R.pool_fwd_ref(u, bn, P, mult), f"pool_fwd {case}")
    r = R.pool_bwd_ref(dp, u, bn, P, mult)
    s = R.pool_sums(r, 1)
    assert r["min_pre"] >= 0
    for bound, quantum, name in [(float(s["s_mag"].max()), 1.0, "sum g"), (float(s["q_mag"].max()), 0.5, "sum g uhat"),
                                 (float(r["du_mag"].max()), 0.5, "du")]:
        assert_exact(bound, quantum, f"pool_bwd {case} {name}")


@pytest.mark.parametrize("case", R.CONV64_CASES)
def test_exact_conv64_cases(case):
    B, T = case
    x, w, du = R.conv64_inputs("exact", B, T)
    check_exact(R.conv64_fwd_ref(x, w), f"conv64_fwd {case}", pre=False)
    check_exact(R.conv64_dgrad_ref(du, w), f"conv64 dgrad {case}", pre=False)
    check_exact(R.conv64_wgrad_ref(du, x), f"conv64_wgrad {case}", pre=False)
    assert float((w != 0).float().mean()) > 0.1 and (w != 0).any(0).all() and (w != 0).any(1).all()


# ------------------------------------------------------------------------------------ the case lists sit where they claim
def test_case_lists_reach_every_form_and_every_second_trip():
    K_fwd = {K for _, _, S, K in R.FIR_FWD_CASES if S == 130}
    assert {1, 65} <= K_fwd and {66, 129} <= K_fwd and {130, 300} <= K_fwd
    assert [R.fir_nstep(K) for K in (1, 65, 66, 129, 130, 300)] == [34, 34, 66, 66, 152, 152]
    assert {(K - 1) % 2 for K in K_fwd} == {0, 1}                              # even and odd kernels: both 'same' splits
    multi = [c for c in R.FIR_FWD_CASES if c[0] * c[1] * R.fir_nseg(c[2]) > 512]
    assert {R.fir_nstep(c[3]) for c in multi} == {66, 152} and all(c[0] * c[1] == 527 for c in multi)
    assert R.fir_nseg(2048) == 1 and R.fir_nseg(2052) == 2 and R.cdiv(2052, 128) - 16 == 1      # second segment: one tile
    assert any(S % 4 for _, _, S, _ in R.FIR_FWD_CASES)
    # weight gradient: S + 1 positions - a multiple of 248 needs one more chunk
    assert [R.wgrad_geometry(S)[0] for S in (3, 247, 248, 249, 496, 1984)] == [1, 1, 2, 2, 3, 9]
    assert [R.wgrad_geometry(S)[1] for S in (3, 247, 248)] == [8, 248, 128]
    assert all(ch % 8 == 0 and ch <= 248 and n * ch >= S + 1 for S in range(1, 2100) for n, ch in [R.wgrad_geometry(S)])
    assert [R.wgrad_nt(K) for K in (1, 64, 65, 128, 129, 300)] == [2, 2, 4, 4, 10, 10]
    multi = [c for c in R.FIR_WGRAD_CASES if c[0] * c[1] * R.wgrad_geometry(c[2])[0] > 4 * 768]
    assert {R.wgrad_nt(c[3]) for c in multi} == {2, 4, 10}
    assert all(R.fir_wgrad_chain(*c[:3]) > R.wgrad_geometry(c[2])[1] + 3 for c in multi)        # a wave's second item
    # inference
    assert {R.fir_nstep(K) for _, _, _, K in R.INFER_CASES} == {34, 66, 152}
    assert {C for _, C, _, _ in R.INFER_CASES} >= {1, 3, 32}
    assert [R.infer_nseg(S) for S in (4, 128, 132, 512, 516)] == [1, 1, 1, 1, 2]
    assert [c for c in R.INFER_CASES if c[0] * R.infer_nseg(c[2]) > 256] == [(130, 2, 516, 300)]
    # depthwise
    assert [R.dw_plan(S) for S in (4, 252, 256, 260, 512, 516, 1024, 1028)] == [4256] * 3 + [4512] * 2 + [1256] * 3
    assert {C for _, C, _ in R.DW_CASES} == {1, 3, 30, 32} and {B for B, _, _ in R.DW_CASES} == {1, 3}
    assert any(S % 4 and R.dw_plan(S) == g for g in (4512, 1256) for _, _, S, _ in R.DW_FUSED_CASES)
    assert {(R.dw_plan(S), d) for _, _, S, d in R.DW_FUSED_CASES} == {(g, d) for g in (4256, 4512, 1256) for d in R.DROP_MODES}
    # pool: the second trip of the 256-thread loops; a tail quad for P = 8
    assert any(P == 4 and T // P > 256 for _, T, P, _ in R.POOL_CASES) and any(P == 8 and T // P > 256 for _, T, P, _ in R.POOL_CASES)
    assert any(P == 8 and T % 8 >= 4 for _, T, P, _ in R.POOL_CASES)
    assert {(P, d) for _, _, P, d in R.POOL_CASES} == {(P, d) for P in (4, 8) for d in R.DROP_MODES}
    # separableConv
    assert [R.conv64_tile(B, T) for B, T in R.CONV64_CASES] == [32, 32, 32, 32, 128, 128]
    assert 129 * R.cdiv(130, 128) == 258 > 256 > 192 and R.conv64_visits(129, 130) == 8 and any(T % 4 for _, T in R.CONV64_CASES)
