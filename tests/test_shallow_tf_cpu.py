"""CPU self-check of tests/shallow_tf_ref.py: the forward references against the torch ops the header names and every
backward reference (written out from the formulas of include/eav_hip.h) against torch.autograd.grad of the float64
forward of the layer it belongs to."""
import pytest
import torch
import torch.nn.functional as F

from tests import shallow_tf_ref as R
from tests.audio_conv_ref import f32_scale

torch.manual_seed(0)
TOL = 1e-11


def rnd(*shape):
    return torch.randn(*shape, dtype=torch.float64)


def close(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float((a - b).abs().max())
    assert err <= TOL * max(1.0, float(b.abs().max())), (what, err)


@pytest.mark.parametrize("KC", [1, 2, 3, 8])
@pytest.mark.parametrize("S", [8, 9, 13])
@pytest.mark.parametrize("C,NF", [(1, 1), (3, 4)])
def test_shallow_embed_in_the_module_order(C, NF, S, KC):
    """The module's own order: conv (1,KC) on [B,1,C,S] (valid), then one Linear(Chans -> 1) per filter.  The kernels
    project the channels first; the references must agree with the module's order, forward and backward."""
    B = 2
    x = rnd(B, C, S)
    wc, wv = rnd(NF, KC).requires_grad_(), rnd(NF, C).requires_grad_()
    h = F.conv2d(x.unsqueeze(1), wc.view(NF, 1, 1, KC))                                   # [B,NF,C,T]
    v = torch.cat([F.linear(h[:, i].permute(0, 2, 1), wv[i:i + 1]) for i in range(NF)], dim=-1)   # [B,T,NF]
    u, vr = R.shallow_embed_fwd_ref(x, wc.detach(), wv.detach())
    close(vr, v.detach(), "v")
    dv = rnd(*v.shape)
    g_wc, g_wv = torch.autograd.grad(v, (wc, wv), dv)
    dwc, dwv = R.shallow_embed_bwd_ref(dv, x, u, wc.detach())
    close(dwc, g_wc, "dWc")
    close(dwv, g_wv, "dWv")


def test_relu_dropout_and_its_backward_follow_torch_at_nan():
    h = torch.tensor([float("nan"), 2.0, -1.0, 0.0, -0.0, 3.0, float("nan")], dtype=torch.float64, requires_grad=True)
    mask = torch.tensor([1, 1, 1, 1, 1, 0, 0], dtype=torch.uint8)
    p = 0.25
    y = F.relu(h) * mask.double() * f32_scale(p)
    got = R.relu_dropout_ref(h.detach(), p, mask)
    assert torch.equal(torch.isnan(got), torch.isnan(y.detach())) and torch.isnan(got[0]) and torch.isnan(got[6])
    close(torch.nan_to_num(got), torch.nan_to_num(y.detach()), "relu_dropout")
    dact = rnd(7)
    want, = torch.autograd.grad(y, h, dact)
    bwd = R.relu_dropout_bwd_ref(dact, got, p)
    # the output does not say whether a NaN was kept: the backward treats it as kept (element 6 is the dropped NaN)
    close(bwd[:6], want[:6], "relu_dropout_bwd")
    assert want[0] == dact[0] * f32_scale(p) and bwd[6] == dact[6] * f32_scale(p) and want[6] == 0
    close(R.dropout_add_ref(h.detach()[1:6], dact[1:6], p, mask[1:6]),
          dact[1:6] + h.detach()[1:6] * mask[1:6].double() * f32_scale(p), "dropout_add")


def test_colstats_and_add_strided():
    x = rnd(600, 7)
    part = R.colstats_ref(x, 5)
    assert part.shape == (3, 10)
    close(part.sum(0), torch.cat([x[:, :5].sum(0), (x[:, :5] ** 2).sum(0)]), "colstats")
    close(part[2], torch.cat([x[512:, :5].sum(0), (x[512:, :5] ** 2).sum(0)]), "last chunk")
    close(R.add_strided_ref(x, x[:, 2:], 3), x[:, :3] + x[:, 2:5], "add_strided")


# (T, NP, win, stride): the model's geometry; gaps (win < stride); win == stride; overlap; all with tail tokens
GEOMS = [(500, 65, 35, 7), (40, 5, 2, 7), (30, 6, 4, 4), (33, 4, 8, 3)]


@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "mask"])
@pytest.mark.parametrize("T,NP,win,stride", GEOMS, ids=[f"T{t}-NP{n}-w{w}-s{s}" for t, n, w, s in GEOMS])
def test_head_backward_through_batchnorm(T, NP, win, stride, drop):
    """BatchNorm (batch statistics over tokens) -> square -> AvgPool(1,win)/stride -> log(clamp) -> masked dropout, with
    pooled values planted below lo, above hi and exactly at both bounds: eav_sqpool_log_bwd's g and sums, finished as
    eav_bn_bwd_finalize does (m1 = mean g, m2 = mean g xhat), give eav_bn_rows_bwd the input gradient of the chain."""
    B, NF, eps, p = 2, 3, 1e-5, 0.25
    need = (NP - 1) * stride + win
    assert need < T                                                # tail tokens beyond the last window
    x = rnd(B, T, NF).requires_grad_()
    gamma, beta = rnd(NF), rnd(NF)
    mean, var = x.detach().mean((0, 1)), x.detach().var((0, 1), unbiased=False)
    invstd = (var + eps).rsqrt()
    bn = torch.stack([mean, invstd, gamma * invstd, beta - mean * gamma * invstd])
    pooled_r, _, _, _ = R.sqpool_ref(x.detach(), bn, NP, win, stride)
    h = F.batch_norm(x.permute(0, 2, 1).unsqueeze(2), None, None, gamma, beta, True, 0.1, eps)
    m = F.avg_pool2d(torch.square(h), (1, win), stride=(1, stride)).squeeze(2)[..., :NP]
    close(pooled_r, m.detach(), "pooled")
    # the backward takes the forward's stored means; the clamp bounds are the third smallest and third largest of them, so
    # that one mean sits exactly on each bound and two fall outside on either side
    pooled_r = m.detach().clone()
    srt = pooled_r.flatten().sort().values
    lo, hi = float(srt[2]), float(srt[-3])
    assert int((m.detach() == lo).sum()) == 1 and int((m.detach() == hi).sum()) == 1
    assert int((m.detach() < lo).sum()) == 2 and int((m.detach() > hi).sum()) == 2
    mask = (torch.rand(B, NF, NP) >= p).to(torch.uint8) if drop else None
    pp = p if drop else 0.0
    out = (torch.log(torch.clamp(m, lo, hi)) * R.drop_mult(m.shape, pp, mask)).flatten(1)
    close(R.sqpool_log_out_ref(pooled_r, lo, hi, pp, mask), out.detach(), "out")
    dy = rnd(*out.shape)
    want, = torch.autograd.grad(out, x, dy)
    r = R.sqpool_log_bwd_ref(dy, pooled_r, x.detach(), bn, NP, win, stride, lo, hi, pp, mask)
    assert (r["g"][:, need:] == 0).all()
    cnt = B * T
    bn6 = torch.cat([bn, (r["part"].sum(0)[:NF] / cnt).unsqueeze(0), (r["part"].sum(0)[NF:] / cnt).unsqueeze(0)])
    dx, mag = R.bn_rows_bwd_ref(r["g"].reshape(B * T, NF), x.detach().reshape(B * T, NF), bn6)
    close(dx.view(B, T, NF), want, "dx")
    assert (mag >= dx.abs() - 1e-12).all() and (r["g_mag"] >= r["g"].abs() - 1e-12).all()
