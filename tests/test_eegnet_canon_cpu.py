"""CPU self-check of tests/eegnet_canon_ref.py: every backward reference (written out from the formulas of
include/eav_hip.h) against torch.autograd.grad of the float64 forward of the layer it belongs to, on small shapes with
even and odd tap counts, fewer samples than taps, and sample counts that are no multiple of 4."""
import pytest
import torch
import torch.nn.functional as F

from tests import eegnet_canon_ref as R

torch.manual_seed(0)
TOL = 1e-11


def rnd(*shape):
    return torch.randn(*shape, dtype=torch.float64)


def close(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float((a - b).abs().max())
    assert err <= TOL * max(1.0, float(b.abs().max())), (what, err)


def bn_rows(mean, var, gamma, beta, eps, m1=None, m2=None):
    """mean, invstd, scale, shift (, m1, m2) as eav_bn_finalize / eav_bn_bwd_finalize leave them."""
    invstd = (var + eps).rsqrt()
    rows = [mean, invstd, gamma * invstd, beta - mean * gamma * invstd]
    if m1 is not None:
        rows += [m1, m2]
    return torch.stack(rows)


@pytest.mark.parametrize("K", [1, 2, 3, 8, 9])
@pytest.mark.parametrize("S", [5, 7, 12])
def test_tconv_fwd_is_torch_same_conv(K, S):
    x, w = rnd(2, 3, S), rnd(4, K)
    ref = F.conv2d(x.unsqueeze(1), w.view(4, 1, 1, K), padding="same")
    close(R.tconv_fwd_ref(x, w), ref, "y1")


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("K", [1, 2, 3, 8, 9])
@pytest.mark.parametrize("S", [5, 7, 12])
def test_tconv_wgrad_with_folded_batchnorm(K, S, training):
    """conv -> BatchNorm2d(F1); g1 = the gradient arriving at the BatchNorm output; m1 = mean(g1), m2 = mean(g1 xhat) over
    (b, c, t) as eav_bn_bwd_finalize forms them in training mode, both 0 on running statistics."""
    B, C, F1, eps = 2, 3, 4, 1e-3
    x, w = rnd(B, C, S), rnd(F1, K).requires_grad_()
    gamma, beta, g1 = rnd(F1), rnd(F1), rnd(B, F1, C, S)
    y1 = F.conv2d(x.unsqueeze(1), w.view(F1, 1, 1, K), padding="same")
    if training:
        mean, var = y1.mean((0, 2, 3)), y1.var((0, 2, 3), unbiased=False)
        out = F.batch_norm(y1, None, None, gamma, beta, True, 0.1, eps)
    else:
        mean, var = rnd(F1), rnd(F1).abs() + 0.5
        out = F.batch_norm(y1, mean, var, gamma, beta, False, 0.1, eps)
    want, = torch.autograd.grad(out, w, g1)
    mean, var, y1d = mean.detach(), var.detach(), y1.detach()
    xhat = (y1d - mean.view(1, -1, 1, 1)) * (var + eps).rsqrt().view(1, -1, 1, 1)
    m1 = g1.mean((0, 2, 3)) if training else torch.zeros(F1, dtype=torch.float64)
    m2 = (g1 * xhat).mean((0, 2, 3)) if training else torch.zeros(F1, dtype=torch.float64)
    got, mag = R.tconv_wgrad_ref(x, y1d, g1, bn_rows(mean, var, gamma, beta, eps, m1, m2), K)
    close(got, want, "dW")
    assert (mag >= got.abs() - 1e-12).all()


@pytest.mark.parametrize("elu", [0, 1])
@pytest.mark.parametrize("S", [1, 5, 8])
@pytest.mark.parametrize("C,D,F1", [(1, 1, 1), (3, 2, 4), (5, 8, 2)])
def test_spatial_fwd_bwd(C, D, F1, S, elu):
    """BatchNorm affine (-> ELU) -> depthwise Conv2d(F1, D F1, (C,1), groups=F1): g1 is the gradient at the affine's
    output, the two statistics sums are those of the BatchNorm backward, dW the depthwise weight gradient."""
    B, eps = 2, 1e-3
    y1 = rnd(B, F1, C, S)
    mean, var, gamma, beta = rnd(F1), rnd(F1).abs() + 0.5, rnd(F1), rnd(F1)
    bn1 = bn_rows(mean, var, gamma, beta, eps)
    wd, dz = rnd(F1 * D, C).requires_grad_(), rnd(B, F1 * D, S)
    o = (y1 * bn1[2].view(1, -1, 1, 1) + bn1[3].view(1, -1, 1, 1)).requires_grad_()
    a = F.elu(o) if elu else o
    z = F.conv2d(a, wd.view(F1 * D, 1, C, 1), groups=F1).squeeze(2)
    zr, zmag = R.spatial_fwd_ref(y1, bn1, wd.detach(), D, elu)
    close(zr, z.detach(), "z")
    assert (zmag >= zr.abs() - 1e-12).all()
    g_o, g_w = torch.autograd.grad(z, (o, wd), dz)
    r = R.spatial_bwd_ref(y1, dz, bn1, wd.detach(), D, elu)
    close(r["g1"], g_o, "g1")
    close(r["dW"], g_w, "dW")
    xhat = (y1 - mean.view(1, -1, 1, 1)) * bn1[1].view(1, -1, 1, 1)
    close(r["gx"].sum((0, 2, 3)), (g_o * xhat).sum((0, 2, 3)), "sum g1 xhat")
    rows = [(b, 0, S) for b in range(B)]
    close(R.spatial_dw_rows(dz, r["a"], D, rows).sum(0), g_w, "dW rows")
    assert (r["g1_mag"] >= r["g1"].abs() - 1e-12).all() and (r["dW_mag"] >= r["dW"].abs() - 1e-12).all()


@pytest.mark.parametrize("K2", [1, 2, 3, 8, 9])
@pytest.mark.parametrize("T", [1, 5, 7, 12])
def test_sepconv_pointwise_dwt(K2, T):
    """depthwise (1,K2) 'same' conv -> pointwise 1x1 conv, T < K2 included."""
    B, C2, F2 = 2, 3, 5
    a, wdw, wp = rnd(B, C2, T).requires_grad_(), rnd(C2, K2).requires_grad_(), rnd(F2, C2).requires_grad_()
    d3 = F.conv2d(a.unsqueeze(2), wdw.view(C2, 1, 1, K2), padding="same", groups=C2)
    z = F.conv2d(d3, wp.view(F2, C2, 1, 1)).squeeze(2)
    d3r, zr = R.sepconv_fwd_ref(a.detach(), wdw.detach(), wp.detach())
    close(d3r, d3.squeeze(2).detach(), "d3")
    close(zr, z.detach(), "z")
    du = rnd(B, F2, T)
    g_d3, g_wp = torch.autograd.grad(z, (d3, wp), du, retain_graph=True)
    dd3, dwp = R.pointwise_bwd_ref(du, d3r, wp.detach())
    close(dd3, g_d3.squeeze(2), "dd3")
    close(dwp, g_wp, "dWp")
    g_a, g_wdw = torch.autograd.grad(d3, (a, wdw), g_d3)
    da, wpart = R.dwt_bwd_ref(dd3, a.detach(), wdw.detach())
    close(da, g_a, "da")
    close(wpart.sum(0), g_wdw, "dWdw")


@pytest.mark.parametrize("K", [1, 2, 5, 8, 16])
@pytest.mark.parametrize("T", [1, 5, 7, 20])
@pytest.mark.parametrize("Ci,Co", [(1, 3), (3, 1), (4, 5)])
def test_dconv_fwd_transposed_wgrad(Ci, Co, T, K):
    """Dense Conv2d(Ci, Co, (1,K), 'same'): the transposed form is the input gradient with the FORWARD weight; for even K
    its left pad K-1-(K-1)//2 differs from the forward's."""
    B = 2
    x, w = rnd(B, Ci, T).requires_grad_(), rnd(Co, Ci, K).requires_grad_()
    y = F.conv2d(x.unsqueeze(2), w.unsqueeze(2), padding="same").squeeze(2)
    close(R.dconv_fwd_ref(x.detach(), w.detach(), 0), y.detach(), "out")
    dy = rnd(B, Co, T)
    g_x, g_w = torch.autograd.grad(y, (x, w), dy)
    close(R.dconv_fwd_ref(dy, w.detach(), 1), g_x, "din")
    close(R.dconv_wgrad_ref(dy, x.detach(), K).sum(0), g_w, "dW")
