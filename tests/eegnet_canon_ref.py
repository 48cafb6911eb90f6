"""Float64 references of the canonical-EEGNet entry points (csrc/eegnet_canon.hip), restated from the contracts in
include/eav_hip.h in plain torch on the CPU, one function per launcher.  Shared by the kernel tests
(test_eegnet_canon_kernels_gpu.py) and their CPU self-check against torch autograd (test_eegnet_canon_cpu.py).

Forward maps are written with F.conv1d on explicitly padded inputs (torch's 'same' rule: (K-1)//2 zeros on the left, the
rest on the right); backward maps are written out from the formulas, never through autograd.  The linear maps double as
their own "magnitude" (the sum with every term replaced by its absolute value): call them on the absolute values of the
operands.  The maps with a BatchNorm or an ELU inside return the magnitude themselves."""
import torch
import torch.nn.functional as F


def same_pad(K):
    """torch's padding='same' for a stride-1 conv of K taps: (left, right)."""
    return (K - 1) // 2, K - 1 - (K - 1) // 2


def elu64(o):
    return torch.where(o > 0, o, torch.expm1(torch.clamp(o, max=0.0)))


def stats(y, dims):
    """(sum, sum of squares) over dims: the two halves of a BatchNorm statistics row."""
    y = y.double()
    return y.sum(dims), (y * y).sum(dims)


# ------------------------------------------------------------------------------------------------------- block1[0]
def tconv_fwd_ref(x, w):
    """eav_tconv_fwd: x [B,C,S], w [F1,K] -> y1 [B,F1,C,S] = Conv2d(1,F1,(1,K),'same') applied to every electrode row."""
    B, C, S = x.shape
    F1, K = w.shape
    xp = F.pad(x.double().reshape(B * C, 1, S), same_pad(K))
    return F.conv1d(xp, w.double().unsqueeze(1)).view(B, C, F1, S).permute(0, 2, 1, 3).contiguous()


def bn_fold(y1, g1, bn):
    """The BatchNorm input gradient folded into eav_tconv_wgrad: dy = scale (g1 - m1 - xhat m2), xhat = (y1 - mean)
    invstd, bn = mean, invstd, scale, shift, m1, m2 [6,F1].  Returns (dy, its magnitude)."""
    mean, invstd, scale, _, m1, m2 = (bn[i].double().view(1, -1, 1, 1) for i in range(6))
    y1, g1 = y1.double(), g1.double()
    dy = scale * (g1 - m1 - (y1 - mean) * invstd * m2)
    mag = scale.abs() * (g1.abs() + m1.abs() + (y1.abs() + mean.abs()) * invstd.abs() * m2.abs())
    return dy, mag


def corr_wgrad(dy, x, K):
    """dW[f,j] = sum_{b,c,t} dy[b,f,c,t] x[b,c,t+j-padl] (x zero outside), as one correlation per filter."""
    B, F1, C, S = dy.shape
    xp = F.pad(x.double(), same_pad(K)).reshape(1, B * C, S + K - 1)
    return F.conv1d(xp, dy.permute(1, 0, 2, 3).reshape(F1, B * C, S))[0]


def tconv_wgrad_ref(x, y1, g1, bn, K):
    """eav_tconv_wgrad (summed over its partial rows): (dW [F1,K], magnitude)."""
    dy, mag = bn_fold(y1, g1, bn)
    return corr_wgrad(dy, x, K), corr_wgrad(mag, x.abs(), K)


# ---------------------------------------------------------------------------------------------------- block1[1..2]
def bn1_out(y1, bn1, elu, f32_elu=False):
    """(o, a, |o| bound): o = scale y1 + shift per filter, a = ELU(o) or o.  f32_elu rounds ELU(o) to fp32: the value a
    correctly rounded fp32 ELU returns, for data on which the kernels' ELU is exact (o > 0, o = 0, o <= -17.5)."""
    sc, sh = bn1[2].double().view(1, -1, 1, 1), bn1[3].double().view(1, -1, 1, 1)
    o = sc * y1.double() + sh
    a = elu64(o) if elu else o
    return o, (a.float().double() if f32_elu else a), sc.abs() * y1.double().abs() + sh.abs()


def spatial_fwd_ref(y1, bn1, wd, D, elu, f32_elu=False):
    """eav_spatial_fwd: y1 [B,F1,C,S], wd [F1*D,C] -> z [B,F1*D,S] = sum_c wd[f D + d, c] a[b,f,c,t].
    Returns (z, magnitude) with |a| bounded by |scale||y1| + |shift| (ELU is 1-Lipschitz with ELU(0) = 0)."""
    B, F1, C, S = y1.shape
    _, a, omag = bn1_out(y1, bn1, elu, f32_elu)
    w = wd.double().view(F1, D, C)
    z = torch.einsum("fdc,bfct->bfdt", w, a).reshape(B, F1 * D, S)
    return z, torch.einsum("fdc,bfct->bfdt", w.abs(), omag).reshape(B, F1 * D, S)


def spatial_bwd_ref(y1, dz, bn1, wd, D, elu, f32_elu=False):
    """eav_spatial_bwd: g1 [B,F1,C,S] = dL/d(BN output) = ELU'(o) sum_d wd[fd,c] dz[b,fd,t] (ELU' = 1 for o > 0, ELU(o) + 1
    otherwise; 1 without the ELU); per-(b, tile) statistics rows are sums of g1 and g1 xhat (xhat = (y1 - mean) invstd)
    over (c, t); dW [F1*D,C] = sum_{b,t} dz[b,fd,t] a[b,f,c,t].  Returns a dict of values and magnitudes (g1_lin_mag: the
    magnitude of the sum before the ELU slope)."""
    B, F1, C, S = y1.shape
    o, a, omag = bn1_out(y1, bn1, elu, f32_elu)
    w = wd.double().view(F1, D, C)
    dzv = dz.double().view(B, F1, D, S)
    gin = torch.einsum("fdc,bfdt->bfct", w, dzv)
    glin = torch.einsum("fdc,bfdt->bfct", w.abs(), dzv.abs())
    slope = torch.where(o > 0, torch.ones_like(o), a + 1.0) if elu else torch.ones_like(o)
    gin, gmag = gin * slope, glin * slope
    mean, invstd = bn1[0].double().view(1, -1, 1, 1), bn1[1].double().view(1, -1, 1, 1)
    xhat = (y1.double() - mean) * invstd
    xmag = (y1.double().abs() + mean.abs()) * invstd.abs()
    return {"g1": gin, "g1_mag": gmag, "g1_lin_mag": glin, "slope": slope, "omag": omag, "xmag": xmag, "gx": gin * xhat,
            "gx_mag": gmag * xmag,
            "dW": torch.einsum("bfdt,bfct->fdc", dzv, a).reshape(F1 * D, C),
            "dW_mag": torch.einsum("bfdt,bfct->fdc", dzv.abs(), omag).reshape(F1 * D, C), "a": a}


def spatial_dw_rows(dz, a, D, rows):
    """w_part rows of eav_spatial_bwd: rows = list of (b, t0, t1); returns [len(rows), F1*D, C]."""
    B, F1, C, S = a.shape
    dzv = dz.double().view(B, F1, D, S)
    return torch.stack([torch.einsum("fdt,fct->fdc", dzv[b, :, :, t0:t1], a[b, :, :, t0:t1]).reshape(F1 * D, C)
                        for b, t0, t1 in rows])


# ---------------------------------------------------------------------------------------------------------- block2
def dw_same(a, wdw):
    """depthwise (1,K2) 'same' conv: d3[b,ch,t] = sum_k wdw[ch,k] a[b,ch,t+k-padl]."""
    C2, K2 = wdw.shape
    return F.conv1d(F.pad(a.double(), same_pad(K2)), wdw.double().unsqueeze(1), groups=C2)


def sepconv_fwd_ref(a, wdw, wp):
    """eav_sepconv_fwd: a [B,C2,T], wdw [C2,K2], wp [F2,C2] -> (d3 [B,C2,T], z [B,F2,T])."""
    d3 = dw_same(a, wdw)
    return d3, torch.einsum("oc,bct->bot", wp.double(), d3)


def pointwise_bwd_ref(du, d3, wp):
    """eav_pointwise_bwd: dd3[b,ch,t] = sum_o wp[o,ch] du[b,o,t]; dWp[o,ch] = sum_{b,t} du[b,o,t] d3[b,ch,t]."""
    du, d3 = du.double(), d3.double()
    return torch.einsum("oc,bot->bct", wp.double(), du), torch.einsum("bot,bct->oc", du, d3)


def dwt_bwd_ref(dd3, a, wdw):
    """eav_dwt_bwd: da[b,ch,t] = sum_k wdw[ch,k] dd3[b,ch,t-k+padl]; w_part[b][ch,k] = sum_t dd3[b,ch,t] a[b,ch,t+k-padl]
    (both zero outside [0,T)).  Returns (da, w_part [B,C2,K2])."""
    C2, K2 = wdw.shape
    pl, pr = same_pad(K2)
    # gu[..., t, i] = dd3[t + i - pr]; with i = K2-1-k this is dd3[t - k + pl]
    gu = F.pad(dd3.double(), (pr, pl)).unfold(2, K2, 1)
    da = torch.einsum("bcti,ci->bct", gu, wdw.double().flip(1))
    au = F.pad(a.double(), (pl, pr)).unfold(2, K2, 1)              # au[..., t, k] = a[t + k - pl]
    return da, torch.einsum("bct,bctk->bck", dd3.double(), au)


# -------------------------------------------------------------------------------- dense temporal conv (EEGNet_tor widths)
def dconv_fwd_ref(inp, w, transposed):
    """eav_dconv_fwd.  transposed = 0: in [B,Cin,T], w [Cout,Cin,K] -> out[b,o,t] = sum_{ci,k} w[o,ci,k] in[b,ci,t+k-padl].
    transposed = 1: in = dL/dout [B,Cin,T], w = the FORWARD weight [Cin,Cout,K] -> dL/din[b,co,u] = sum_{ci,k} w[ci,co,k]
    in[b,ci,u-k+padl]."""
    K = w.shape[2]
    pl, pr = same_pad(K)
    if not transposed:
        return F.conv1d(F.pad(inp.double(), (pl, pr)), w.double())
    # (pad (pr, pl)) [t + i] = in[t + i - pr]; tap i of the flipped, transposed weight is w[ci,co,K-1-i]: in[t - k + pl]
    return F.conv1d(F.pad(inp.double(), (pr, pl)), w.double().transpose(0, 1).flip(2))


def dconv_wgrad_ref(dy, x, K):
    """eav_dconv_wgrad: part[b][o,ci,k] = sum_t dy[b,o,t] x[b,ci,t+k-padl] -> [B,Cout,Cin,K]."""
    xu = F.pad(x.double(), same_pad(K)).unfold(2, K, 1)
    return torch.einsum("bot,bctk->bock", dy.double(), xu)
