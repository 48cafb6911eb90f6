"""Float64 references of the ShallowConvNet / transformer-glue entry points (csrc/shallow_tf.hip), restated from the
contracts in include/eav_hip.h in plain torch on the CPU, one function per launcher.  Shared by the kernel tests
(test_shallow_tf_kernels_gpu.py) and their CPU self-check against torch autograd (test_shallow_tf_cpu.py).

Backward maps are written out from the formulas, never through autograd.  The linear maps double as their own
"magnitude" (every term replaced by its absolute value): call them on the absolute values of the operands."""
import torch
import torch.nn.functional as F

from tests.audio_conv_ref import f32_scale


def drop_mult(shape, p, mask):
    """The dropout multiplier: mask * 1.f/(1.f-p) (fp32 scale), 1 when p = 0."""
    if p <= 0:
        return torch.ones(shape, dtype=torch.float64)
    return mask.double().reshape(shape) * f32_scale(p)


# ------------------------------------------------------------------------------------------------------ patch embedding
def shallow_embed_fwd_ref(x, wc, wv):
    """eav_shallow_embed_fwd: x [B,C,S], wc [NF,KC], wv [NF,C] -> u[b,f,s] = sum_c wv[f,c] x[b,c,s] and the tokens
    v[b,t,f] = sum_j wc[f,j] u[b,f,t+j], t < S-KC+1."""
    NF, KC = wc.shape
    u = torch.einsum("fc,bcs->bfs", wv.double(), x.double())
    v = F.conv1d(u, wc.double().unsqueeze(1), groups=NF)           # valid cross-correlation per filter
    return u, v.transpose(1, 2).contiguous()


def shallow_embed_bwd_ref(dv, x, u, wc):
    """eav_shallow_embed_bwd (summed over the partial rows): dWc[f,j] = sum_{b,t} dv[b,t,f] u[b,f,t+j];
    dWv[f,c] = sum_{b,s} e[b,f,s] x[b,c,s] with e[b,f,s] = sum_j wc[f,j] dv[b,s-j,f] (dv zero outside [0,T))."""
    NF, KC = wc.shape
    g = dv.double().transpose(1, 2)                                # [B,NF,T]
    uu = u.double().unfold(2, KC, 1)                               # [B,NF,T,KC]: u[t + j]
    dwc = torch.einsum("bft,bftj->fj", g, uu)
    # e[s] = sum_j wc[j] g[s - j]: full convolution = correlation of the (KC-1)-padded g with the flipped taps
    e = F.conv1d(F.pad(g, (KC - 1, KC - 1)), wc.double().flip(1).unsqueeze(1), groups=NF)
    return dwc, torch.einsum("bfs,bcs->fc", e, x.double())


# --------------------------------------------------------------------------------------------------------- element-wise
def relu_dropout_ref(h, p=0.0, mask=None):
    """eav_relu_dropout: Dropout(ReLU(h)); a NaN propagates whatever its keep decision (NaN * 0 = NaN, as in torch)."""
    h = h.double()
    return torch.relu(h) * drop_mult(h.shape, p, mask)


def relu_dropout_bwd_ref(dact, act, p=0.0):
    """eav_relu_dropout_bwd: act is the forward's OUTPUT; the gradient passes with the dropout scale where act > 0 and - as
    torch's ReLU backward passes it at a NaN - where act is NaN; it is zero elsewhere."""
    s = f32_scale(p) if p > 0 else 1.0
    return torch.where((act > 0) | torch.isnan(act), dact.double() * s, torch.zeros_like(dact, dtype=torch.float64))


def dropout_add_ref(y, resid, p=0.0, mask=None):
    """eav_dropout_add: resid + Dropout(y); resid None: Dropout(y)."""
    d = y.double() * drop_mult(y.shape, p, mask)
    return d if resid is None else resid.double() + d


def add_strided_ref(a, b, n):
    """eav_add_strided on host views a [M,lda], b [M,ldb] or None: the first n columns of a (+ b)."""
    o = a[:, :n].double()
    return o if b is None else o + b[:, :n].double()


def colstats_ref(x, N, rows=256):
    """eav_colstats: x [M,ld] -> part [ceil(M/rows), 2N] = column sums | sums of squares of each chunk of `rows` rows."""
    xs = x[:, :N].double()
    return torch.stack([torch.cat([c.sum(0), (c * c).sum(0)]) for c in xs.split(rows)])


# ----------------------------------------------------------------------------------------------------------------- head
def sqpool_ref(v, bn, NP, win, stride):
    """The pre-log means of eav_sqpool_log_fwd: o = scale v + shift, pooled[b,f,p] = mean_{k<win} o[b, p stride + k, f]^2.
    Returns (pooled [B,NF,NP], o [B,T,NF], bound of |o|, magnitude of pooled)."""
    sc, sh = bn[2].double(), bn[3].double()
    o = v.double() * sc + sh
    omag = v.double().abs() * sc.abs() + sh.abs()
    sq = (o * o).transpose(1, 2)                                    # [B,NF,T]
    need = (NP - 1) * stride + win
    pooled = F.avg_pool1d(sq[..., :need], win, stride)
    mag = F.avg_pool1d((omag * omag).transpose(1, 2)[..., :need], win, stride)
    return pooled, o, omag, mag


def sqpool_log_out_ref(pooled, lo, hi, p=0.0, mask=None):
    """out = Dropout(log(clamp(pooled, lo, hi))) flattened to [B, NF*NP]; a NaN mean stays NaN (torch.clamp)."""
    out = torch.log(torch.clamp(pooled.double(), lo, hi)) * drop_mult(pooled.shape, p, mask)
    return out.flatten(1)


def sqpool_log_bwd_ref(dy, pooled, v, bn, NP, win, stride, lo, hi, p=0.0, mask=None):
    """eav_sqpool_log_bwd: g[b,t,f] = dL/do = (2/win) o[b,t,f] sum_{p: p stride <= t < p stride + win} dm[b,f,p],
    dm = dy * dropout / pooled where lo <= pooled <= hi (bounds included, as torch.clamp's backward), else 0;
    part[b] = sum_t g | sum_t g xhat, xhat = (v - mean) invstd.  Returns a dict of values and magnitudes."""
    B, T, NF = v.shape
    mean, invstd, sc, sh = (bn[i].double() for i in range(4))
    m = pooled.double()
    inside = (m >= lo) & (m <= hi)
    dmv = dy.double().view(B, NF, NP) * drop_mult(m.shape, p, mask) / m
    dm = torch.where(inside, dmv, torch.zeros_like(m))
    cover, cmag = torch.zeros(B, NF, T, dtype=torch.float64), torch.zeros(B, NF, T, dtype=torch.float64)
    for q in range(NP):
        cover[..., q * stride:q * stride + win] += dm[..., q:q + 1]
        cmag[..., q * stride:q * stride + win] += dm[..., q:q + 1].abs()
    o = v.double() * sc + sh
    omag = v.double().abs() * sc.abs() + sh.abs()
    g = (2.0 / win) * o * cover.transpose(1, 2)
    gmag = (2.0 / win) * omag * cmag.transpose(1, 2)
    xhat = (v.double() - mean) * invstd
    xmag = (v.double().abs() + mean.abs()) * invstd.abs()
    return {"g": g, "g_mag": gmag, "part": torch.cat([g.sum(1), (g * xhat).sum(1)], 1),
            "part_mag": torch.cat([gmag.sum(1), (gmag * xmag).sum(1)], 1)}


def bn_rows_bwd_ref(g, v, bn):
    """eav_bn_rows_bwd: dx[m,f] = scale_f (g - m1_f - xhat m2_f), xhat = (v - mean_f) invstd_f; bn = mean, invstd, scale,
    shift, m1, m2 [6,NF].  Returns (dx, magnitude)."""
    mean, invstd, scale, _, m1, m2 = (bn[i].double() for i in range(6))
    g, v = g.double(), v.double()
    dx = scale * (g - m1 - (v - mean) * invstd * m2)
    mag = scale.abs() * (g.abs() + m1.abs() + (v.abs() + mean.abs()) * invstd.abs() * m2.abs())
    return dx, mag
