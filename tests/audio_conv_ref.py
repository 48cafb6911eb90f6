"""Float64 references of the audio CNN's three conv entry points (eav_audio_conv5_fwd, _dgrad, _wgrad), restated from
the contracts in include/eav_hip.h in plain torch on the CPU.  Shared by the kernel tests (test_audio_cnn_kernels_gpu.py)
and their CPU self-check against torch autograd (test_audio_cnn_cpu.py)."""
import numpy as np
import torch
import torch.nn.functional as F


def f32_scale(p):
    """The kernels' dropout scale 1.f / (1.f - p), evaluated in fp32."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u) for fp32 (u = 2^-24): the relative bound of an n-term fp32 sum of products."""
    u = 2.0 ** -24
    return n * u / (1.0 - n * u)


def fwd_ref(x, w, b, Lout, pool=0, mask=None, p=0.0):
    """eav_audio_conv5_fwd: ReLU(conv1d(x, w, b, padding 2)), times mask * 1.f/(1.f-p) when p > 0; pool = 1 crops to Lout
    and takes MaxPool1d(8), returning (pooled, offset of the argmax within its window as uint8)."""
    y = F.relu(F.conv1d(x.double(), w.double(), b.double(), padding=2))
    if p > 0:
        y = y * mask.double() * f32_scale(p)
    if not pool:
        return y
    v, i = F.max_pool1d(y[..., :Lout], 8, return_indices=True)
    return v, (i - 8 * torch.arange(Lout // 8)).to(torch.uint8)


def dgrad_ref(dout, w, Lout, gate_in=None, gscale_in=1.0, mode=0, aux=None, idx=None, gscale_out=1.0):
    """eav_audio_conv5_dgrad with w [C][N][5]: din[b][n][t] = sum_{c,tap} w[c][n][tap] g[b][c][t - tap + 2] for t < Lout,
    g = dout * (gate_in > 0 ? gscale_in : 0), zero beyond Lin.  mode 0: zero where aux <= 0 (a NaN aux passes).  mode 1:
    the dense [B][N][8 Lout] gradient holding din * gscale_out at 8 t + idx where aux > 0, zero everywhere else."""
    g = dout.double()
    if gate_in is not None:
        g = g * torch.where(gate_in > 0, gscale_in, 0.0).double()
    Lin = g.shape[2]
    L = max(Lin, Lout)
    d = F.conv_transpose1d(F.pad(g, (0, L - Lin)), w.double(), padding=2)[..., :Lout]
    if mode == 0:
        return d if aux is None else torch.where(aux <= 0, 0.0, d)
    gv = torch.where(aux > 0, d * gscale_out, 0.0)
    out = torch.zeros(*d.shape, 8, dtype=torch.float64)
    out.scatter_(3, idx.long().unsqueeze(3), gv.unsqueeze(3))
    return out.flatten(2)


def wgrad_ref(dout, act, gate=None, gscale=1.0):
    """eav_audio_conv5_wgrad + eav_reduce_partials: dW[m][c][tap] = sum_{b,t < Lout} g[b][m][t] act[b][c][t + tap - 2]
    and db[m] = sum_{b,t} g[b][m][t], g = dout * (gate > 0 ? gscale : 0), act zero outside [0, Lact)."""
    g = dout.double()
    if gate is not None:
        g = g * torch.where(gate > 0, gscale, 0.0).double()
    B, Cact, Lact = act.shape
    Lout = g.shape[2]
    ext = torch.zeros(B, Cact, Lout + 4, dtype=torch.float64)
    n = min(Lact, Lout + 2)
    ext[..., 2:2 + n] = act[..., :n].double()
    dw = torch.einsum("bmt,bctk->mck", g, ext.unfold(2, 5, 1))
    return dw, g.sum((0, 2))
