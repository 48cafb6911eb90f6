"""float64 numpy restatement of the per-trial input tables of the FFT FIR weight gradient (csrc/eegnet_fir_fft.hip, "wgrad
from per-trial input tables") - shared by test_fir_xtab_cpu.py and test_fir_xtab_gpu.py.

    left = (K - 1) // 2, xp = the row zero-padded by (left, K - 1 - left)
    y[b,f,c,t]  = sum_j w[f,j] xp[b,c,t+j]
    dW[f,k]     = sum_{b,c,t<S} dy[b,f,c,t] xp[b,c,t+k],   dy = scale (g - m1 - (y - mean) invstd m2)
                = scale_f (G[f,k] - (m1_f - mean_f invstd_f m2_f) X1[k] - invstd_f m2_f Y[f,k])
    G[f,k]      = sum_{b,c,t<S} g[b,f,c,t] xp[b,c,t+k]
    X1[k]       = sum_b X1_b[k],  X1_b[k]   = sum_c sum_{t<S} xp[t+k]
    Y[f,k]      = sum_j w[f,j] A[j,k],  A = sum_b A_b,  A_b[j,k] = sum_c sum_{t<S} xp[t+j] xp[t+k]
Table layout: per trial K K + K values - A_b row-major, then X1_b."""
import numpy as np


def padded(x, K):
    """x [..., S] -> xp [..., S + K - 1] in float64"""
    left = (K - 1) // 2
    pad = [(0, 0)] * (x.ndim - 1) + [(left, K - 1 - left)]
    return np.pad(np.asarray(x, np.float64), pad)


def windows(x, K):
    """win[..., k, t] = xp[..., t + k], t < S"""
    S = x.shape[-1]
    return np.lib.stride_tricks.sliding_window_view(padded(x, K), S, axis=-1)


def tables_direct(x, K):
    """x [N,C,S] -> (A [N,K,K], X1 [N,K]) from the definition."""
    win = windows(x, K)                                   # [N,C,K,S]
    N, C = x.shape[:2]
    A = np.zeros((N, K, K))
    for n in range(N):
        for c in range(C):                                # (one K x S window matrix at a time: a row's Gram matrix)
            wc = np.ascontiguousarray(win[n, c])
            A[n] += wc @ wc.T
    return A, win.sum((1, 3))


def tables_autocorr(x, K):
    """The same tables as the builder forms them: per lag d one autocorrelation sum R over the whole row, and the diagonal
    A[j, j+d] = R - (products of the first j samples) + (products of the j samples from S on)."""
    N, C, S = x.shape
    xp = np.concatenate([padded(x, K), np.zeros((N, C, K))], -1)      # (reads of u + d stay below S + K - 1: zeros are never used)
    A, X1 = np.zeros((N, K, K)), np.zeros((N, K))
    for d in range(K):
        prod = xp[..., :S + K] * xp[..., d:d + S + K]                 # prod[u] = xp[u] xp[u+d]
        R = prod[..., :S].sum((1, 2))
        X1[:, d] = xp[..., d:d + S].sum((1, 2))
        nj = K - d
        step = (prod[..., S:S + nj] - prod[..., :nj]).sum(1)          # [N, nj]
        diag = R[:, None] + np.concatenate([np.zeros((N, 1)), np.cumsum(step, 1)[:, :-1]], 1)
        j = np.arange(nj)
        A[:, j, j + d] = diag
        A[:, j + d, j] = diag
    return A, X1


def flat_tables(A, X1):
    """[N, K K + K]: the layout of eav_eegnet_fir_xtab_build"""
    N, K = X1.shape
    return np.concatenate([A.reshape(N, K * K), X1], 1)


def conv_same(x, w):
    """y [B,F,C,S] = firstConv(x [B,C,S]; w [F,K]) in float64"""
    return np.einsum("fk,bcks->bfcs", np.asarray(w, np.float64), windows(x, w.shape[1]))


def wgrad_direct(x, y, g, mean, invstd, scale, m1, m2, K):
    """The reference of test_fir_wgrad_fft: dy formed per element, then the einsum."""
    bc = lambda v: np.asarray(v, np.float64)[None, :, None, None]  # noqa: E731
    dy = bc(scale) * (np.asarray(g, np.float64) - bc(m1) - (np.asarray(y, np.float64) - bc(mean)) * bc(invstd) * bc(m2))
    return np.einsum("bfcs,bcks->fk", dy, windows(x, K))


def wgrad_from_tables(x, w, g, mean, invstd, scale, m1, m2, A, X1, idx=None):
    """The identity: x [N,C,S] the data set, idx the batch (None: all of it, in order); A / X1 the per-trial tables."""
    K = w.shape[1]
    idx = np.arange(x.shape[0]) if idx is None else np.asarray(idx)
    f64 = lambda v: np.asarray(v, np.float64)  # noqa: E731
    G = np.einsum("bfcs,bcks->fk", f64(g), windows(x[idx], K))
    As, X1s = np.zeros((K, K)), np.zeros(K)
    for b in idx:                                                     # repeated indices count as often as they occur
        As += A[b]
        X1s += X1[b]
    Y = f64(w) @ As
    c1 = f64(m1) - f64(mean) * f64(invstd) * f64(m2)
    c2 = f64(invstd) * f64(m2)
    return f64(scale)[:, None] * (G - c1[:, None] * X1s[None, :] - c2[:, None] * Y)
