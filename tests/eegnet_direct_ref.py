"""Float64 references of the direct (non-FFT) EEGNet_tor kernels - csrc/eegnet_fir.hip, csrc/eegnet_block.hip,
csrc/eegnet_conv64.hip - restated in plain torch on the CPU from the PyTorch semantics quoted in the kernel headers, one
function per operation; plus the input sets, the case lists, the launch geometry restated from the documented thresholds
and the rounding bounds that test_eegnet_direct_kernels_gpu.py uses.  test_eegnet_direct_ref_cpu.py pins every reference
to torch autograd in double and checks the case lists and the exactness conditions without a device.

Two data modes for every case.

"exact": inputs are small integers, weights small integers, BatchNorm constants integers or powers of two, dropout p 0.5
or 0.75 (multiplier 2 or 4), and the BatchNorm shifts are large enough that every pre-activation is >= 0: ELU is the
identity there and ELU' = 1 (elu_f(0) = 0 and elu_grad_from_out(0, 0) = 1 exactly).  Every product and every partial sum,
in any order, is then a multiple of a quantum q with magnitude <= sum |terms|, hence exact in fp32 while
sum |terms| < 2^24 q: the kernel must return the float64 value bit for bit.  Every reference returns its (sum |terms|, q)
pairs under "exact" and its smallest pre-activation under "min_pre"; the CPU test asserts both for every case.  Statistics
are compared after the partial rows were added in float64 on the host, so their condition is on the total of the absolute
values that are summed (it bounds every partial sum of every block).

"rounded": normal data, pre-activations on both sides of zero, general BatchNorm constants.  Each reference returns the
float64 value and a first-order bound propagated stage by stage.  With u = 2^-24 a sum of n fp32 terms accumulated by fma
(the MFMA chains; one rounding per term) or by multiply-then-add (two), in any order, is within
n_roundings * u * sum |terms| of the true sum to first order (Higham, Accuracy and Stability, section 3.1); rb() adds c = 1
to n, which covers the second-order term for every chain shorter than 4096.  Errors of a stage's inputs pass through the
linear maps with the absolute weights, through ELU with Lipschitz constant 1 and through ELU' = exp(min(o, 0)) with
Lipschitz constant 1.  elu_f is within 1.5 ulp (tests/test_eegnet_kernels_gpu.py asserts it): 1.5 * 2^-23 |a| = 3 u |a|.
elu_fast (the inference kernel) is allowed 2^-22 absolute: 2^-23 for the Taylor truncation plus eight fma roundings on
(-0.5, 0], or one native exp and one subtraction below, doubled because the native exp's accuracy is not measured here.
The chain lengths n of every kernel are derived beside the reference that uses them."""
import numpy as np
import torch
import torch.nn.functional as F

from eav_amd import synth
from tests.kernel_check import ints, normal, seed_of

U = 2.0 ** -24
ELU_ULP = 3.0 * U                 # 1.5 ulp of elu_f, relative to |ELU(o)|
ELU_FAST_ABS = 2.0 ** -22         # elu_fast, absolute
F1, DD, NCH = 8, 8, 64
MODES = ["exact", "rounded"]


def cdiv(a, b):
    return -(-a // b)


def rb(n, mag, c=1):
    """First-order bound of n roundings on partial sums bounded by mag."""
    return (n + c) * U * mag


def same_pad(K):
    """torch's padding='same' for a stride-1 conv of K taps: (left, right)."""
    return (K - 1) // 2, K - 1 - (K - 1) // 2


def elu64(o):
    return torch.where(o > 0, o, torch.expm1(torch.clamp(o, max=0.0)))


def slope64(o):
    """ELU'(o) = 1 for o > 0, ELU(o) + 1 = exp(o) otherwise."""
    return torch.exp(torch.clamp(o, max=0.0))


def pick(seed, n, values):
    v = np.asarray(values, np.float32)
    return torch.from_numpy(v[(synth.splitmix64(seed, n) % np.uint64(len(values))).astype(np.int64)])


def uniform(seed, shape, lo, hi):
    return torch.from_numpy(synth.uniform(seed, shape, lo, hi))


def chunk_sum(a, width=1024):
    """[..., S] -> [..., ceil(S / width)]: sums over consecutive blocks of `width` samples (the rows of the block-1 partial
    buffers)."""
    S = a.shape[-1]
    n = cdiv(S, width)
    return F.pad(a, (0, n * width - S)).reshape(*a.shape[:-1], n, width).sum(-1)


# ------------------------------------------------------------------------------------------- launch geometry
# Restated from the thresholds documented in include/eav_hip.h and the kernel headers; the GPU test asserts that the
# plan queries of the library return the same numbers.
def fir_nstep(klen):
    return 34 if klen <= 65 else 66 if klen <= 129 else 152


def fir_nseg(S):
    return cdiv(cdiv(S, 128), 16)              # 16 tiles of 128 samples per forward work item


def fir_fwd_grid(B, C, S):
    return min(B * C * fir_nseg(S), 512)


def wgrad_geometry(S):
    """(nchunk, CH): items of at most 248 samples over S + 1 positions (the odd lags need dy[S-1] at u = S), CH a multiple
    of 8."""
    n = cdiv(S + 1, 248)
    return n, cdiv(cdiv(S + 1, n), 8) * 8


def wgrad_nt(klen):
    return 2 if klen <= 64 else 4 if klen <= 128 else 10


def wgrad_grid(B, C, S):
    return min(B * C * wgrad_geometry(S)[0], 768)


def infer_nseg(S):
    return cdiv(cdiv(S, 128), 4)               # 4 tiles (one per wave) per inference work item


def infer_grid(B, S):
    return min(B * infer_nseg(S), 256)


def dw_plan(S):
    return 4256 if S <= 256 else 4512 if S <= 512 else 1256


def conv64_tile(B, T):
    return 32 if B * cdiv(T, 128) < 128 else 128


def conv64_fwd_grid(B, T):
    return min(B * cdiv(T, conv64_tile(B, T)), 256)


def conv64_wgrad_grid(B, T):
    return min(B * cdiv(T, 128), 192)


# ------------------------------------------------------------------------------------------------ BatchNorm blocks
def bn_block(mode, seed, nch, lift=0.0):
    """[6, nch]: mean, invstd, scale, shift, m1, m2 - the block eav_bn_finalize / eav_bn_bwd_finalize leave (the first four
    rows are what eav_bn_finalize(training = 0) writes from the running statistics).  exact: integers / powers of two with
    invstd * m2 an integer, shift = lift (large enough for the pre-activations of the case to stay >= 0)."""
    if mode == "exact":
        return torch.stack([ints(seed, (nch,), -1, 2), pick(seed + 1, nch, [1.0, 0.5]), pick(seed + 2, nch, [1.0, 2.0]),
                            torch.full((nch,), float(lift)), ints(seed + 3, (nch,), -1, 1),
                            2.0 * ints(seed + 4, (nch,), -1, 1)])
    mean, invstd = uniform(seed, (nch,), -0.2, 0.2), uniform(seed + 1, (nch,), 0.5, 2.0)
    gamma, beta = uniform(seed + 2, (nch,), 0.5, 1.5), uniform(seed + 3, (nch,), -0.2, 0.2)
    scale = gamma * invstd
    return torch.stack([mean, invstd, scale, beta - mean * scale, uniform(seed + 4, (nch,), -0.1, 0.1),
                        uniform(seed + 5, (nch,), -0.1, 0.1)])


def _bc(v, nd):
    """[nch] -> broadcast over [B, nch, ...] with nd trailing dims."""
    return v.double().view(1, -1, *([1] * nd))


# ----------------------------------------------------------------------------------------------------- firstConv
def sparse_taps(seed, K):
    """[8, K] integer taps, non-zero at tap 0, tap K - 1 and two inside: both ends of the window are hit while the sums of
    squares stay small."""
    pos = sorted({0, K - 1, K // 2, K // 3})
    w = torch.zeros(F1, K)
    w[:, pos] = pick(seed, F1 * len(pos), [-2.0, -1.0, 1.0, 2.0]).view(F1, len(pos))
    return w


def batch_index(B):
    """B rows of a resident array of 3 B samples: starts at the last row (so it is not monotone), and repeats one row."""
    idx = [(5 * i + 3 * B - 1) % (3 * B) for i in range(B)]
    if B >= 3:
        idx[B - 1] = idx[0]
    return torch.tensor(idx, dtype=torch.int64)


def fir_inputs(mode, B, C, S, K):
    """(resident array [3B, C, S], batch index [B], taps [8, K])."""
    seed = seed_of("fir", mode, B, C, S, K)
    if mode == "exact":
        return ints(seed, (3 * B, C, S), -2, 2), batch_index(B), sparse_taps(seed + 1, K)
    return normal(seed, (3 * B, C, S)), batch_index(B), uniform(seed + 1, (F1, K), -0.1, 0.1)


def unfold_same(x, K):
    """[..., S] -> [..., S, K]: window t holds x[t + k - padl], zero outside (Conv2d(1, 8, (1, K), padding='same'))."""
    return F.pad(x, same_pad(K)).unfold(-1, K, 1)


def fir_fwd_ref(x, w, visits=1):
    """eav_eegnet_fir_fwd: y1[b,f,c,t] = sum_k w[f,k] x[b,c,t+k-(K-1)//2], and the per-filter sum / sum of squares.
    Rounding: y is one MFMA fma chain over the K non-zero taps -> (K + 1) u sum |w||x|.  Statistics: a lane adds the four
    samples of a (filter, tile) as (v0 + v1) + (v2 + v3) (2 roundings on an element's path), accumulates it once per tile it
    visits (`visits` = 4 tiles per work item x the work items of a block), then half_sum (5) and the four waves (2): an
    element's path has visits + 9 additions; the squares add one rounding each (or none, contracted), and an error dy of y
    moves y^2 by 2 |y| dy.  The partial rows are added in float64 by the test."""
    B, C, S = x.shape
    K = w.shape[1]
    xu = unfold_same(x.double(), K).reshape(B * C * S, K)
    wt = w.double().t()
    y = (xu @ wt).view(B, C, S, F1).permute(0, 3, 1, 2).contiguous()
    mag = (xu.abs() @ wt.abs()).view(B, C, S, F1).permute(0, 3, 1, 2).contiguous()
    yb = rb(K, mag)
    d = (0, 2, 3)
    return {"y": y, "y_bound": yb, "s": y.sum(d), "q": (y * y).sum(d),
            "s_bound": yb.sum(d) + rb(visits + 9, y.abs().sum(d)),
            "q_bound": (2 * y.abs() * yb).sum(d) + rb(visits + 10, (y * y).sum(d)),
            "exact": [(float(mag.max()), 1.0, "y1"), (float(y.abs().sum(d).max()), 1.0, "sum y1"),
                      (float((y * y).sum(d).max()), 1.0, "sum y1^2")]}


def fir_fwd_visits(B, C, S):
    return 4 * cdiv(B * C * fir_nseg(S), fir_fwd_grid(B, C, S))


def bn_fold(y1, g1, bn, train):
    """The BatchNorm input gradient formed while the weight-gradient kernel stages dy: train: dy = scale (g1 - m1 - (y1 -
    mean) invstd m2) (6 roundings, every intermediate bounded by the magnitude returned); eval (y1 == NULL): dy = scale g1
    (1 rounding).  Returns (dy, magnitude, roundings)."""
    mean, invstd, scale, _, m1, m2 = (_bc(bn[i], 2) for i in range(6))
    g1 = g1.double()
    if not train:
        return scale * g1, scale.abs() * g1.abs(), 1
    y1 = y1.double()
    dy = scale * (g1 - m1 - (y1 - mean) * invstd * m2)
    return dy, scale.abs() * (g1.abs() + m1.abs() + (y1.abs() + mean.abs()) * invstd.abs() * m2.abs()), 6


def corr_direct(dy, x, K):
    """dW[f,k] = sum_{b,c,t} dy[b,f,c,t] x[b,c,t+k-padl] (x zero outside): autograd's weight gradient of the 'same' conv."""
    B, Fn, C, S = dy.shape
    xu = unfold_same(x.double(), K).reshape(B * C * S, K)
    return dy.double().permute(1, 0, 2, 3).reshape(Fn, B * C * S) @ xu


def corr_fft(dy, x, K):
    """The same correlation through one real FFT per row (zero-padded to >= S + K - 1: the K lags never wrap), summed over
    the rows in the frequency domain.  Pinned to corr_direct in the CPU test; its own error, ~1e-15 of sum |terms|, is nine
    orders below the fp32 bounds, and in exact mode the result is rounded to the quantum it is known to be a multiple of."""
    B, Fn, C, S = dy.shape
    n = 1 << int(np.ceil(np.log2(S + K - 1)))
    X = torch.fft.rfft(F.pad(x.double(), same_pad(K)).reshape(B * C, S + K - 1), n)
    out = []
    for f in range(Fn):
        D = torch.fft.rfft(dy[:, f].double().reshape(B * C, S), n)
        out.append(torch.fft.irfft((D.conj() * X).sum(0), n)[:K])
    return torch.stack(out)


FFT_ABOVE = 4.0e7          # B C S K beyond which the weight-gradient reference takes corr_fft


def fir_wgrad_chain(B, C, S):
    """Longest fma chain of one dW element: a wave owns cdiv(items, waves) work items of CH positions each (4 per MFMA
    K-step, zero padding included), then the four waves of a block meet in LDS (3 additions); the partial rows of the
    blocks are added in float64 by the test."""
    nchunk, CH = wgrad_geometry(S)
    return cdiv(B * C * nchunk, 4 * wgrad_grid(B, C, S)) * CH + 3


def fir_wgrad_ref(x, y1, g1, bn, K, train, mode="rounded"):
    """eav_eegnet_fir_wgrad summed over its partial rows: (dW [8, K], bound, exactness pairs).  Bound: the chain of
    fir_wgrad_chain() terms plus the roundings of dy."""
    B, C, S = x.shape
    dy, mag, nr = bn_fold(y1, g1, bn, train)
    fft = B * C * S * K > FFT_ABOVE
    corr = corr_fft if fft else corr_direct
    dW, dWmag = corr(dy, x, K), corr(mag, x.abs(), K)
    if fft and mode == "exact":
        dW = torch.round(dW)                  # exact mode: dy and x are integers
    return {"dW": dW, "bound": rb(fir_wgrad_chain(B, C, S) + nr, dWmag), "exact": [(float(dWmag.max()), 1.0, "dW1")]}


def fir_wgrad_inputs(mode, B, C, S, K):
    """(resident x [3B, C, S], index, y1, g1 [B, 8, C, S], bn [6, 8]); exact: integers in [-1, 1], so that the 825 344 terms
    of one dW element of the largest case stay below 2^24 in absolute sum."""
    seed = seed_of("firwg", mode, B, C, S, K)
    sh = (B, F1, C, S)
    if mode == "exact":
        return (ints(seed, (3 * B, C, S), -1, 1), batch_index(B), ints(seed + 1, sh, -1, 1), ints(seed + 2, sh, -1, 1),
                bn_block(mode, seed + 3, F1))
    return normal(seed, (3 * B, C, S)), batch_index(B), normal(seed + 1, sh), normal(seed + 2, sh), bn_block(mode, seed + 3, F1)


# ------------------------------------------------------------------------------------------- block-1 inference
def block1_inputs(mode, B, C, S, K):
    """(resident x, index, w1 [8, K], bn1 [6, 8], w2 [64, C], bn2 [6, 64]); exact: |y1| <= 2 * 2 * 4 taps = 16, scale <= 2
    -> shift 32 keeps o1 in [0, 64]; |z| <= 64 C, scale <= 2 -> shift 128 C keeps o2 >= 0."""
    seed = seed_of("infer", mode, B, C, S, K)
    if mode == "exact":
        return (ints(seed, (3 * B, C, S), -2, 2), batch_index(B), sparse_taps(seed + 1, K), bn_block(mode, seed + 2, F1, 32.0),
                ints(seed + 3, (NCH, C), -1, 1), bn_block(mode, seed + 4, NCH, 128.0 * C))
    return (normal(seed, (3 * B, C, S)), batch_index(B), uniform(seed + 1, (F1, K), -0.1, 0.1), bn_block(mode, seed + 2, F1),
            uniform(seed + 3, (NCH, C), -0.3, 0.3), bn_block(mode, seed + 4, NCH))


def block1_infer_ref(x, w1, bn1, w2, bn2):
    """eav_eegnet_block1_infer: p2[b,fd,t/4] = mean of 4 of ELU(bn2(sum_c w2[fd,c] ELU(bn1(FIR_f(x[b,c,:]))))), both
    BatchNorms as scale * v + shift.  Stage by stage, as the kernel computes it:
      y   MFMA chain over K taps                         e_y  = (K + 1) u sum |w1||x|
      o1  fmaf(sc1, y, sh1): 1 rounding                  e_o1 = |sc1| e_y + u (|sc1||y| + |sh1|)
      a1  elu_fast                                       e_a1 = e_o1 + 2^-22
      z   fma chain over the C electrodes                e_z  = sum |w2| e_a1 + (C + 1) u sum |w2||a1|
      o2  fmaf(s2, z, h2)                                e_o2 = |s2| e_z + u (|s2||z| + |h2|)
      a2  elu_f                                          e_a2 = e_o2 + 3 u |a2|
      p   0.25 ((a + a) + (a + a)): 2 additions per path e_p  = 0.25 (sum e_a2 + 2 u sum |a2|)   (x 0.25 is exact)"""
    B, C, S = x.shape
    K = w1.shape[1]
    r = fir_fwd_ref(x, w1)
    y, ey, ymag = r["y"], r["y_bound"], r["exact"][0][0]
    sc1, sh1 = _bc(bn1[2], 2), _bc(bn1[3], 2)
    o1 = sc1 * y + sh1
    o1mag = sc1.abs() * y.abs() + sh1.abs()
    a1 = elu64(o1)
    ea1 = sc1.abs() * ey + U * o1mag + ELU_FAST_ABS
    w = w2.double().view(F1, DD, C)
    z = torch.einsum("fdc,bfct->bfdt", w, a1).reshape(B, NCH, S)
    zmag = torch.einsum("fdc,bfct->bfdt", w.abs(), a1.abs()).reshape(B, NCH, S)
    ez = torch.einsum("fdc,bfct->bfdt", w.abs(), ea1).reshape(B, NCH, S) + rb(C, zmag)
    s2, h2 = _bc(bn2[2], 1), _bc(bn2[3], 1)
    o2 = s2 * z + h2
    a2 = elu64(o2)
    ea2 = s2.abs() * ez + U * (s2.abs() * z.abs() + h2.abs()) + ELU_ULP * a2.abs()
    pool = lambda v: v.view(B, NCH, S // 4, 4).sum(-1)  # noqa: E731
    return {"p": 0.25 * pool(a2), "bound": 0.25 * (pool(ea2) + 2 * U * pool(a2.abs())),
            "min_pre": min(float(o1.min()), float(o2.min())),
            "exact": [(ymag, 1.0, "y1"), (float(zmag.max()), 1.0, "z"), (float(pool(o2.abs()).max()), 1.0, "pool")]}


# ------------------------------------------------------------------------------------------------ separableConv
def conv64_inputs(mode, B, T):
    """(x [B,64,T], w [64,64,16], du [B,64,T]); exact: three weights in four are zero, so that the sums of squares of the
    largest case stay below 2^24."""
    seed = seed_of("conv64", mode, B, T)
    if mode == "exact":
        w = ints(seed + 1, (NCH, NCH, 16), -1, 1) * (ints(seed + 2, (NCH, NCH, 16), 0, 3) == 0).float()
        return ints(seed, (B, NCH, T), -2, 2), w, ints(seed + 3, (B, NCH, T), -2, 2)
    return normal(seed, (B, NCH, T)), uniform(seed + 1, (NCH, NCH, 16), -0.05, 0.05), normal(seed + 3, (B, NCH, T))


def conv64_unfold(x, padl):
    """[B,64,T] -> [B T, 1024]: row (b, t), column i * 16 + k holds x[b, i, t + k - padl], zero outside."""
    B, _, T = x.shape
    return F.pad(x.double(), (padl, 15 - padl)).unfold(2, 16, 1).permute(0, 2, 1, 3).reshape(B * T, NCH * 16)


def conv64_prep_ref(w):
    """eav_conv64_prep_weights: wT_fwd[i * 16 + k][o] = W[o][i][k]; wT_bwd[o * 16 + k'][i] = W[o][i][15 - k']."""
    return (w.permute(1, 2, 0).reshape(1024, NCH).contiguous(), w.flip(2).permute(0, 2, 1).reshape(1024, NCH).contiguous())


def conv64_visits(B, T):
    tile = conv64_tile(B, T)
    return cdiv(B * cdiv(T, tile), conv64_fwd_grid(B, T)) * (tile // 32)


def _conv64_apply(xu, wm, B, T, visits):
    """out = xu . wm as [B,64,T] with its bound: four chunk chains of 256 fma terms, summed (a + b) + (c + d): 258 roundings on
    an element's path.  Statistics: one accumulation per 32-sample sub-tile a thread visits, then half_sum (5): visits + 5
    additions (+ 1 for the square); the partial rows are added in float64 by the test."""
    out = (xu @ wm.double()).view(B, T, NCH).permute(0, 2, 1).contiguous()
    mag = (xu.abs() @ wm.double().abs()).view(B, T, NCH).permute(0, 2, 1).contiguous()
    ob = rb(258, mag)
    d = (0, 2)
    return {"out": out, "bound": ob, "s": out.sum(d), "q": (out * out).sum(d),
            "s_bound": ob.sum(d) + rb(visits + 5, out.abs().sum(d)),
            "q_bound": (2 * out.abs() * ob).sum(d) + rb(visits + 6, (out * out).sum(d)),
            "exact": [(float(mag.max()), 1.0, "out"), (float(out.abs().sum(d).max()), 1.0, "sum"),
                      (float((out * out).sum(d).max()), 1.0, "sum of squares")]}


def conv64_fwd_ref(x, w, visits=1):
    """nn.Conv2d(64, 64, (1, 16), padding='same', bias=False): out[b,o,t] = sum_{i,k} W[o,i,k] x[b,i,t+k-7]."""
    B, _, T = x.shape
    return _conv64_apply(conv64_unfold(x, 7), w.double().reshape(NCH, 1024).t(), B, T, visits)


def conv64_dgrad_ref(du, w):
    """Its input gradient: dx[b,i,u] = sum_{o,k} W[o,i,k] du[b,o,u-k+7] = sum_{o,k'} W[o,i,15-k'] du[b,o,u+k'-8]."""
    B, _, T = du.shape
    return _conv64_apply(conv64_unfold(du, 8), w.double().flip(2).permute(0, 2, 1).reshape(1024, NCH), B, T, 1)


def conv64_wgrad_ref(du, x):
    """Its weight gradient, summed over the partial rows: dW[o,i,k] = sum_{b,t} du[b,o,t] x[b,i,t+k-7].  A block's chain
    runs over its cdiv(items, grid) work items of 128 positions each (zero padding included)."""
    B, _, T = x.shape
    xu = conv64_unfold(x, 7)
    d2 = du.double().permute(1, 0, 2).reshape(NCH, B * T)
    mag = (d2.abs() @ xu.abs()).view(NCH, NCH, 16)
    n = cdiv(B * cdiv(T, 128), conv64_wgrad_grid(B, T)) * 128
    return {"dW": (d2 @ xu).view(NCH, NCH, 16), "bound": rb(n, mag), "exact": [(float(mag.max()), 1.0, "dW")]}


# -------------------------------------------------------------------------------- firstBN -> ELU -> depthwiseConv
def dw_inputs(mode, B, C, S):
    """(y1 [B,8,C,S], bn1 [6,8], w2 [64,C], bn2 [6,64], dz [B,64,S]); exact: |y1| <= 2, scale <= 2 -> shift 4; |z| <= 8 C,
    scale2 <= 2 -> shift 16 C."""
    seed = seed_of("dw", mode, B, C, S)
    if mode == "exact":
        return (ints(seed, (B, F1, C, S), -2, 2), bn_block(mode, seed + 1, F1, 4.0), ints(seed + 2, (NCH, C), -1, 1),
                bn_block(mode, seed + 3, NCH, 16.0 * C), ints(seed + 4, (B, NCH, S), -2, 2))
    return (normal(seed, (B, F1, C, S)), bn_block(mode, seed + 1, F1), uniform(seed + 2, (NCH, C), -0.3, 0.3),
            bn_block(mode, seed + 3, NCH), normal(seed + 4, (B, NCH, S)))


def _bn1_act(y1, bn1):
    """o = sc y1 + sh (2 roundings, or 1 contracted), a = elu_f(o), ELU'(o) = 1 or a + 1 (1 more rounding), xhat = (y1 - mean)
    invstd (2 roundings): values, and the bounds e_o = 2 u omag, e_a = e_o + 3 u |a|, e_slope = e_o + 3 u |a| + u slope,
    e_xhat = 2 u xmag."""
    mean, invstd, sc, sh = (_bc(bn1[i], 2) for i in range(4))
    y = y1.double()
    o = sc * y + sh
    omag = sc.abs() * y.abs() + sh.abs()
    a, slope = elu64(o), slope64(o)
    eo = 2 * U * omag
    xmag = (y.abs() + mean.abs()) * invstd.abs()
    return {"o": o, "a": a, "slope": slope, "e_a": eo + ELU_ULP * a.abs(), "e_slope": eo + ELU_ULP * a.abs() + U * slope,
            "xhat": (y - mean) * invstd, "xmag": xmag, "e_xhat": 2 * U * xmag}


def dw_fwd_ref(y1, bn1, w2, bn2=None):
    """eav_eegnet_dw_fwd(_pool_eval): z[b,f*8+d,t] = sum_c w2[f*8+d,c] ELU(scale1[f] y1[b,f,c,t] + shift1[f]); the rows of
    the statistics buffer are the sums of z and z^2 over one (sample, 1024-sample chunk); p2 = AvgPool4(ELU(bn2(z))).
    z: CG channel groups each run a chain of ceil(C / CG) multiply-adds (2 roundings a term), then CG - 1 additions.
    Statistics: 4 samples per thread (3 additions), wave sum (6), up to 8 waves in wave order (7): 16, + 1 for the square.
    p2: o2 = sc2 z + sh2 (2 roundings), elu_f, a chain of 4 (3 additions), x 0.25 exact."""
    B, _, C, S = y1.shape
    act = _bn1_act(y1, bn1)
    w = w2.double().view(F1, DD, C)
    z = torch.einsum("fdc,bfct->bfdt", w, act["a"]).reshape(B, NCH, S)
    zmag = torch.einsum("fdc,bfct->bfdt", w.abs(), act["a"].abs()).reshape(B, NCH, S)
    cg = dw_plan(S) // 1000
    ez = torch.einsum("fdc,bfct->bfdt", w.abs(), act["e_a"]).reshape(B, NCH, S) + rb(2 * cdiv(C, cg) + cg - 1, zmag)
    rows = lambda v: chunk_sum(v).permute(0, 2, 1)  # noqa: E731    [B, nchunk, 64]
    r = {"z": z, "z_bound": ez, "s": rows(z), "q": rows(z * z), "s_bound": rows(ez) + rb(16, rows(z.abs())),
         "q_bound": rows(2 * z.abs() * ez) + rb(17, rows(z * z)), "min_pre": float(act["o"].min()),
         "exact": [(float(zmag.max()), 0.5, "z"), (float(rows(z.abs()).max()), 0.5, "sum z"),
                   (float(rows(z * z).max()), 0.25, "sum z^2")]}
    if bn2 is not None:
        s2, h2 = _bc(bn2[2], 1), _bc(bn2[3], 1)
        o2 = s2 * z + h2
        a2 = elu64(o2)
        ea2 = s2.abs() * ez + 2 * U * (s2.abs() * z.abs() + h2.abs()) + ELU_ULP * a2.abs()
        pool = lambda v: v.view(B, NCH, S // 4, 4).sum(-1)  # noqa: E731
        r.update(p=0.25 * pool(a2), p_bound=0.25 * (pool(ea2) + 3 * U * pool(a2.abs())),
                 min_pre=min(r["min_pre"], float(o2.min())))
        r["exact"].append((float(pool(o2.abs()).max()), 0.5, "pool"))
    return r


def pool_mult(mask, drop_p, shape):
    """Dropout multiplier of every pooled output: 1 / (1 - |p|) where the keep mask is set, 0 elsewhere; all ones for p = 0."""
    if drop_p == 0.0:
        return torch.ones(shape, dtype=torch.float64)
    return mask.double() / (1.0 - abs(drop_p))


def pool_bwd_ref(dp, u, bn, P, mult, train=True, nround=3):
    """Backward of BN -> ELU -> AvgPool(1,P) -> Dropout at the BatchNorm input u [B,CH,T] (eav_bn_elu_pool_bwd_*; the prologue
    of eav_eegnet_dw_bwd_fused with P = 4):  go = dp[t/P] / P * mult (exact: powers of two; 0 on the tail past the last whole
    window), g = go ELU'(o) with o = scale u + shift, uhat = (u - mean) invstd, du = scale (g - m1 - uhat m2) (train) or scale g.
      e_g  = |go| e_slope + u |g|          (e_slope = e_o + 3 u |a| + u slope, e_o = 2 u (|scale||u| + |shift|))
      e_du = |scale| (|go| e_slope + |m2| e_uhat) + nround u |scale| (|g| + |m1| + |m2||uhat|)
    nround = 3 for pool_bwd_du (two fmas and the product with scale), 7 for the fused kernel's plain expression."""
    B, CH, T = u.shape
    mean, invstd, sc, sh, m1, m2 = (_bc(bn[i], 1) for i in range(6))
    if not train:
        m1, m2 = torch.zeros_like(m1), torch.zeros_like(m2)
    To = T // P
    go = F.pad((dp.double() * mult / P).repeat_interleave(P, dim=2), (0, T - To * P))
    ud = u.double()
    o = sc * ud + sh
    a, slope = elu64(o), slope64(o)
    es = 2 * U * (sc.abs() * ud.abs() + sh.abs()) + ELU_ULP * a.abs() + U * slope
    g = go * slope
    eg = go.abs() * es + U * g.abs()
    uhat = (ud - mean) * invstd
    umag = (ud.abs() + mean.abs()) * invstd.abs()
    dumag = sc.abs() * (g.abs() + m1.abs() + m2.abs() * umag)
    return {"g": g, "e_g": eg, "uhat": uhat, "umag": umag, "e_uhat": 2 * U * umag, "du": sc * (g - m1 - uhat * m2),
            "e_du": sc.abs() * (go.abs() * es + m2.abs() * 2 * U * umag) + nround * U * dumag, "du_mag": dumag,
            "min_pre": float(o.min())}


def pool_sums(r, n):
    """part [B][2 CH] of the pool backward: sum_t g and sum_t g uhat per (sample, channel) row, a chain of n additions."""
    g, uh = r["g"], r["uhat"]
    gu_err = r["e_g"] * r["umag"] + g.abs() * r["e_uhat"] + U * (g * uh).abs()
    gmag, gumag = g.abs().sum(-1), (g.abs() * r["umag"]).sum(-1)
    return {"s": g.sum(-1), "q": (g * uh).sum(-1), "s_bound": r["e_g"].sum(-1) + rb(n, gmag),
            "q_bound": gu_err.sum(-1) + rb(n, gumag), "s_mag": gmag, "q_mag": gumag}


def dw_bwd_ref(y1, dz, e_dz, bn1, w2):
    """eav_eegnet_dw_bwd (and the body of the fused forms, with dz and its error bound e_dz from pool_bwd_ref):
      da[b,f,c,t] = sum_d w2[f*8+d,c] dz[b,f*8+d,t]  (8 multiply-adds: 16 roundings),  g1 = da ELU'(o)  (1 rounding)
      stat rows [B, nchunk, 16]: sum g1 and sum g1 xhat over (c, t) of a 1024-sample chunk: a thread's chain of 4 samples x
          ceil(C / CG) channels, wave sum (6), waves in order (<= 7): 4 ceil(C / CG) + 13 additions, + 1 for the product
      dW2 rows [B, nchunk, 64 C]: sum_t dz a: 4 products and 3 additions per thread (<= 5 roundings on a path), the
          butterfly over the wave (6), the wave slots (<= 3): 14."""
    B, _, C, S = y1.shape
    act = _bn1_act(y1, bn1)
    w = w2.double().view(F1, DD, C)
    dzv = dz.double().view(B, F1, DD, S)
    da = torch.einsum("fdc,bfdt->bfct", w, dzv)
    damag = torch.einsum("fdc,bfdt->bfct", w.abs(), dzv.abs())
    eda = rb(16, damag)
    if e_dz is not None:
        eda = eda + torch.einsum("fdc,bfdt->bfct", w.abs(), e_dz.view(B, F1, DD, S))
    g = da * act["slope"]
    eg = eda * act["slope"] + damag * act["e_slope"] + U * g.abs()
    gx = g * act["xhat"]
    egx = eg * act["xmag"] + g.abs() * act["e_xhat"] + U * gx.abs()
    cg = dw_plan(S) // 1000 if e_dz is not None else 1
    n = 4 * cdiv(C, cg) + 13
    rows = lambda v: chunk_sum(v.sum(2)).permute(0, 2, 1)  # noqa: E731     [B,8,C,S] -> [B, nchunk, 8]
    gmag, gxmag = damag * act["slope"], damag * act["slope"] * act["xmag"]
    st = torch.cat([rows(g), rows(gx)], 2)
    st_bound = torch.cat([rows(eg) + rb(n, rows(gmag)), rows(egx) + rb(n + 1, rows(gxmag))], 2)
    nchunk = cdiv(S, 1024)
    padS = nchunk * 1024 - S
    dzc = F.pad(dzv, (0, padS)).view(B, F1, DD, nchunk, 1024)
    ac = lambda v: F.pad(v, (0, padS)).view(B, F1, C, nchunk, 1024)  # noqa: E731
    dw = torch.einsum("bfdnt,bfcnt->bnfdc", dzc, ac(act["a"])).reshape(B, nchunk, NCH * C)
    dwmag = torch.einsum("bfdnt,bfcnt->bnfdc", dzc.abs(), ac(act["a"].abs())).reshape(B, nchunk, NCH * C)
    edw = torch.einsum("bfdnt,bfcnt->bnfdc", dzc.abs(), ac(act["e_a"])).reshape(B, nchunk, NCH * C) + rb(14, dwmag)
    if e_dz is not None:
        edzc = F.pad(e_dz.view(B, F1, DD, S), (0, padS)).view(B, F1, DD, nchunk, 1024)
        edw = edw + torch.einsum("bfdnt,bfcnt->bnfdc", edzc, ac(act["a"].abs())).reshape(B, nchunk, NCH * C)
    return {"g1": g, "g1_bound": eg, "st": st, "st_bound": st_bound, "dW": dw, "dW_bound": edw,
            "min_pre": float(act["o"].min()),
            "exact": [(float(damag.max()), 0.25, "g1"), (float(rows(g.abs()).max()), 0.25, "sum g1"),
                      (float(rows(gx.abs()).max()), 0.125, "sum g1 xhat"), (float(dwmag.max()), 0.25, "dW2")]}


def dw_fused_inputs(mode, B, C, S, drop_p):
    """(y1, z [B,64,S], dp2 [B,64,S/4], bn2, bn1, w2, mask or None); exact: |z| <= 2 and scale2 <= 2 -> shift 4; dp2 is a
    multiple of 4, so that dp2 / 4 * mult stays an integer.  A negative drop_p (row mode) gets a mask that is constant
    along every (sample, channel) row, as nn.Dropout2d draws it."""
    seed = seed_of("dwf", mode, B, C, S, drop_p)
    To = S // 4
    mask = None
    if drop_p > 0:
        mask = torch.from_numpy((synth.uniform(seed + 9, (B, NCH, To)) >= drop_p).astype(np.uint8))
    elif drop_p < 0:
        mask = torch.from_numpy((synth.uniform(seed + 9, (B, NCH, 1)) >= -drop_p).astype(np.uint8)).expand(B, NCH, To).contiguous()
    if mode == "exact":
        return (ints(seed, (B, F1, C, S), -2, 2), ints(seed + 1, (B, NCH, S), -2, 2), 4.0 * ints(seed + 2, (B, NCH, To), -1, 1),
                bn_block(mode, seed + 3, NCH, 4.0), bn_block(mode, seed + 4, F1, 4.0), ints(seed + 5, (NCH, C), -1, 1), mask)
    return (normal(seed, (B, F1, C, S)), normal(seed + 1, (B, NCH, S)), normal(seed + 2, (B, NCH, To)),
            bn_block(mode, seed + 3, NCH), bn_block(mode, seed + 4, F1), uniform(seed + 5, (NCH, C), -0.3, 0.3), mask)


def dw_bwd_fused_ref(y1, z, dp2, bn2, bn1, w2, mult, train):
    """eav_eegnet_dw_bwd_fused (train) / _fused_eval (depthwiseBN on its running statistics: m1 = m2 = 0 whatever the slots
    hold, and the rows of bn2_part [B, nchunk, 128] = sum g2, sum g2 zhat per channel over a chunk: 4 samples (3 additions),
    wave total (6), <= 4 waves (3), + 1 for the product: 13)."""
    pr = pool_bwd_ref(dp2, z, bn2, 4, mult, train, nround=7)
    r = dw_bwd_ref(y1, pr["du"], pr["e_du"], bn1, w2)
    r["min_pre"] = min(r["min_pre"], pr["min_pre"])
    r["exact"].append((float(pr["du_mag"].max()), 0.5, "dz"))
    if not train:
        g, uh = pr["g"], pr["uhat"]
        egu = pr["e_g"] * pr["umag"] + g.abs() * pr["e_uhat"] + U * (g * uh).abs()
        rows = lambda v: chunk_sum(v).permute(0, 2, 1)  # noqa: E731
        gmag, gumag = rows(g.abs()), rows(g.abs() * pr["umag"])
        r["p2"] = torch.cat([rows(g), rows(g * uh)], 2)
        r["p2_bound"] = torch.cat([rows(pr["e_g"]) + rb(12, gmag), rows(egu) + rb(13, gumag)], 2)
        r["exact"] += [(float(gmag.max()), 0.5, "sum g2"), (float(gumag.max()), 0.25, "sum g2 zhat")]
    return r


# ----------------------------------------------------------------------------- BN -> ELU -> AvgPool(1,P) -> Dropout
def pool_inputs(mode, B, T, P, drop_p):
    """(u [B,64,T], bn [6,64], dp [B,64,T/P], mask or None); exact: dp is a multiple of P."""
    seed = seed_of("pool", mode, B, T, P, drop_p)
    To = T // P
    mask = None
    if drop_p > 0:
        mask = torch.from_numpy((synth.uniform(seed + 9, (B, NCH, To)) >= drop_p).astype(np.uint8))
    elif drop_p < 0:
        mask = torch.from_numpy((synth.uniform(seed + 9, (B, NCH, 1)) >= -drop_p).astype(np.uint8)).expand(B, NCH, To).contiguous()
    if mode == "exact":
        return ints(seed, (B, NCH, T), -2, 2), bn_block(mode, seed + 1, NCH, 4.0), float(P) * ints(seed + 2, (B, NCH, To), -1, 1), mask
    return normal(seed, (B, NCH, T)), bn_block(mode, seed + 1, NCH), normal(seed + 2, (B, NCH, To)), mask


def pool_fwd_ref(u, bn, P, mult):
    """eav_bn_elu_pool_fwd: out[b,ch,to] = mult / P * sum_{j<P} ELU(scale u[b,ch,to P + j] + shift): o 2 roundings, elu_f, a
    chain of P (P - 1 additions); the two scalings are by powers of two."""
    B, CH, T = u.shape
    To = T // P
    sc, sh = _bc(bn[2], 1), _bc(bn[3], 1)
    ud = u.double()[:, :, :To * P]
    o = sc * ud + sh
    a = elu64(o)
    ea = 2 * U * (sc.abs() * ud.abs() + sh.abs()) + ELU_ULP * a.abs()
    win = lambda v: v.reshape(B, CH, To, P).sum(-1)  # noqa: E731
    return {"out": win(a) * mult / P, "bound": (win(ea) + (P - 1) * U * win(a.abs())) * mult / P, "min_pre": float(o.min()),
            "exact": [(float((win(o.abs()) * mult).max()), 1.0 / P, "pool out")]}


def pool_chain(T, P, one_pass):
    """Additions on the path of one element of the pool backward sums: reduce walks ceil(T/P / 256) windows of P samples
    per thread, the one-pass form ceil(ceil(T/4) / 256) quads of 4; then the wave sum (6) and the four waves (<= 3)."""
    return (4 * cdiv(cdiv(T, 4), 256) if one_pass else P * cdiv(T // P, 256)) + 9


# --------------------------------------------------------------------------------------------------- case lists
# firstConv forward (B, C, S, K): every instantiation edge of kernLength at the smallest shape with two work rows per block
# dimension; row lengths around one tile, the scalar store path (333), one full segment and a second segment of ONE tile
# (2052); 527 work items for the 512 blocks of the grid at the 152- and the 66-step instantiation.
FIR_FWD_CASES = ([(2, 3, 130, K) for K in (1, 7, 64, 65, 66, 128, 129, 130, 299, 300)]
                 + [(2, 3, S, 300) for S in (1, 127, 128, 129, 333, 2048, 2052)]
                 + [(17, 31, 130, 300), (17, 31, 130, 100)])
# firstConv weight gradient: the WG_NT edges of kernLength; S around the S + 1 rule of wgrad_geometry (248 k positions
# need k + 1 chunks); 13 * 32 * 9 = 3744 work items for the 3072 waves of the grid at every WG_NT.
FIR_WGRAD_CASES = ([(2, 3, 333, K) for K in (1, 64, 65, 128, 129, 300)]
                   + [(2, 3, S, 300) for S in (3, 247, 248, 249, 496, 1984)]
                   + [(13, 32, 1984, 300), (13, 32, 1984, 100), (13, 32, 1984, 9)])
# block-1 inference: the NSTEP edges, C = 1 / 32 (CHMAX), S around one and four tiles, 260 work items on 256 blocks
INFER_CASES = ([(2, 3, 132, K) for K in (9, 65, 66, 129, 130, 300)] + [(2, C, 132, 9) for C in (1, 32)]
               + [(2, 3, S, 66) for S in (4, 128, 512, 516)] + [(130, 2, 516, 300)])
# depthwise passes (B, C, S): S on both sides of the 256 / 512 geometry thresholds and of the 1024-sample chunk, S % 4 != 0
# (333, 1023), a chunk of four samples (1028), three chunks (2052); C = 1, 30 and CHMAX = 32 at one S of every geometry
DW_CASES = ([(3, 3, S) for S in (4, 252, 256, 260, 333, 512, 516, 1023, 1024, 1028, 2052)]
            + [(1, C, S) for C in (1, 30, 32) for S in (256, 512, 1028)])
DROP_MODES = [0.0, 0.5, -0.5]
# dropout of the fused backward per case: every mode at one S of every geometry, alternating elsewhere
DW_FUSED_CASES = [(B, C, S, DROP_MODES[i % 3]) for i, (B, C, S) in enumerate(DW_CASES) if S >= 4] + \
                 [(3, 3, S, d) for S in (256, 516, 1023) for d in DROP_MODES]
# pool passes (B, T, P, drop): one window, a tail quad beyond the last whole window for P = 8 (12: one window + one quad),
# T % 4 != 0 (333, 335), T / P just above 256 for P = 4 (1028) and P = 8 (2056), a tail past the second trip (2060)
POOL_CASES = [(B, T, P, DROP_MODES[(i + j) % 3]) for j, P in enumerate((4, 8))
              for i, (B, T) in enumerate([(3, P), (1, 12), (3, 333), (1, 335), (3, 1028), (1, 2056), (3, 2060)])] + \
             [(3, 2060, P, d) for P in (4, 8) for d in (0.5, -0.5)]
# separableConv (B, T): the 32-sample tile (fewer than 128 items of 128 samples) at T % 4 != 0 and T % 32 != 0; the
# 128-sample tile at one item per sample and at 258 items for the 256 / 192 blocks of the two grids
CONV64_CASES = [(2, 125), (1, 33), (3, 300), (2, 131), (128, 33), (129, 130)]
