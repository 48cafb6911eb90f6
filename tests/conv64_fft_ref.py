"""References for the frequency-domain separableConv kernels (csrc/eegnet_conv64_fft.hip): the launch geometry restated,
float64 references, a float32 restatement of the algorithm, an a-priori rounding bound, and the case lists of
tests/test_conv64_fft_ref_cpu.py (no GPU) and tests/test_conv64_fft_kernels_gpu.py.

The geometry
------------
LV = 49 valid outputs per 64-sample block, nblk = ceil(T / 49) blocks per sample, two of them per column (block 2 p real,
block 2 p + 1 imaginary): npair = ceil(nblk / 2), ncol = B npair, ncolp = ncol rounded up to 128.  The pack kernels run
min(512, ncolp / 4) workgroups of 4 waves, a wave per column (a second column from column 2048 on); the per-bin GEMM walks
ncolp / 32 tiles on min(8, ncolp / 32) workgroups per bin, starting at tile (workgroup + bin) mod workgroups; the weight
gradient contracts 4 chunks of nkb = ncolp / 128 K-blocks of 32 columns through a ring of 4 stages.  `ws_floats` and
`nparts` restate the two sizing exports; ncolp is recoverable from ws_floats (`ncolp_of_ws`), which is how every GPU case
asserts the shape class it is listed for.

The references
--------------
out[b,o,t] = sum_{i,k} W[o,i,k] x[b,i,t+k-7] ('same' padding of a 16-tap filter: 7 left, 8 right);
dx[b,i,t] = sum_{o,k'} W[o,i,15-k'] du[b,o,t+k'-8] (flipped and transposed taps, padding 8 / 7);
dW[o,i,k] = sum_{b,t} du[b,o,t] x[b,i,t+k-7].  They are evaluated by float64 numpy.fft with one transform per row (error
~1e-16 of the operand norms) and pinned to F.conv1d in float64 and its autograd, and to conv64_*_ref of
tests/eegnet_direct_ref.py, by the CPU test.  The fused form's du is pool_bwd_ref of tests/eegnet_direct_ref.py (P = 8).

The yardstick
-------------
`fwd_c32` / `wgrad_c32` run the kernel's ALGORITHM on the CPU in float32 / complex64: 64-sample overlap-save blocks that
start padl before each 49-sample block, two blocks of a sample as the real and imaginary part of one column, scipy.fft in
complex64 (asserted), G = conj(FFT(w)) / 64 rounded to float32, per bin the real [cols x 128] . [128 x 128] product in
float32, the inverse transform without 1 / N; for the weight gradient the zero-padded 49-sample du blocks, per bin
P = D^T Z over the columns in four chunks summed in order, Acc = (Prr + Pii, Pri - Pir), the inverse transform, taps
0 .. 15, times 1 / 64.  Its error against float64 is what fp32 arithmetic costs this design; the kernels are held to twice
its RMS (another correct ordering of the same depth), not to a guessed tolerance.  `fft=` replaces the forward transform
of the inputs (`fft64_8x8`: the kernel's own 8 x 8 factorisation with an explicit twiddle table), `G_hook` / `leak` perturb
the filter spectra and the columns: the CPU test uses them to show what the criteria notice and rtol 1e-4 does not.

The bound (u = 2^-24)
---------------------
One 64-point transform of the kernel is 8 x 8: two dft8, each a radix-2 x radix-4 butterfly = three levels of additions,
six in all, and at most three twiddle products per element (W8 inside each dft8, W64^(n2 k1) between them).  Every computed
sum is (a + b)(1 + d), |d| <= u, and every level is sqrt(2) times a unitary map: a level adds u to the relative 2-norm
error.  A twiddle product fl(a w') is a w' (1 + d), |d| <= sqrt(5) u (Brent, Percival, Zimmermann 2007), and the tabulated
w' is w to within one ulp per component, |w' - w| <= sqrt(2) u.  To first order
    ||T'(v) - T(v)||_2 <= eT ||T(v)||_2 = 8 eT ||v||_2,     eT = (6 + 3 (sqrt(5) + sqrt(2))) u = 16.95 u
(Higham, Accuracy and Stability of Numerical Algorithms, section 24.1, with the stage count of this factorisation; the
module adds 1 % for the second-order terms).

Forward and data gradient, output channel o of column c: y = F^H (sum_i Z_i . G_oi), Z_i = F s_i the spectrum of the
complex column of input channel i (BOTH blocks), G_oi = conj(F w_oi) / 64.  An error e in the frequency domain reaches
every output as at most ||e||_1, ||a . b||_1 <= ||a||_2 ||b||_2, ||Z_i||_2 = 8 ||s_i||_2, ||G_oi||_2 = ||w_oi||_2 / 8:
    the transform of s_i         eT ||s_i|| ||w_oi||
    the transform of w_oi        eT ||s_i|| ||w_oi||           (the scaling by 1 / 64 is exact)
    the per-bin product          128 sqrt(2) u ||s_i|| ||w_oi||   (a k-ordered chain of 128 fused multiply-adds per real
                                 output: 128 u sum_k |terms|, |Gr||zr| + |Gi||zi| <= |G||Z| per channel, real and
                                 imaginary part together sqrt(2))
    the inverse transform        eT ||F^H (Z_i . G_oi)||_2 <= eT 8 ||Z_i||_2 ||G_oi||_inf <= eT ||s_i||_2 ||w_oi||_1
                                 <= eT sqrt(16) ||s_i|| ||w_oi||
    |err| <= g u sum_i ||s_{c,i}||_2 ||w_{o,i}||_2,     g = 1.01 ((1 + 1 + sqrt(16)) eT / u + 128 sqrt(2)) = 285.6
A worst-case bound without any assumption on how errors combine.  It says what the design cannot do better than: the error
of an output scales with the norm of the whole column - a quiet block beside a loud one, or a quiet stretch of a loud
block, keeps the loud one's absolute error - where the direct kernel's scales with the 16 samples under the filter.

Weight gradient: dW_oi = Re F^H (sum_c conj(D_co) . Z_ci) / 64, D_co the spectrum of the zero-padded du blocks d_co:
    the transforms of s, d       2 eT ||s_ci|| ||d_co||
    the products                 sqrt(5) u ||s_ci|| ||d_co||    (the bound of an unfused complex product; the MFMA fuses)
    the accumulation             sqrt(2) (ncolp / 4 + 5) u sum_c ||s_ci|| ||d_co||: ncolp / 4 columns per chunk in one chain,
                                 4 additions of the chunks, 1 for Prr + Pii / Pri - Pir
    the inverse transform        eT 8 sum_c ||s_ci|| ||d_co||   (||Z . D||_2 <= ||Z||_2 ||d||_1 <= 8 ||s|| 8 ||d||, / 64,
                                 and the transform's own factor 8)
    |err| <= gw u sum_c ||d_{c,o}||_2 ||s_{c,i}||_2,     gw = 1.01 ((2 + 8) eT / u + sqrt(5) + sqrt(2) (ncolp / 4 + 5))
The fused form (du formed while loading) adds the fp32 formation of du: sum_c ||dd_co|| ||s_ci|| for dW and
sum_{o,k} |W[o,i,k]| dd[b,o,.] for dx, dd = e_du of pool_bwd_ref (three roundings).

Statistics: stat_part is compared with the float64 sums of the kernel's OWN fp32 output over exactly t < T - only the
order of fp32 additions lies between them: a wave adds its columns' values one by one, n = columns per wave x 98
additions per channel: 1.01 n u sum |v|, and n + 1 for the squares (the rows are added in float64 by the test).

The CPU test asserts that the float32 restatement stays within 0.1 of every bound and prints its worst ratio."""
import functools
import zlib

import numpy as np
import scipy.fft as sf
import torch

from eav_amd import synth
from tests import eegnet_direct_ref as DR

LV, NB, KT, NCH = 49, 64, 16, 64
PADF, PADB = 7, 8
U = 2.0 ** -24
ET = 6 + 3 * (5 ** 0.5 + 2 ** 0.5)            # relative 2-norm error of one 64-point transform, in units of u
G_FWD = 1.01 * ((1 + 1 + KT ** 0.5) * ET + 128 * 2 ** 0.5)
TABLE = 64 * 128 * 128                         # floats of one filter-spectrum table
RMS_MARGIN = 2.0


def cdiv(a, b):
    return -(-a // b)


# --------------------------------------------------------------------------------------------------------- the geometry
def geometry(B, T):
    nblk = cdiv(T, LV)
    npair = cdiv(nblk, 2)
    ncol = B * npair
    ncolp = cdiv(ncol, 128) * 128
    pack = max(1, min(512, ncolp // 4))
    return dict(nblk=nblk, npair=npair, ncol=ncol, ncolp=ncolp, pack_wgs=pack, waves=4 * pack,
                cols_per_wave=cdiv(ncolp, 4 * pack), tiles=ncolp // 32, gemm_wgs=min(8, ncolp // 32), nkb=ncolp // 128)


def ws_floats(B, T):
    """two filter tables, three spectra buffers [64][ncolp][128], four split-K partial products, their sum"""
    return 2 * TABLE + 3 * 64 * geometry(B, T)["ncolp"] * 128 + 4 * TABLE + 64 * 64 * 64 * 2


def ws_offsets(B, T):
    """float offsets of BmF, BmB, Zf, Zb, Y, Pp, Acc and the end"""
    sp = 64 * geometry(B, T)["ncolp"] * 128
    sizes = [TABLE, TABLE, sp, sp, sp, 4 * TABLE, 64 * 64 * 64 * 2]
    return dict(zip(("BmF", "BmB", "Zf", "Zb", "Y", "Pp", "Acc", "end"), np.concatenate([[0], np.cumsum(sizes)]).tolist()))


def nparts(B, T):
    return geometry(B, T)["waves"]


def ncolp_of_ws(floats):
    n, r = divmod(floats - 6 * TABLE - 64 * 64 * 64 * 2, 3 * 64 * 128)
    assert r == 0 and n > 0 and n % 128 == 0, floats
    return n


def stat_chain(B, T):
    """additions per channel of one wave: its columns (the stride of the walk is the wave count) x 98 samples"""
    g = geometry(B, T)
    return cdiv(g["ncol"], g["waves"]) * 2 * LV


# -------------------------------------------------------------------------------------------------- float64 references
def flip_w(w):
    """filters of the data gradient: w'[i][o][k'] = w[o][i][15 - k']"""
    return np.ascontiguousarray(np.asarray(w)[:, :, ::-1].transpose(1, 0, 2))


def corr_ref(x, wf, padl):
    """float64 [B,64,T]: out[b,o,t] = sum_{i,k} wf[o,i,k] x[b,i,t+k-padl], x zero outside"""
    x, wf = np.asarray(x, np.float64), np.asarray(wf, np.float64)
    T = x.shape[-1]
    L = sf.next_fast_len(T + KT - 1, real=True)
    X = np.fft.rfft(np.pad(x, ((0, 0), (0, 0), (padl, KT - 1 - padl))), L)
    W = np.fft.rfft(wf, L)
    return np.fft.irfft(np.einsum("oif,bif->bof", np.conj(W), X), L)[..., :T]


def fwd_ref(x, w):
    return corr_ref(x, w, PADF)


def dgrad_ref(du, w):
    return corr_ref(du, flip_w(w), PADB)


def wgrad_ref(du, x):
    """float64 [64,64,16]"""
    x, du = np.asarray(x, np.float64), np.asarray(du, np.float64)
    T = x.shape[-1]
    L = sf.next_fast_len(T + KT - 1, real=True)
    X = np.fft.rfft(np.pad(x, ((0, 0), (0, 0), (PADF, KT - 1 - PADF))), L)
    D = np.fft.rfft(du, L)
    return np.fft.irfft(np.einsum("bof,bif->oif", np.conj(D), X), L)[..., :KT]


def stat_ref(out):
    """[128] float64: sums and sums of squares per channel"""
    o = np.asarray(out, np.float64)
    return np.concatenate([o.sum((0, 2)), (o * o).sum((0, 2))])


def du_ref(dp, u, bn, mask, drop_p):
    """pool_bwd_ref of the direct module at P = 8 (torch in, its dictionary out: 'du', 'e_du')"""
    B, _, T = u.shape
    mult = DR.pool_mult(mask, drop_p, (B, NCH, T // 8))
    return DR.pool_bwd_ref(dp, u, bn, 8, mult, True, nround=3)


# ------------------------------------------------------------------------------------- the algorithm in float32
def columns(x, padl, valid_only=False, dtype=np.complex64):
    """[B,64,T] -> [ncol, 64 channels, 64 samples] complex: block 2 p + i block 2 p + 1; the 64 samples from padl before the
    block, or (valid_only) the block's 49 samples zero-padded"""
    B, _, T = x.shape
    g = geometry(B, T)
    left = 0 if valid_only else padl
    real = np.float64 if dtype == np.complex128 else np.float32
    xp = np.zeros((B, NCH, left + 2 * g["npair"] * LV + NB), real)
    xp[:, :, left:left + T] = x
    col = np.zeros((B, g["npair"], NCH, NB), dtype)
    width = LV if valid_only else NB
    for pr in range(g["npair"]):
        a, b = 2 * pr * LV, (2 * pr + 1) * LV
        col[:, pr, :, :width] = xp[:, :, a:a + width] + 1j * xp[:, :, b:b + width]
    return col.reshape(g["ncol"], NCH, NB)


def twiddles64():
    """[k1, n2] = W64^(n2 k1) in complex64: the table between the two dft8 of the kernel's transform"""
    k = np.arange(8)
    return np.exp(-2j * np.pi * np.outer(k, k) / 64).astype(np.complex64)


def fft64_8x8(a, tw=None):
    """the kernel's factorisation along the last axis (64): dft8 over n1 (n = 8 n1 + n2), twiddle, dft8 over n2; X[k1 + 8 k2]"""
    tw = twiddles64() if tw is None else tw
    v = a.reshape(a.shape[:-1] + (8, 8))                  # [n1, n2]
    v = sf.fft(v, axis=-2) * tw                           # [k1, n2]
    v = sf.fft(v, axis=-1)                                # [k1, k2]
    out = np.swapaxes(v, -1, -2).reshape(a.shape)         # index 8 k2 + k1
    assert out.dtype == np.complex64
    return out


def filter_spectra(wf):
    """G[o,i,m] = conj(FFT(w_oi)) / 64 in complex64"""
    wz = np.zeros((NCH, NCH, NB), np.complex64)
    wz[:, :, :KT] = wf
    G = np.conj(sf.fft(wz, axis=-1)) * np.float32(1.0 / NB)
    assert G.dtype == np.complex64
    return G


def real_rows(Z):
    """[cols, 64, bins] complex -> [bins, cols, 128] float32: (re | im) x channel, the layout of the spectra buffers"""
    return np.ascontiguousarray(np.concatenate([Z.real, Z.imag], 1).transpose(2, 0, 1))


def fwd_c32(x, wf, padl, fft=None, G_hook=None, leak=0.0, stages=False, full=False):
    """float32 [B,64,T] (full: [B,64,2 npair 49], the samples past T that the kernel computes and drops included)"""
    B, _, T = x.shape
    g = geometry(B, T)
    s = columns(np.asarray(x, np.float32), padl)
    if leak:                                               # block B picks up a share of block A
        s = (s.real + 1j * (s.imag + np.float32(leak) * s.real)).astype(np.complex64)
    Z = (fft or (lambda a: sf.fft(a, axis=-1)))(s)
    assert Z.dtype == np.complex64
    G = filter_spectra(np.asarray(wf, np.float32))
    if G_hook is not None:
        G = G_hook(G)
    Gr, Gi = G.real.transpose(2, 1, 0), G.imag.transpose(2, 1, 0)          # [bin, i, o]
    Bm = np.ascontiguousarray(np.concatenate([np.concatenate([Gr, Gi], 2), np.concatenate([-Gi, Gr], 2)], 1))
    Y = np.matmul(real_rows(Z), Bm)                        # [bin, col, (re | im) x o]
    assert Y.dtype == np.float32
    Yc = (Y[:, :, :NCH] + 1j * Y[:, :, NCH:]).transpose(1, 2, 0)
    y = sf.ifft(np.ascontiguousarray(Yc), axis=-1, norm="forward")         # (norm='forward': no 1 / N here)
    assert y.dtype == np.complex64
    y = y.reshape(B, g["npair"], NCH, NB)[..., :LV]
    out = np.stack([y.real, y.imag], 2).reshape(B, 2 * g["npair"], NCH, LV).transpose(0, 2, 1, 3).reshape(B, NCH, -1)
    out = np.ascontiguousarray(out if full else out[..., :T])
    return (out, dict(Z=Z, G=G, Y=Yc)) if stages else out


def wgrad_c32(x, du, fft=None, leak=0.0):
    """float32 [64,64,16]"""
    B, _, T = x.shape
    g = geometry(B, T)
    tr = fft or (lambda a: sf.fft(a, axis=-1))
    s = columns(np.asarray(x, np.float32), PADF)
    if leak:
        s = (s.real + 1j * (s.imag + np.float32(leak) * s.real)).astype(np.complex64)
    Z, D = tr(s), tr(columns(np.asarray(du, np.float32), 0, True))
    assert Z.dtype == np.complex64 and D.dtype == np.complex64
    Zr, Dr = real_rows(Z), real_rows(D)                    # [bin, col, 128]
    cpc = g["ncolp"] // 4
    P = np.zeros((NB, 128, 128), np.float32)
    for c in range(4):                                     # the chunks in order; the zero padding columns add nothing
        a, b = c * cpc, min((c + 1) * cpc, g["ncol"])
        if b > a:
            P = P + np.matmul(Dr[:, a:b].transpose(0, 2, 1), Zr[:, a:b])
    assert P.dtype == np.float32
    acc = (P[:, :NCH, :NCH] + P[:, NCH:, NCH:]) + 1j * (P[:, :NCH, NCH:] - P[:, NCH:, :NCH])      # [bin, o, i]
    d = sf.ifft(np.ascontiguousarray(acc.astype(np.complex64).transpose(1, 2, 0)), axis=-1, norm="forward")
    out = d.real[..., :KT] * np.float32(1.0 / NB)
    assert out.dtype == np.float32
    return np.ascontiguousarray(out)


# ------------------------------------------------------------------------------------------------------------ the bound
def col_norms(x, padl, valid_only=False):
    """[ncol, 64]: 2-norm of the complex column of every channel, in float64"""
    return np.linalg.norm(columns(np.asarray(x, np.float64), padl, valid_only, np.complex128), axis=-1)


def fwd_bound(x, wf, padl):
    """float64 [B,64,T]: g u sum_i ||s_{c,i}|| ||w_{o,i}||, c the column of (b, t)"""
    B, _, T = x.shape
    g = geometry(B, T)
    wn = np.linalg.norm(np.asarray(wf, np.float64), axis=-1)                  # [o, i]
    per = (G_FWD * U) * (col_norms(x, padl) @ wn.T).reshape(B, g["npair"], NCH)
    pr = (np.arange(T) // LV) // 2
    return np.ascontiguousarray(per[:, pr, :].transpose(0, 2, 1))


def g_wgrad(ncolp):
    return 1.01 * ((2 + 8) * ET + 5 ** 0.5 + 2 ** 0.5 * (ncolp / 4 + 5))


def wgrad_bound(x, du, e_du=None):
    """float64 [64,64,1]; e_du: the element-wise bound of a du formed in fp32 (the fused form)"""
    B, _, T = x.shape
    sn = col_norms(x, PADF)
    b = (g_wgrad(geometry(B, T)["ncolp"]) * U) * (col_norms(du, 0, True).T @ sn)
    if e_du is not None:
        b = b + col_norms(e_du, 0, True).T @ sn
    return b[:, :, None]


def dgrad_bound(du, w, e_du=None):
    b = fwd_bound(du, flip_w(w), PADB)
    if e_du is not None:
        b = b + corr_ref(e_du, np.abs(flip_w(w)), PADB)
    return b


def stat_bound(out, B, T, extra=0):
    """[128]: 1.01 n u sum |v| and (n + 1) for the squares, of the kernel's own output"""
    o = np.asarray(out, np.float64)
    n = stat_chain(B, T)
    return 1.01 * U * np.concatenate([(n + extra) * np.abs(o).sum((0, 2)), (n + 1 + extra) * (o * o).sum((0, 2))])


def rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, np.float64)))))


def passes_old_tolerance(got, ref, atol=1e-5):
    """what stood in front of these kernels: rtol 1e-4, atol 1e-5, element-wise"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return bool((np.abs(got - ref) <= atol + 1e-4 * np.abs(ref)).all())


# ------------------------------------------------------------------------------------------------------------ the cases
# (B, T): T below one block and below / at the tap count (8: the smallest the fused form accepts); the last samples whose
# 8 / 7 halo crosses the block end, one full block, one block + 1 (block B holds one sample); a full pair, pair + 1 (the
# second column half empty), an odd block count
SMALL = [(2, 1), (2, 7), (2, 8), (3, 15), (3, 16), (2, 41), (2, 42), (2, 48), (3, 49), (2, 50), (2, 97), (3, 98), (2, 99),
         (2, 147)]
# the column-count classes, "normal" data only -> what geometry() must give (asserted from the exports by both tests)
COLUMNS = {
    (128, 50): dict(ncol=128, ncolp=128, tiles=4, gemm_wgs=4, nkb=1),       # no padding column
    (129, 50): dict(ncol=129, ncolp=256, tiles=8, gemm_wgs=8, nkb=2),       # 127 padding columns, the wait_dma<WDMA> prologue
    (257, 50): dict(ncol=257, ncolp=384, tiles=12, gemm_wgs=8, nkb=3),      # uneven wrap of 12 tiles on 8 workgroups
    (385, 50): dict(ncol=385, ncolp=512, tiles=16, gemm_wgs=8, nkb=4),      # first DMA issued inside the loop, ring not wrapped
    (513, 50): dict(ncol=513, ncolp=640, tiles=20, gemm_wgs=8, nkb=5),      # both LDS buffers reused, a ring stage refilled
    (2049, 8): dict(ncol=2049, ncolp=2176, pack_wgs=512, waves=2048, cols_per_wave=2),      # a wave's second column
}
ALL = SMALL + list(COLUMNS)
TONE_CASE = (2, 147)
TONE_BINS = [0, 1, 7, 8, 9, 31, 32]
IMPULSE_T = [0, 6, 7, 8, 40, 41, 42, 48, 49, 56, 57]
IMPULSE_TAPS = [0, 7, 8, 15]
RANGE_CASES = [(2, 50), (3, 98), (2, 147)]
RANGE_KINDS = ["blocks", "channels"]


def seed_of(*case):
    return zlib.crc32(repr(case).encode())


def weights(seed):
    return synth.uniform(seed, (NCH, NCH, KT), -0.05, 0.05)


@functools.lru_cache(maxsize=None)
def inputs(B, T, mode, arg=None):
    """(x, w, du) float32: 'normal', 'dc' (normal + 3), 'tone' (arg = bin), 'impulse', 'range' (arg = kind)"""
    seed = seed_of("conv64_fft", B, T)
    w = weights(seed + 1)
    if mode in ("normal", "dc", "range"):
        x, du = synth.normal(seed, (B, NCH, T)), synth.normal(seed + 2, (B, NCH, T))
        if mode == "dc":
            x, du = x + np.float32(3.0), du + np.float32(3.0)
        if mode == "range":
            lo, hi = np.float32(1e-3), np.float32(1e3)
            if arg == "blocks":                            # block A loud, block B quiet: they share one complex transform
                sc = np.where((np.arange(T) // LV) % 2 == 0, hi, lo)[None, None, :]
            else:                                          # odd channels loud, even ones quiet; filters within a parity
                sc = np.where(np.arange(NCH) % 2 == 1, hi, lo)[None, :, None]
                ch = np.arange(NCH)
                w = w * ((ch[:, None] + ch[None, :]) % 2 == 0)[:, :, None].astype(np.float32)
            x, du = x * sc, du * sc
        return x, w, du
    if mode == "tone":
        t = np.arange(T)[None, None, :]
        ch = np.arange(NCH)[None, :, None]
        b = np.arange(B)[:, None, None]
        x = ((1.0 + 0.1 * ch) * np.cos(2 * np.pi * arg * t / NB + 0.7 * ch + b)).astype(np.float32)
        du = ((2.0 - 0.02 * ch) * np.cos(2 * np.pi * arg * t / NB + 0.3 * ch + 2.0 * b + 0.5)).astype(np.float32)
        return x, w, du
    assert mode == "impulse"
    pos = sorted({t for t in IMPULSE_T + [T - 1] if 0 <= t < T})
    x, du = np.zeros((B, NCH, T), np.float32), np.zeros((B, NCH, T), np.float32)
    w = np.zeros((NCH, NCH, KT), np.float32)
    vals = [1.0, 2.0, -1.0, 4.0]
    for j, t in enumerate(pos):                            # distinct (sample, channel) rows, distinct (o, i) filters
        ci, co = (5 * j + 3) % NCH, (7 * j + 1) % NCH
        x[j % B, ci, t] = 1.0
        du[j % B, co, pos[(j + 1) % len(pos)]] = 1.0
        w[co, ci, IMPULSE_TAPS[j % 4]] = vals[(j // 4) % 4]
        w[(co + 32) % NCH, ci, IMPULSE_TAPS[(j + 1) % 4]] = vals[(j // 4 + 1) % 4]
    return x, w, du


@functools.lru_cache(maxsize=None)
def refs(B, T, mode, arg=None):
    """float64 (out, dx, dW) of inputs(...); impulse data: integers (every output is a shifted copy, a count, or exactly 0)"""
    x, w, du = inputs(B, T, mode, arg)
    r = fwd_ref(x, w), dgrad_ref(du, w), wgrad_ref(du, x)
    if mode == "impulse":
        assert max(np.abs(a - np.rint(a)).max() for a in r) < 1e-9
        r = tuple(np.rint(a) for a in r)
    return r


@functools.lru_cache(maxsize=None)
def bounds(B, T, mode, arg=None):
    x, w, du = inputs(B, T, mode, arg)
    return fwd_bound(x, w, PADF), dgrad_bound(du, w), wgrad_bound(x, du)


@functools.lru_cache(maxsize=None)
def yardsticks(B, T, mode, arg=None):
    x, w, du = inputs(B, T, mode, arg)
    return fwd_c32(x, w, PADF), fwd_c32(du, flip_w(w), PADB), wgrad_c32(x, du)


@functools.lru_cache(maxsize=None)
def fused_inputs(B, T):
    """(dp [B,64,T/8], u [B,64,T], bn [6,64], mask [B,64,T/8] uint8) as torch tensors: the pool backward's operands"""
    seed = seed_of("conv64_fft_fused", B, T)
    return (DR.normal(seed, (B, NCH, T // 8)), DR.normal(seed + 1, (B, NCH, T)), DR.bn_block("rounded", seed + 2, NCH),
            torch.from_numpy((synth.uniform(seed + 9, (B, NCH, T // 8)) >= 0.5).astype(np.uint8)))
