"""Float64 references of the fp32 GEMM (csrc/gemm_f32.hip) and of the encoder's row-wise / element-wise kernels
(csrc/tf_kernels.hip), written from the contracts in include/eav_hip.h in plain numpy on the CPU, one function per
operation; plus the input sets, the strided layouts, the guarded output allocator and the rounding bound that
test_fp32_encoder_kernels_gpu.py uses.  test_fp32_kernels_ref_cpu.py pins every reference to an independent statement of
it (torch.nn.functional / autograd in double) and checks the input sets without a device.

Data modes of every contraction.  "exact": small integers in [-4, 4] (alpha 0.5 or 1), so that every fp32 product and
partial sum is an exact integer (K <= 16 200: |sum| <= 16 * 16 200 < 2^24) and the kernel must equal the float64 result
bit for bit in any summation order.  "rounded": synth.normal operands, each element held to rounding_bound()."""
import math

import numpy as np
import torch

from eav_amd import synth
# SENT: the NaN payload of the guard bands, pad columns and never-written outputs; GUARD: floats of sentinel before an
# output (and at least as many after it)
from tests.kernel_check import GUARD, SENT, seed_of  # noqa: F401

U = 2.0 ** -24            # unit roundoff of fp32
BIG = 3.0e30              # fill of operand pads: finite, and ruinous to any sum it is read into

# Rounding bound of one output element that is a sum of n fp32 terms followed by the epilogue:
#     |fl(result) - result| <= (n + C_EPI) * 2^-24 * sum |terms|
# with sum |terms| formed in float64 from the absolute operands (|alpha| |A| |B| + |bias| + |resid| + |C_old|).
# The MFMA chain is an fma chain: one rounding per term, n in all, and every partial sum is bounded by sum |terms|, so
# to first order the chain contributes n * u * sum |terms| (Higham, Accuracy and Stability, section 3.1, any order).
# C_EPI = 12 = 4 + 8: the epilogue adds at most 4 roundings (alpha * acc, + bias, resid + C_old, the final add; the
# split-K form has a single one, the fp32 rounding of its fp64 reduction), each of a value bounded by sum |terms|; the
# other 8 make the first-order expression a true bound: (1 + u)^(n + 4) - 1 <= (n + 4) u + ((n + 4) u)^2 / 2 * 1.001 and
# ((n + 4) u)^2 / 2 <= 7.9 u for every n <= 16 200, the longest contraction used here.
C_EPI = 12


def rounding_bound(nterms, abs_sum, c=C_EPI):
    return (nterms + c) * U * np.asarray(abs_sum, np.float64)


def pad4(v):
    return (v + 3) // 4 * 4


def cdiv(a, b):
    return -(-a // b)


def ints(seed, shape, lo=-4, hi=4):
    n = int(np.prod(shape))
    return (lo + (synth.splitmix64(seed, n) % np.uint64(hi - lo + 1)).astype(np.int64)).astype(np.float32).reshape(shape)


def data(mode, seed, shape, std=1.0):
    return ints(seed, shape) if mode == "exact" else synth.normal(seed, shape, 0.0, std)


def f64(a):
    return np.asarray(a, np.float64)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def erf64(z):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(f64(z)))).numpy()


def gelu64(z):
    z = f64(z)
    return 0.5 * z * (1.0 + erf64(z / math.sqrt(2.0)))


def gelu_grad64(z):
    """d/dz of erf-GELU: Phi(z) + z phi(z)."""
    z = f64(z)
    return 0.5 * (1.0 + erf64(z / math.sqrt(2.0))) + z * np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


# --------------------------------------------------------------------------------------------- strided layouts
class Layout:
    """Where a logical [Z, R, C] array sits in a flat buffer: element (z, r, c) at base(z) + r * ld + c with
    base(z) = (z // H) * sb + (z % H) * sh (the two-level batch strides of eav_gemm_f32)."""

    def __init__(self, Z, R, C, ld, H=1, sb=0, sh=0):
        assert ld >= C and Z % H == 0
        self.Z, self.R, self.C, self.ld, self.H, self.sb, self.sh = Z, R, C, ld, H, sb, sh

    def index(self):
        z = np.arange(self.Z, dtype=np.int64)
        base = (z // self.H) * self.sb + (z % self.H) * self.sh
        return (base[:, None, None] + np.arange(self.R, dtype=np.int64)[None, :, None] * self.ld
                + np.arange(self.C, dtype=np.int64)[None, None, :])

    def span(self):
        return (self.Z - 1) // self.H * self.sb + (self.H - 1) * self.sh + (self.R - 1) * self.ld + self.C

    def distinct(self):
        idx = self.index().ravel()
        return np.unique(idx).size == idx.size


def store(layout, values, fill=BIG, tail=64):
    """Flat fp32 buffer holding `values` ([Z, R, C]) in `layout`; every other word (pad columns, gaps between slabs and
    `tail` words past the end) holds `fill`."""
    buf = np.full(layout.span() + tail, fill, np.float32)
    buf[layout.index()] = np.asarray(values, np.float32).reshape(layout.Z, layout.R, layout.C)
    return buf


class Guarded:
    """One buffer [guard | n words | guard'] filled with the NaN sentinel, on any torch device.  Outputs live in the
    middle (`ptr(off)`); `check(index)` asserts bit for bit that every word outside `index` - guard bands, pad columns,
    gaps between slabs - still holds the sentinel and that every word inside was written, and returns those words.
    guard' covers `slack` words past the end as well (e.g. a full tile of rows), so that a write past an edge tile lands
    in the band and is reported, not in someone else's memory."""

    def __init__(self, n, device, slack=0):
        self.n, self.after = int(n), GUARD + int(slack)
        self.buf = torch.full((GUARD + self.n + self.after,), SENT, dtype=torch.int32, device=device).view(torch.float32)

    def ptr(self, off=0):
        return self.buf.data_ptr() + 4 * (GUARD + off)

    def body(self):
        return self.buf[GUARD:GUARD + self.n]

    def fill(self, index, values):
        """Pre-set the words at `index` (a value to accumulate into, an in-place operand)."""
        v = torch.from_numpy(np.ascontiguousarray(values, np.float32).ravel()).to(self.buf.device)
        self.buf[torch.from_numpy(GUARD + np.asarray(index, np.int64).ravel()).to(self.buf.device)] = v

    def check(self, index, what, all_written=True):
        if self.buf.is_cuda:
            torch.cuda.synchronize()
        h = self.buf.cpu().view(torch.int32).numpy()
        index = np.asarray(index, np.int64)
        outside = np.ones(h.size, bool)
        outside[GUARD + index.ravel()] = False
        bad = np.flatnonzero(outside & (h != SENT))
        assert bad.size == 0, (f"{what}: {bad.size} words outside the output were written (first at offset "
                               f"{int(bad[0]) - GUARD} of an output of {self.n})")
        got = h[GUARD + index]
        if all_written:
            unwritten = int((got == SENT).sum())
            assert unwritten == 0, f"{what}: {unwritten} of {got.size} output words never written"
        return got.view(np.float32)


def compare(mode, got, want64, abs64, nterms, what, c=C_EPI):
    """exact: bit equality with the float64 result; rounded: the derived bound, element by element."""
    got, want64 = f64(got), f64(want64)
    assert got.shape == want64.shape, (what, got.shape, want64.shape)
    if mode == "exact":
        ne = got != want64
        assert not ne.any(), f"{what}: {int(ne.sum())} elements not bit-exact (max |diff| {np.abs(got - want64).max():.3e})"
    else:
        err = np.abs(got - want64)
        bound = rounding_bound(nterms, abs64, c)
        over = ~(err <= bound)              # (a NaN is beyond any bound)
        assert not over.any(), (f"{what}: {int(over.sum())} elements beyond (n + {c}) u sum|terms|, worst "
                                f"{float(np.nanmax(err / np.maximum(bound, 1e-300))):.2f} x the bound")


def close(got, ref, rtol, atol, what=""):
    got, ref = f64(got), f64(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    assert (err <= atol + rtol * np.abs(ref)).all(), f"{what}: max err {np.nanmax(err):.3e}, ref max {np.abs(ref).max():.3e}"


# --------------------------------------------------------------------------------------------------- GEMM
def gemm_ref(a, b, alpha=1.0, bias=None, gelu=False, resid=None, prev=None):
    """a [Z, M, K], b [Z, K, N] (op() already applied).  Returns (out, pre, abs): out = act(alpha a.b + bias) + resid
    + prev, pre = the value before the activation, abs = the sum of the absolute terms of out (without activation)."""
    a, b = f64(a), f64(b)
    pre = alpha * np.matmul(a, b)
    ab = abs(alpha) * np.matmul(np.abs(a), np.abs(b))
    if bias is not None:
        pre = pre + f64(bias)
        ab = ab + np.abs(f64(bias))
    out = gelu64(pre) if gelu else pre.copy()
    for extra in (resid, prev):
        if extra is not None:
            out = out + f64(extra)
            ab = ab + np.abs(f64(extra))
    return out, pre, ab


def splitk_slice(K, nsplit):
    """Length of a K slice of eav_gemm_f32_splitk (a multiple of the K tile, 16) for a plan of nsplit slices."""
    return cdiv(cdiv(K, nsplit), 16) * 16 if nsplit > 1 else K


def splitk_ref(a, b):
    """a [M, K], b [K, N]: the product and the sum of its absolute terms.  Each slice is an fp32 chain of at most
    splitk_slice() terms; the slices are summed in fp64 and rounded once (covered by C_EPI)."""
    a, b = f64(a), f64(b)
    return a @ b, np.abs(a) @ np.abs(b)


class GemmCase:
    """Operands of one eav_gemm_f32 call in their stored layouts.  Logical a [Z, M, K], b [Z, K, N]; A is stored
    [M, K] (tA = 0) or [K, M] (tA = 1), B [N, K] (tB = 0) or [K, N] (tB = 1), leading dimensions multiples of 4 with at
    least 4 pad columns holding BIG.  Z > 1: the heads of an image interleave along the columns (head stride = a padded
    width), the images follow each other with a gap - the two-level strides of the attention products."""

    def __init__(self, mode, M, N, K, tA, tB, Z=1, H=1, seed=0, std_b=0.25):
        self.mode, self.M, self.N, self.K, self.tA, self.tB, self.Z, self.H = mode, M, N, K, tA, tB, Z, H
        self.a = data(mode, seed_of("a", seed, M, N, K, Z), (Z, M, K))
        self.b = data(mode, seed_of("b", seed, M, N, K, Z), (Z, K, N), std_b)
        ra, ca = (K, M) if tA else (M, K)
        rb, cb = (K, N) if tB else (N, K)
        self.LA = self._layout(ra, ca)
        self.LB = self._layout(rb, cb)
        self.lda, self.ldb = self.LA.ld, self.LB.ld
        self.A = store(self.LA, self.a.transpose(0, 2, 1) if tA else self.a)
        self.B = store(self.LB, self.b if tB else self.b.transpose(0, 2, 1))
        # C: heads side by side with pad columns each, 4 more at the end of a row, a gap of 8 between images
        wc = pad4(N) + 4
        self.LC = Layout(Z, M, N, H * wc + 4, H, M * (H * wc + 4) + 8, wc) if Z > 1 else Layout(1, M, N, N + 3)
        self.ldc = self.LC.ld

    def _layout(self, rows, cols):
        w = pad4(cols) + 4
        if self.Z == 1:
            return Layout(1, rows, cols, w)
        ld = self.H * w + 4
        return Layout(self.Z, rows, cols, ld, self.H, rows * ld + 8, w)

    def strides(self, L):
        return (L.sb, L.sh) if self.Z > 1 else (0, 0)


# ------------------------------------------------------------------------------------------------ softmax
def softmax_ref(s):
    s = f64(s)
    e = np.exp(s - s.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def softmax_bwd_ref(p, dp):
    p, dp = f64(p), f64(dp)
    return p * (dp - (dp * p).sum(-1, keepdims=True))


SOFTMAX_N = [1, 63, 64, 65, 256, 257, 1280, 1281, 2047, 2048]
SOFTMAX_ROWS = 6


def softmax_rows(N):
    """6 rows (more than one block of 4, not a multiple of 4): three normal ones, one spanning +-80 (wrong without the
    max subtraction), one constant, one whose maximum sits in the last column."""
    s = synth.normal(seed_of("softmax", N), (SOFTMAX_ROWS, N), 0.0, 2.0)
    s[3] = np.linspace(80.0, -80.0, N, dtype=np.float32) if N > 1 else 80.0
    s[4] = 0.375
    s[5, N - 1] = 9.0
    return s


def softmax_instance(N):
    """Registers per lane of the instantiation eav_softmax_* takes (rows of up to 64 * NPL columns)."""
    return 4 if N <= 256 else 20 if N <= 1280 else 32


# ---------------------------------------------------------------------------------------------- LayerNorm
def layernorm_fwd_ref(x, gamma, beta, eps):
    x = f64(x)
    mean = x.mean(-1)
    var = ((x - mean[:, None]) ** 2).mean(-1)
    rstd = 1.0 / np.sqrt(var + eps)
    return (x - mean[:, None]) * rstd[:, None] * f64(gamma) + f64(beta), mean, rstd


def layernorm_bwd_ref(dy, x, gamma, mean, rstd):
    """dx, dgamma, dbeta and the absolute sums of the last two, from the saved statistics."""
    dy, x = f64(dy), f64(x)
    xhat = (x - f64(mean)[:, None]) * f64(rstd)[:, None]
    gd = dy * f64(gamma)
    m1, m2 = gd.mean(-1, keepdims=True), (gd * xhat).mean(-1, keepdims=True)
    dx = f64(rstd)[:, None] * (gd - m1 - xhat * m2)
    return dx, (dy * xhat).sum(0), dy.sum(0), np.abs(dy * xhat).sum(0), np.abs(dy).sum(0)


# (32789, 8): wave 0 of block 0 reaches a second group of 16 rows (row 32768 on) and the last group has 5 rows
LN_SHAPES = [(1, 4), (5, 8), (7, 252), (6, 256), (3, 260), (5, 1020), (9, 1024), (32789, 8)]
LN_EPS = 1e-12


def layernorm_inputs(M, D):
    x = synth.normal(seed_of("ln x", M, D), (M, D), 0.3, 2.0)
    dy = synth.normal(seed_of("ln dy", M, D), (M, D))
    keep = np.ones(M, bool)
    if M > 1:
        x[1] = 0.467        # constant row (AST padding value): var = 0, eps = 1e-12 - checked for finiteness only
        dy[1] = 0
        keep[1] = False
    g = synth.uniform(seed_of("ln g", D), (D,), 0.5, 1.5)
    b = synth.normal(seed_of("ln b", D), (D,), 0, 0.1)
    old = ints(seed_of("ln old", M, D), (M, D))
    return x, g, b, dy, old, keep


# ---------------------------------------------------------------------------------- element-wise / row kernels
GELU_N = [4, 1028, 4 * (4096 * 256 + 300)]       # the last: some threads of the 4096-block grid make a second pass


def gelu_inputs(n):
    pre, d = synth.normal(seed_of("gelu pre", n), (n,), 0, 2.0), synth.normal(seed_of("gelu d", n), (n,))
    pre[:4] = [0.0, 12.0, -12.0, 1e-40]
    if n > 8:
        pre[n - 3:] = [12.0, -1e-40, -12.0]
    return pre, d


def gelu_bwd_ref(d, pre):
    return f64(d) * gelu_grad64(pre)


COLSUM_SHAPES = [(1, 1, 1), (255, 63, 63), (256, 64, 70), (257, 65, 68), (1000, 200, 203)]


def colsum_ref(dy):
    return f64(dy).sum(0), np.abs(f64(dy)).sum(0)


def im2col_ref(x, P, sy, sx, transposed):
    """col[(b, py, px), (c, i, j)] = img[b, c, py sy + i, px sx + j]; transposed: x is [B, W, H], one channel."""
    x = np.asarray(x)
    img = x.transpose(0, 2, 1)[:, None] if transposed else x
    B, C, H, W = img.shape
    ny, nx = (H - P) // sy + 1, (W - P) // sx + 1
    col = np.empty((B, ny, nx, C, P, P), img.dtype)
    for py in range(ny):
        for px in range(nx):
            col[:, py, px] = img[:, :, py * sy:py * sy + P, px * sx:px * sx + P]
    return col.reshape(B * ny * nx, C * P * P)


# (name, B, C, H, W, P, stride, transposed): the ViT view and the AST view beyond 1 048 576 items (a second grid-stride
# pass), and maps whose last patch does not end at the border
IM2COL_CASES = [("vit_b8", 8, 3, 224, 224, 16, 16, 0), ("ast_b4", 4, 1, 128, 1024, 16, 10, 1),
                ("ragged", 3, 2, 37, 45, 16, 10, 0), ("ragged_t", 3, 1, 37, 45, 16, 10, 1)]


def im2col_input(name, B, C, H, W, transposed):
    return synth.normal(seed_of("im2col", name), (B, W, H) if transposed else (B, C, H, W))


def embed_finish_ref(h, cls, dist, pos, nextra):
    """h[b, t] = (t < nextra ? token t : h[b, t]) + pos[t]: one fp32 addition per element (float64 holds it exactly
    for these magnitudes, so its fp32 rounding is the fp32 sum)."""
    r = f64(h).copy()
    r[:, 0] = f64(cls)
    if nextra == 2:
        r[:, 1] = f64(dist)
    return r + f64(pos)


def embed_bwd_ref(dh, nextra):
    """dpos = sum over the batch (and the sum of the absolute terms), demb = the patch rows, batch-major."""
    dh = f64(dh)
    return dh.sum(0), np.abs(dh).sum(0), dh[:, nextra:].reshape(-1, dh.shape[-1])


# (B, ntok, D, nextra); the third makes B ntok D / 4 exceed 1 048 576 float4s (embed_finish), the fourth ntok D / 4
# (embed_bwd loops over the tokens of one image)
EMBED_CASES = [(3, 7, 4, 1), (3, 7, 4, 2), (6, 1214, 768, 2), (2, 5500, 768, 1)]


def token_rows_ref(h, rows, nextra, scatter):
    """gather: rows[b nextra + e] = h[b, e]; scatter: the same rows of h replaced, every other row untouched."""
    if not scatter:
        return np.asarray(h)[:, :nextra].reshape(-1, h.shape[-1]).copy()
    out = np.asarray(h).copy()
    out[:, :nextra] = np.asarray(rows).reshape(h.shape[0], nextra, h.shape[-1])
    return out


# (B, ntok, D, nextra); the last: B nextra D / 4 > 1 048 576
TOKEN_CASES = [(3, 7, 8, 2), (5, 4, 12, 1), (2740, 3, 768, 2)]


def pair_mean_ref(seq):
    s = f64(seq).reshape(-1, 2, seq.shape[-1])
    return (s[:, 0] + s[:, 1]) * 0.5


def pair_mean_bwd_ref(dpooled):
    return np.repeat(f64(dpooled) * 0.5, 2, axis=0)


# (B, D): D no multiple of 4; the last: B D > 1 048 576
PAIR_CASES = [(3, 7), (5, 770), (1400, 770)]


# ------------------------------------------------------------------------------------------- GEMM case lists
# (M, N, Z, H, form): the smallest shapes that reach the 128-row tiles (cdiv(M, 128) cdiv(N, BN) Z >= 640 and M > 64)
GEMM_BIG = [(40970, 130, 1, 1, 128128),     # 321 x 2 = 642 blocks; last row tile 10 rows, last column tile 2 columns
            (81930, 40, 1, 1, 128064),      # 641 blocks of 128 x 64, 40 of the 64 columns
            (81930, 64, 1, 1, 128064),      # the same with an exact column tile
            (130, 130, 160, 4, 128128),     # 2 x 2 x 160 = 640 blocks, two-level strides
            (130, 40, 320, 4, 128064)]      # 2 x 1 x 320 = 640
GEMM_BIG_K = [32, 37]                       # 32: interior tiles beside guarded edge tiles; 37: all guarded, K tail
# (M, N, K, form): both sides of the M <= 64 / N <= 64 rules
GEMM_SMALL = [(1, 1, 1, 64064), (64, 64, 16, 64064), (65, 65, 17, 64128)]
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]

# epilogue options, each alone or in the pairs the encoder issues: (name, alpha, bias, gelu, pre, resid, accumulate)
EPILOGUES = [("bias", 1.0, 1, 0, 0, 0, 0), ("bias_gelu", 1.0, 1, 1, 0, 0, 0), ("bias_gelu_pre", 1.0, 1, 1, 1, 0, 0),
             ("resid", 1.0, 0, 0, 0, 1, 0), ("bias_resid", 1.0, 1, 0, 0, 1, 0), ("acc_half", 0.5, 0, 0, 0, 0, 1),
             ("acc_resid", 1.0, 0, 0, 0, 1, 1)]
# (M, N, K, form): the unbatched 128-row shapes at K = 37 and one 64-row shape with N % 4 != 0
EPILOGUE_SHAPES = [(40970, 130, 37, 128128), (81930, 40, 37, 128064), (81930, 64, 37, 128064), (200, 137, 72, 64128)]

# (M, N, K, nz, form, reduce): reduce 2 = the wide reduce (nz >= 16 and M N <= 2^18), 1 = the plain one
SPLITK_CASES = [(300, 500, 16200, 64, 128128, 2),   # ragged M and N tiles, last slice 72 long (72 % 16 = 8)
                (40, 160, 4100, 17, 64128, 2),      # nz no multiple of the 8 reduce lanes, ShallowConvNet output size
                (200, 40, 700, 3, 64064, 1)]        # plain-reduce control (from test_gemm_splitk_weight_gradient)


def splitk_layouts(M, N, K):
    return LAYOUTS if (M, N, K) != (40, 160, 4100) else [(1, 1)]


def gemm_instances():
    """Every (BM, BN, tA, tB) the case lists are meant to run, from their stated forms."""
    s = set()
    for M, N, Z, H, form in GEMM_BIG:
        s |= {(form // 1000, form % 1000, tA, tB) for tA, tB in LAYOUTS}
    for M, N, K, form in GEMM_SMALL:
        s |= {(form // 1000, form % 1000, tA, tB) for tA, tB in LAYOUTS}
    return s
