// EEGNet "separableConv" (dense 64 -> 64 channels, 16 taps, 'same' padding 7 / 8 - nn.Conv2d(64, 64, (1,16), padding='same',
// bias=False), CNN_torch/EEGNet_tor.py:37,59) and its data gradient in the frequency domain, exact fp32 arithmetic.
//
// The direct form is a K = 1024 contraction per output (64 input channels x 16 taps): 20.97 GFLOP per pass at [64,64,2500],
// 0.18 ms on the fp32 matrix cores (eegnet_conv64.hip, 0.73-0.76 of the 157 TFLOP/s peak).  With overlap-save blocks of 64
// samples (49 valid outputs) the tap dimension disappears: per frequency bin the 64 x 64 channel mixing is ONE complex
// matrix-vector product,
//     Y_o[m] = sum_i conj(W_oi[m]) X_i[m]                (W_oi = FFT of the 16 taps of filter (o, i))
// i.e. 64 bins x a [128 x 128] real matrix instead of a [64 x 1024] one: 6 x fewer multiply-adds, and they are still
// plain GEMMs for the fp32 MFMA.  Two blocks of the same sample travel as ONE complex signal (block A real, block B
// imaginary): every step - FFT, complex-linear mixing, inverse FFT - keeps them apart (real filters), no unpacking.
//
// Three kernels + the filter spectra:
//   c64_spectra_wave     BmT[bin][(ri_i, i)][(ri_o, o)] = the transpose of [[Gr, -Gi], [Gi, Gr]], G = conj(W) / 64 (forward), or the
//                        flipped / transposed filters of the data gradient - the leading workgroups of the pack launch
//   c64_pack_fft_kernel  a wave per column (sample b, block pair): coalesced row loads -> LDS transpose -> lane = channel,
//                        64-point complex FFT entirely in registers (8 x 8, no exchange) -> Z[bin][col][re | im][64 ch]
//   c64_pack_bwd_kernel  the backward's pack: BOTH spectra of a du block pair from one load (64-sample window of the data
//                        gradient; its samples 8 .. 56, zero-padded, are the weight gradient's block), du itself optionally
//                        formed from dp3 / u3 while loading (the backward of separableBN -> ELU -> AvgPool8 -> Dropout)
//   c64_bin_gemm_kernel  per bin C[cols x 128] = Z[cols x 128] . Bm^T on v_mfma_f32_32x32x2_f32, weight-stationary (a wave
//                        keeps its 32 outputs x 128 contraction rows of Bm in 64 VGPRs), column tiles through LDS
//   c64_ifft_unpack_kernel  lane = output channel: inverse FFT in registers, BatchNorm sums per channel (= per lane),
//                        LDS transpose, coalesced row stores
// Spectra layout [bin][col][2][64]: every global access of all three kernels is a whole 256-byte row segment.
#include <algorithm>

#include "eav_common.h"
#include "../../include/eav_hip.h"

namespace {

constexpr int NCH = 64, KT = 16, NB = 64, LV = NB - KT + 1;      // 49 valid outputs per 64-sample block
constexpr int PADF = (KT - 1) / 2, PADB = KT / 2;      // left padding of the forward (7) / of the data gradient (8)
typedef float v2f __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;
constexpr float C64[50] = {1.0f, 0.995184727f, 0.98078528f, 0.956940336f, 0.923879533f, 0.881921264f, 0.831469612f, 0.773010453f, 0.707106781f, 0.634393284f, 0.555570233f, 0.471396737f, 0.382683432f, 0.290284677f, 0.195090322f, 0.0980171403f, 0.0f, -0.0980171403f, -0.195090322f, -0.290284677f, -0.382683432f, -0.471396737f, -0.555570233f, -0.634393284f, -0.707106781f, -0.773010453f, -0.831469612f, -0.881921264f, -0.923879533f, -0.956940336f, -0.98078528f, -0.995184727f, -1.0f, -0.995184727f, -0.98078528f, -0.956940336f, -0.923879533f, -0.881921264f, -0.831469612f, -0.773010453f, -0.707106781f, -0.634393284f, -0.555570233f, -0.471396737f, -0.382683432f, -0.290284677f, -0.195090322f, -0.0980171403f, 0.0f, 0.0980171403f};
constexpr float S64[50] = {0.0f, 0.0980171403f, 0.195090322f, 0.290284677f, 0.382683432f, 0.471396737f, 0.555570233f, 0.634393284f, 0.707106781f, 0.773010453f, 0.831469612f, 0.881921264f, 0.923879533f, 0.956940336f, 0.98078528f, 0.995184727f, 1.0f, 0.995184727f, 0.98078528f, 0.956940336f, 0.923879533f, 0.881921264f, 0.831469612f, 0.773010453f, 0.707106781f, 0.634393284f, 0.555570233f, 0.471396737f, 0.382683432f, 0.290284677f, 0.195090322f, 0.0980171403f, 0.0f, -0.0980171403f, -0.195090322f, -0.290284677f, -0.382683432f, -0.471396737f, -0.555570233f, -0.634393284f, -0.707106781f, -0.773010453f, -0.831469612f, -0.881921264f, -0.923879533f, -0.956940336f, -0.98078528f, -0.995184727f, -1.0f, -0.995184727f};

__device__ __forceinline__ v2f cmul(v2f a, v2f b) { return a.xx * b + a.yy * (v2f){-b.y, b.x}; }
__device__ __forceinline__ v2f cmulc(v2f a, v2f b) { return a.xx * (v2f){b.x, -b.y} + a.yy * (v2f){b.y, b.x}; }
template <bool INV>
__device__ __forceinline__ v2f twmul(v2f a, v2f w) { return INV ? cmulc(a, w) : cmul(a, w); }
template <bool INV>
__device__ __forceinline__ v2f rot(v2f a) { return INV ? (v2f){-a.y, a.x} : (v2f){a.y, -a.x}; }      // x (-i) / x (+i)

template <bool INV>
__device__ __forceinline__ void dft4(v2f& a0, v2f& a1, v2f& a2, v2f& a3) {
  const v2f t0 = a0 + a2, t1 = a0 - a2, t2 = a1 + a3, t3 = rot<INV>(a1 - a3);
  a0 = t0 + t2; a1 = t1 + t3; a2 = t0 - t2; a3 = t1 - t3;
}

// 8-point DFT, natural order in and out
template <bool INV>
__device__ __forceinline__ void dft8(v2f& a0, v2f& a1, v2f& a2, v2f& a3, v2f& a4, v2f& a5, v2f& a6, v2f& a7) {
  constexpr float R = 0.70710678118654752f;
  dft4<INV>(a0, a2, a4, a6);      // E0..E3 in a0, a2, a4, a6
  dft4<INV>(a1, a3, a5, a7);      // O0..O3 in a1, a3, a5, a7
  const v2f t0 = a1, t1 = twmul<INV>(a3, (v2f){R, -R}), t2 = rot<INV>(a5), t3 = twmul<INV>(a7, (v2f){-R, -R});
  const v2f e0 = a0, e1 = a2, e2 = a4, e3 = a6;
  a0 = e0 + t0; a1 = e1 + t1; a2 = e2 + t2; a3 = e3 + t3;
  a4 = e0 - t0; a5 = e1 - t1; a6 = e2 - t2; a7 = e3 - t3;
}

// 64-point complex FFT of one lane's registers: x[n] in, X[k] out at x[pos64(k)] (8 x 8, digit-reversed output: all
// indices are compile-time constants, the permutation costs nothing).  INV: conjugate twiddles, no 1/N.
__host__ __device__ constexpr int pos64(int k) { return 8 * (k & 7) + (k >> 3); }

template <bool INV>
__device__ __forceinline__ void fft64(v2f (&x)[64]) {
#pragma unroll
  for (int n2 = 0; n2 < 8; ++n2)
    dft8<INV>(x[n2], x[8 + n2], x[16 + n2], x[24 + n2], x[32 + n2], x[40 + n2], x[48 + n2], x[56 + n2]);
#pragma unroll
  for (int k1 = 1; k1 < 8; ++k1)
#pragma unroll
    for (int n2 = 1; n2 < 8; ++n2) x[8 * k1 + n2] = twmul<INV>(x[8 * k1 + n2], (v2f){C64[n2 * k1], -S64[n2 * k1]});
#pragma unroll
  for (int k1 = 0; k1 < 8; ++k1)
    dft8<INV>(x[8 * k1], x[8 * k1 + 1], x[8 * k1 + 2], x[8 * k1 + 3], x[8 * k1 + 4], x[8 * k1 + 5], x[8 * k1 + 6],
              x[8 * k1 + 7]);
}

struct Geo {
  int B, T, padl, nblk, npair, ncol, ncolp;      // ncolp = columns rounded up to 128: whole 32-column GEMM tiles and 4 equal
                                                 // weight-gradient chunks of whole 32-column K-blocks; columns >= ncol are ZERO
};

Geo geometry(int B, int T, int padl) {
  Geo g;
  g.B = B; g.T = T; g.padl = padl;
  g.nblk = cdiv(T, LV);
  g.npair = cdiv(g.nblk, 2);
  g.ncol = B * g.npair;
  g.ncolp = cdiv(g.ncol, 128) * 128;
  return g;
}

// ---------------------------------------------------------------------------------------------------------- filter spectra
// BmT[bin][k = (ri_i, in)][n = (ri_o, out)] (contraction index major: the GEMM's weight-stationary waves then load their
// operand registers as whole 128-byte rows).  One wave per input channel `in`, lane = output channel `out`.
// Table 0 (forward): filter (out, in) = w[out][in][:]; table 1 (data gradient: dp2[i] = sum_o w'[i][o] * du[o],
// w'[i][o][k'] = w[o][i][15 - k']): out = i, in = o.
__device__ __forceinline__ void c64_spectra_wave(const float* __restrict__ w, float* __restrict__ Bm, int in, int bwd,
                                                 int lane) {
  v2f x[64];
#pragma unroll
  for (int n = 0; n < 64; ++n) {
    float t = 0.f;
    if (n < KT) t = bwd ? w[((int64_t)in * NCH + lane) * KT + (KT - 1 - n)] : w[((int64_t)lane * NCH + in) * KT + n];
    x[n] = (v2f){t, 0.f};
  }
  fft64<false>(x);
#pragma unroll
  for (int m = 0; m < 64; ++m) {
    const v2f W = x[pos64(m)];
    const float gr = W.x * (1.0f / NB), gi = -W.y * (1.0f / NB);      // G = conj(W) / 64
    float* row0 = Bm + ((int64_t)m * 128 + in) * 128;                 // contraction row (re, in)
    float* row1 = Bm + ((int64_t)m * 128 + 64 + in) * 128;            // contraction row (im, in)
    row0[lane] = gr;   row0[64 + lane] = gi;                          // y_re += gr z_re,  y_im += gi z_re
    row1[lane] = -gi;  row1[64 + lane] = gr;                          // y_re -= gi z_im,  y_im += gr z_im
  }
}

// ------------------------------------------------------------------------------------------------------------ pack + FFT
// A wave per column.  Rows of 64 samples are loaded coalesced (lane = sample), transposed through a [64][65] LDS tile and
// read back with lane = channel (bank (lane + n) mod 32: conflict-free); block A -> real parts, block B -> imaginary parts.
constexpr int TS = 65;

// x[ch] = (sample `lane` of block A, of block B) of channel ch  ->  x[n] = sample n of channel `lane`
__device__ __forceinline__ void pack_transpose(float* tile, v2f (&x)[64], int lane) {
#pragma unroll
  for (int half = 0; half < 2; ++half) {
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) tile[ch * TS + lane] = half == 0 ? x[ch].x : x[ch].y;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    float r[64];
#pragma unroll
    for (int n = 0; n < 64; ++n) r[n] = tile[lane * TS + n];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int n = 0; n < 64; ++n) {
      if (half == 0) x[n].x = r[n]; else x[n].y = r[n];
    }
  }
}

__device__ __forceinline__ void pack_store(float* __restrict__ Z, const v2f (&x)[64], int col, int ncolp, int lane) {
  float* dst = Z + (int64_t)col * 128 + lane;
#pragma unroll
  for (int m = 0; m < 64; ++m) {
    dst[(int64_t)m * ncolp * 128] = x[pos64(m)].x;
    dst[(int64_t)m * ncolp * 128 + 64] = x[pos64(m)].y;
  }
}

// vonly: the block is its 49 valid samples, zero-padded (the du operand of the weight gradient), instead of 64 samples
// starting padl before the block (forward / data gradient inputs).
// The first nspec workgroups form the filter spectra instead (a wave per input channel; tables bwd0 .. of Bm0): the per-bin
// GEMM is the first reader of both, so the tables need no launch - no graph node on the critical path - of their own.
__global__ __launch_bounds__(256) void c64_pack_fft_kernel(const float* __restrict__ in, float* __restrict__ Z, Geo g,
                                                           int vonly, const float* __restrict__ w, float* __restrict__ Bm0,
                                                           int nspec, int bwd0) {
  __shared__ float tiles[4][64 * TS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if ((int)blockIdx.x < nspec) {
    const int job = blockIdx.x * 4 + wave, table = job >> 6;
    c64_spectra_wave(w, Bm0 + (int64_t)table * 64 * 128 * 128, job & 63, bwd0 + table, lane);
    return;
  }
  float* tile = tiles[wave];
  const int nwaves = (gridDim.x - nspec) * 4;
  for (int col = (blockIdx.x - nspec) * 4 + wave; col < g.ncolp; col += nwaves) {
    if (col >= g.ncol) {                       // padding column: zero spectra (the weight gradient contracts over columns)
      float* dz = Z + (int64_t)col * 128 + lane;
#pragma unroll 8
      for (int m = 0; m < 64; ++m) {
        dz[(int64_t)m * g.ncolp * 128] = 0.f;
        dz[(int64_t)m * g.ncolp * 128 + 64] = 0.f;
      }
      continue;
    }
    const int b = col / g.npair, pr = col - b * g.npair;
    v2f x[64];
    // all 128 row loads of the column are issued before the first one is consumed (8 at a time left the kernel waiting on
    // HBM latency 16 times per column: 45 us; x[] doubles as the landing zone)
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int blk = 2 * pr + half;
      const int t = blk * LV - (vonly ? 0 : g.padl) + lane;
      const bool ok = blk < g.nblk && t >= 0 && t < g.T && (!vonly || lane < LV);
      const float* src = in + (int64_t)b * NCH * g.T + t;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const float v = ok ? src[(int64_t)ch * g.T] : 0.f;
        if (half == 0) x[ch].x = v; else x[ch].y = v;
      }
    }
    pack_transpose(tile, x, lane);
    fft64<false>(x);
    pack_store(Z, x, col, g.ncolp, lane);
  }
}

// ------------------------------------------------------------------------------------------------- backward pack + 2 FFTs
// The separableConv backward needs two spectra of du: of the 64-sample windows that start 8 samples before each block (data
// gradient -> Zb) and of the blocks' 49 valid samples, zero-padded (weight gradient -> D).  The second block is samples
// 8 .. 56 of the first: after the transpose both are compile-time register indices of ONE load of the column.
// FUSE: du is not read but formed per loaded sample from u3 (separableConv output) and dp3 (gradient of the pooled,
// dropped-out block-2 output) with pool_bwd_apply_kernel<8>'s arithmetic (pool_bwd_du) - no du tensor in HBM.  The pooled
// gradient x dropout multiplier of a (channel, pooling window) is formed ONCE per column (a 64-sample window touches at most
// 9 pooling windows: 576 values per block, 9 per lane) and handed to the 8 lanes of the window through the (still idle) tile.
struct DuSrc {
  const float *dp, *u, *bn, *m12;      // dp3 [B,64,T/8], u3 [B,64,T], bn = mean, invstd, scale, shift [64] each, m1 m2 [64] each
  float drop_p;
  uint64_t seed;
  const uint8_t* mask;
  const uint64_t* seed_dev;
};
constexpr int NPW = 9;      // pooling windows a 64-sample window can touch

template <bool FUSE>
__global__ __launch_bounds__(256, 2) void c64_pack_bwd_kernel(const float* __restrict__ du, DuSrc s, float* __restrict__ Zb,
                                                           float* __restrict__ D, Geo g) {
  __shared__ float tiles[4][64 * TS];
  __shared__ __attribute__((aligned(16))) float cst[FUSE ? 64 * 8 : 1];      // per channel: mean, invstd, scale, shift, m1, m2
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* tile = tiles[wave];
  uint64_t seed = 0;
  const int To = g.T / 8;
  if (FUSE) {
    seed = dropout_seed(s.seed, s.seed_dev);
    if (threadIdx.x < 64) {
#pragma unroll
      for (int k = 0; k < 4; ++k) cst[threadIdx.x * 8 + k] = s.bn[k * 64 + threadIdx.x];
      cst[threadIdx.x * 8 + 4] = s.m12[threadIdx.x];
      cst[threadIdx.x * 8 + 5] = s.m12[64 + threadIdx.x];
    }
    __syncthreads();
  }
  const int nwaves = gridDim.x * 4;
  for (int col = blockIdx.x * 4 + wave; col < g.ncolp; col += nwaves) {
    if (col >= g.ncol) {                       // padding column: zero spectra in both buffers
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        float* dz = (q ? D : Zb) + (int64_t)col * 128 + lane;
#pragma unroll 8
        for (int m = 0; m < 64; ++m) {
          dz[(int64_t)m * g.ncolp * 128] = 0.f;
          dz[(int64_t)m * g.ncolp * 128 + 64] = 0.f;
        }
      }
      continue;
    }
    const int b = col / g.npair, pr = col - b * g.npair;
    v2f x[64];
    const float* in = FUSE ? s.u : du;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int blk = 2 * pr + half;
      const int t = blk * LV - PADB + lane;
      const bool ok = blk < g.nblk && t >= 0 && t < g.T;
      const float* src = in + (int64_t)b * NCH * g.T + t;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const float v = ok ? src[(int64_t)ch * g.T] : 0.f;
        if (half == 0) x[ch].x = v; else x[ch].y = v;
      }
    }
    if (FUSE) {
      // (under the latency of the loads above) go[half][ch][w]: window to0 + w of row (b, ch)
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int blk = 2 * pr + half, to0 = (blk * LV - PADB) >> 3;      // arithmetic shift: floor (block 0 starts at -8)
#pragma unroll
        for (int i = 0; i < NCH * NPW / 64; ++i) {
          const int item = i * 64 + lane, ch = item / NPW, to = to0 + item - ch * NPW;
          float go = 0.f;
          if (blk < g.nblk && to >= 0 && to < To) {
            const uint64_t row = (uint64_t)b * NCH + ch, oi = row * To + to;
            go = s.dp[oi] * (1.0f / 8) * dropout_mult_row(s.drop_p, seed, s.mask, oi, row);
          }
          tile[half * NCH * NPW + item] = go;
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      int wofs[2];
      bool okh[2];
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int blk = 2 * pr + half, t = blk * LV - PADB + lane;
        okh[half] = blk < g.nblk && t >= 0 && t < g.T;
        wofs[half] = half * NCH * NPW + (t >> 3) - ((blk * LV - PADB) >> 3);
      }
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const f32x4 c0 = *reinterpret_cast<const f32x4*>(cst + ch * 8);
        const v2f c1 = *reinterpret_cast<const v2f*>(cst + ch * 8 + 4);
        float gd, ud;
        const float o0 = pool_bwd_du(x[ch].x, tile[wofs[0] + ch * NPW], c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, gd, ud);
        const float o1 = pool_bwd_du(x[ch].y, tile[wofs[1] + ch * NPW], c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, gd, ud);
        x[ch].x = okh[0] ? o0 : 0.f;
        x[ch].y = okh[1] ? o1 : 0.f;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    pack_transpose(tile, x, lane);
    // the weight gradient's block waits for the window's FFT: 65 of its 98 values per lane in the tile (idle now; [k][lane]:
    // a lane re-reads its own words), the rest in registers - all 98 in registers halve the occupancy (256 + 62 registers)
    constexpr int NPK = TS - LV;               // imaginary parts that still fit into the tile
    float yk[LV - NPK];
#pragma unroll
    for (int n = 0; n < LV; ++n) {
      tile[n * 64 + lane] = x[PADB + n].x;
      if (n < NPK) tile[(LV + n) * 64 + lane] = x[PADB + n].y;
      else yk[n - NPK] = x[PADB + n].y;
    }
    fft64<false>(x);
    pack_store(Zb, x, col, g.ncolp, lane);
#pragma unroll
    for (int n = 0; n < 64; ++n) {
      x[n] = (v2f){0.f, 0.f};
      if (n < LV) {
        x[n].x = tile[n * 64 + lane];
        x[n].y = n < NPK ? tile[(LV + n) * 64 + lane] : yk[n - NPK];
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    fft64<false>(x);
    pack_store(D, x, col, g.ncolp, lane);
  }
}

// ------------------------------------------------------------------------------------------------------- per-bin GEMM
// C[bin][col][n] = sum_k Z[bin][col][k] BmT[bin][k][n], n, k in [0,128).  grid (64 bins, GEMM_GW workgroups per bin) - the
// bin is blockIdx.x: consecutive workgroup ids go to consecutive XCDs, so the workgroups of a bin share one XCD's L2 and the
// bin's 64 KiB of filter spectra cross the fabric once, not once per workgroup (33 MB per launch, all of it in front of the
// first MFMA).  4 waves; wave w owns outputs [32 w, 32 w + 32): its Bm rows stay in 64 VGPRs (B operand of
// v_mfma_f32_32x32x2_f32: lane = (k & 1, n)).  Column tiles of 32 go global -> registers -> LDS (row stride 129: the
// A-operand reads AND the commit's writes hit 32 banks), one tile ahead of the MFMAs.  A tile of a wave: the fetch of tile
// t + 1, 64 MFMAs with their A operands read GEMM_AW MFMAs ahead (a rolling window of ds_reads, waited for by count), the
// 16 stores - which nothing in the loop waits for: they drain under the next tile's MFMAs -, the commit of tile t + 1.
// The waves of one workgroup meet at one barrier per tile; the other workgroup of the CU issues meanwhile.
// The contraction order per output is k = 0 .. 127: bit for bit the k-ordered fmaf chain.
constexpr int XS = 129;

#ifndef C64V_GW         // tuning builds: workgroups per bin of the per-bin GEMM (profiles/c64_gemm_before_after.txt)
#define C64V_GW 8
#endif
constexpr int GEMM_GW = C64V_GW, GEMM_AW = 8;

__global__ __launch_bounds__(256, 4) void c64_bin_gemm_kernel(const float* __restrict__ Z, const float* __restrict__ Bm,
                                                              float* __restrict__ C, int ncolp) {
  __shared__ float xs[2][32 * XS];
  const int bin = blockIdx.x, step = gridDim.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 31, kk = lane >> 5;
  const int ntiles = ncolp >> 5;
  // the walk starts at a tile that rotates with the bin: the workgroups that get one tile more than the others are not
  // the same blockIdx.y in every bin
  int tile = (blockIdx.y + bin) % step;
  const float* zb = Z + (int64_t)bin * ncolp * 128;
  float* cb = C + (int64_t)bin * ncolp * 128;
  // staging: thread -> column threadIdx.x >> 3, float4 pieces (threadIdx.x & 7) + 8 i: 128-byte runs in global memory, and
  // the 32 lanes of a half-wave write banks (4 g + (l >> 3) + 4 (l & 7) + j) mod 32 - all different
  const int scol = threadIdx.x >> 3, sk4 = threadIdx.x & 7;
  float4 pre[4];
  auto fetch = [&](int t) {
    const float4* src = reinterpret_cast<const float4*>(zb + ((int64_t)t * 32 + scol) * 128) + sk4;
#pragma unroll
    for (int i = 0; i < 4; ++i) pre[i] = src[8 * i];
  };
  auto commit = [&](int buf) {
    float* d = xs[buf] + scol * XS + 4 * sk4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      d[32 * i] = pre[i].x; d[32 * i + 1] = pre[i].y; d[32 * i + 2] = pre[i].z; d[32 * i + 3] = pre[i].w;
    }
  };
  if (tile < ntiles) fetch(tile);
  float wreg[64];
  {
    const float* bp = Bm + ((int64_t)bin * 128 + kk) * 128 + 32 * wave + n;      // BmT[bin][k][n]: 128-byte rows per half-wave
#pragma unroll
    for (int ks = 0; ks < 64; ++ks) wreg[ks] = bp[(int64_t)2 * ks * 128];
  }
  if (tile < ntiles) commit(0);
  // the weights are complete HERE: left to the first use, hipcc's waits for them (vmcnt counts loads and stores in one
  // queue) stay in the tile loop, where they wait for the previous tile's stores in front of the fifth MFMA
#pragma unroll
  for (int ks = 0; ks < 64; ++ks) asm volatile("" : "+v"(wreg[ks]));
  __syncthreads();
  for (int buf = 0; tile < ntiles; tile += step, buf ^= 1) {
    const int nxt = tile + step;
    if (nxt < ntiles) fetch(nxt);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float* ap = xs[buf] + n * XS + kk;
    float av[64];
#pragma unroll
    for (int ks = 0; ks < GEMM_AW; ++ks) av[ks] = ap[2 * ks];
#pragma unroll
    for (int ks = 0; ks < 64; ++ks) {
      if (ks + GEMM_AW < 64) av[ks + GEMM_AW] = ap[2 * (ks + GEMM_AW)];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[ks], wreg[ks], acc, 0, 0, 0);
    }
    // the order asked of the scheduler (hipcc pairs the reads into ds_read2_b32): the window first, then one read per two
    // MFMAs; left alone it reads each pair just in time, an LDS round trip in front of every second MFMA
    __builtin_amdgcn_sched_group_barrier(0x100, GEMM_AW / 2, 0);
#pragma unroll
    for (int i = 0; i < 32 - GEMM_AW / 2; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    }
    __builtin_amdgcn_sched_group_barrier(0x008, GEMM_AW, 0);
    // D[m = column][n = output]: lane holds output n, registers = columns (r & 3) + 8 (r >> 2) + 4 kk
    float* dst = cb + ((int64_t)tile * 32) * 128 + 32 * wave + n;
#pragma unroll
    for (int r = 0; r < 16; ++r) dst[(int64_t)((r & 3) + 8 * (r >> 2) + 4 * kk) * 128] = acc[r];
    if (nxt < ntiles) commit(buf ^ 1);        // (waits for the fetch, issued before the stores: not for the stores)
    // raw barrier: __syncthreads() would also wait for this tile's 16 global stores per lane (vmcnt(0)) at every tile
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
}

// ------------------------------------------------------------------------------------------------------- IFFT + unpack
// A wave per column, lane = output channel.  stat_part (optional): [waves][128] - sums and sums of squares per channel.
__global__ __launch_bounds__(256) void c64_ifft_unpack_kernel(const float* __restrict__ Y, float* __restrict__ out,
                                                              float* __restrict__ part, Geo g) {
  __shared__ float tiles[4][64 * TS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* tile = tiles[wave];
  const int nwaves = gridDim.x * 4, wg = blockIdx.x * 4 + wave;
  float s1 = 0.f, s2 = 0.f;
  for (int col = wg; col < g.ncol; col += nwaves) {
    const int b = col / g.npair, pr = col - b * g.npair;
    v2f x[64];
    const float* src = Y + (int64_t)col * 128 + lane;
#pragma unroll
    for (int m = 0; m < 64; ++m) {
      x[m].x = src[(int64_t)m * g.ncolp * 128];
      x[m].y = src[(int64_t)m * g.ncolp * 128 + 64];
    }
    fft64<true>(x);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int blk = 2 * pr + half, t0 = blk * LV;
      if (blk >= g.nblk) break;
#pragma unroll
      for (int j = 0; j < LV; ++j) {
        const float v = half == 0 ? x[pos64(j)].x : x[pos64(j)].y;
        tile[lane * TS + j] = v;
        if (t0 + j < g.T) {
          s1 += v;
          s2 += v * v;
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      float* dst = out + (int64_t)b * NCH * g.T + t0 + lane;
      const bool ok = lane < LV && t0 + lane < g.T;
#pragma unroll 8
      for (int ch = 0; ch < NCH; ++ch) {
        const float v = tile[ch * TS + lane];
        if (ok) dst[(int64_t)ch * g.T] = v;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
  }
  if (part) {
    part[(int64_t)wg * 128 + lane] = s1;
    part[(int64_t)wg * 128 + 64 + lane] = s2;
  }
}


// ------------------------------------------------------------------------------------------------------- weight gradient
// dW[o][i][k] = sum_{b,t} du[b,o,t] in[b,i,t+k-7] = Re IFFT_m( sum_cols conj(D_o[m]) Z_i[m] )[k], D = spectra of the
// zero-padded 49-sample blocks of du (two blocks per column: real + imaginary), Z = the forward's input spectra.  Per bin
// one real [128 x cols]^T [cols x 128] product P[a][b] = sum_col D[col][a] Z[col][b] (a = (re|im, o), b = (re|im, i)):
//   Re Acc[o][i] = P[(re,o)][(re,i)] + P[(im,o)][(im,i)],   Im Acc[o][i] = P[(re,o)][(im,i)] - P[(im,o)][(re,i)].
// c64_bin_wgemm_kernel: grid (column chunks, 64 bins), 4 waves, one workgroup per CU; wave w = rows a in [32 w, 32 w + 32),
// all 128 columns b (four 32 x 32 accumulators).  The D and Z slabs of a K-block of WKB columns (2 x 16 KiB, contiguous
// in global memory) are staged ONCE per workgroup by LDS-DMA (global_load_lds_dwordx4: no VGPR round trip, no ds_write)
// into a ring of WNST stages; for a fixed column the 32 lanes of a half-wave read 128 consecutive bytes of LDS.  Block
// kb + WNST - 1 is issued when block kb starts and is waited for when block kb + 1 ends: WNST - 2 blocks of MFMAs
// (2 x 4096 cycles) cover its latency.  Blocks kb and kb + 1 are both readable during block kb, so the operand reads run
// WAW K-steps ahead of the MFMAs across the block boundary; one barrier per K-block.  The columns of a chunk are
// contracted in ascending order and the chunk's partial product goes to Pp[chunk][bin]: the bits of a k-ordered fmaf chain.
// c64_wfinish_kernel: lane = i, workgroup = o: sums the chunks in order, forms Acc, inverse FFT over the bins, taps 0..15.
constexpr int WCH = 4;             // column chunks (split-K) of the weight-gradient GEMM
constexpr int WKB = 32;            // columns per K-block: geometry() pads the columns to 128 = WCH x WKB
constexpr int WNST = 4;            // ring stages of [D slab | Z slab], 32 KiB each
constexpr int WAW = 4;             // K-steps (2 columns each) the operand reads run ahead
constexpr int WSTAGE = 2 * WKB * 128 * 4, WDMA = WSTAGE / 1024 / 4;      // bytes per stage, LDS-DMA instructions per wave and stage

template <int N>
__device__ __forceinline__ void wait_dma() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

__global__ __launch_bounds__(256) void c64_bin_wgemm_kernel(const float* __restrict__ D, const float* __restrict__ Z,
                                                            float* __restrict__ Pp, int ncolp, int cpc) {
  __shared__ __attribute__((aligned(1024))) unsigned char smem[WNST * WSTAGE];
  const int bin = blockIdx.y, chunk = blockIdx.x, lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = lane & 31, kk = lane >> 5;
  const int nkb = cpc / WKB;                   // cpc: a multiple of WKB columns, all inside the zero-padded buffers
  f32x16 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  // ---- staging: the stage image is [D rows of the block | Z rows of the block], 1 KiB pieces; wave w copies pieces
  // 8 w .. 8 w + 7 (waves 0, 1 the D slab, waves 2, 3 the Z slab), lane l the 16 bytes at 16 l of a piece
  const int64_t slab0 = ((int64_t)bin * ncolp + (int64_t)chunk * cpc) * 128;
  const float* src0 = (wave < 2 ? D : Z) + slab0 + (wave & 1) * (WDMA * 256);
  const unsigned lds0 = (unsigned)(uintptr_t)(lds_ptr_t)smem;
  const unsigned voff = lane * 16;
  // (the LDS-DMA is issued from inline asm and counted by hand: see gemm_sp.hip; m0 is written in the statement that uses it)
  auto issue = [&](int kb) {
    const float* sb = src0 + (int64_t)kb * (WKB * 128);
    const unsigned dst = lds0 + (kb % WNST) * WSTAGE + wave * (WDMA * 1024);
#pragma unroll
    for (int i = 0; i < WDMA; ++i)
      asm volatile("s_mov_b32 m0, %2\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sb + i * 256), "s"(dst + i * 1024)
                   : "memory");
  };
  // ---- operands of K-step s (columns 2 s + kk) of a stage: A = D[col][32 wave + n], B_j = Z[col][32 j + n]
  const float* lds = reinterpret_cast<const float*>(smem);
  const int aoff = kk * 128 + 32 * wave + n, boff = WKB * 128 + kk * 128 + n;
  float ra[WAW], rb[WAW][4];
  auto read_step = [&](int slot, const float* stg, int s) {
    ra[slot] = stg[aoff + s * 256];
#pragma unroll
    for (int j = 0; j < 4; ++j) rb[slot][j] = stg[boff + s * 256 + 32 * j];
  };
#pragma unroll
  for (int kb = 0; kb < WNST - 1; ++kb)
    if (kb < nkb) issue(kb);
  // block 0 landed (a wave's DMA completes in order: all but the WDMA instructions of each younger block)
  if (nkb >= 3) wait_dma<2 * WDMA>();
  else if (nkb == 2) wait_dma<WDMA>();
  else wait_dma<0>();
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
#pragma unroll
  for (int s = 0; s < WAW; ++s) read_step(s, lds, s);
  constexpr int NS = WKB / 2;                  // K-steps per block
  for (int kb = 0; kb < nkb; ++kb) {
    // block kb + 1 landed: this wave's part by count, the other waves' by the barrier - which also says that every wave
    // has left block kb - 1, whose stage takes block kb + WNST - 1
    if (kb + 2 < nkb) wait_dma<WDMA>();
    else wait_dma<0>();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");             // (no operand read of block kb + 1 above the barrier)
    if (kb + WNST - 1 < nkb) issue(kb + WNST - 1);
    const float* cur = lds + (kb % WNST) * (WSTAGE / 4);
    const float* nx = lds + ((kb + 1) % WNST) * (WSTAGE / 4);      // (past the last block: reads of a stale stage, never used)
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int slot = s % WAW;
      const float a = ra[slot];
      const float b0 = rb[slot][0], b1 = rb[slot][1], b2 = rb[slot][2], b3 = rb[slot][3];
      if (s + WAW < NS) read_step(slot, cur, s + WAW);
      else read_step(slot, nx, s + WAW - NS);
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc[1], 0, 0, 0);
      acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b2, acc[2], 0, 0, 0);
      acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b3, acc[3], 0, 0, 0);
    }
    // the order asked of the scheduler: the reads stay WAW K-steps ahead, spread between the MFMAs (hipcc pairs them: 5
    // ds_read2 per two K-steps); left alone it sinks every read to just in front of the MFMA that uses it
#pragma unroll
    for (int i = 0; i < NS / 2; ++i) {
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
    }
  }
  // D-layout: lane holds column b = 32 j + n, rows a = 32 wave + (r & 3) + 8 (r >> 2) + 4 kk
  float* out = Pp + (((int64_t)chunk * 64 + bin) * 128 + 32 * wave) * 128 + n;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) out[(int64_t)((r & 3) + 8 * (r >> 2) + 4 * kk) * 128 + 32 * j] = acc[j][r];
}

// (bin m, output o) per workgroup, lane = i: the chunk sums in a fixed order and the complex combination -> Acc[m][o][i]
__global__ __launch_bounds__(64) void c64_wsum_kernel(const float* __restrict__ Pp, float* __restrict__ Acc, int nchunk) {
  const int m = blockIdx.x, o = blockIdx.y, lane = threadIdx.x;
  float prr = 0.f, pii = 0.f, pri = 0.f, pir = 0.f;
  for (int c = 0; c < nchunk; ++c) {                // fixed order: bit-reproducible
    const float* p = Pp + (((int64_t)c * 64 + m) * 128) * 128;
    prr += p[(int64_t)o * 128 + lane];
    pri += p[(int64_t)o * 128 + 64 + lane];
    pir += p[(int64_t)(64 + o) * 128 + lane];
    pii += p[(int64_t)(64 + o) * 128 + 64 + lane];
  }
  *reinterpret_cast<v2f*>(Acc + 2 * (((int64_t)m * 64 + o) * 64 + lane)) = (v2f){prr + pii, pri - pir};
}

// workgroup = o, lane = i: inverse FFT over the bins, real parts of lags 0 .. 15
__global__ __launch_bounds__(64) void c64_wfinish_kernel(const float* __restrict__ Acc, float* __restrict__ dW) {
  const int o = blockIdx.x, lane = threadIdx.x;
  v2f x[64];
#pragma unroll
  for (int m = 0; m < 64; ++m) x[m] = *reinterpret_cast<const v2f*>(Acc + 2 * (((int64_t)m * 64 + o) * 64 + lane));
  fft64<true>(x);
#pragma unroll
  for (int k = 0; k < KT; ++k) dW[((int64_t)o * NCH + lane) * KT + k] = x[pos64(k)].x * (1.0f / NB);
}

int pack_grid(const Geo& g) { return std::max(1, std::min(512, cdiv(g.ncolp, 4))); }

// The workspace of eav_conv64_fft_*, in this order: two filter-spectrum tables [64 bins][128][128] (forward BmF, data
// gradient BmB), three spectra buffers [64 bins][columns][128] (Zf: input of the forward - kept for the weight gradient -,
// Zb: input of the data gradient, Y: a scratch one - GEMM output / du blocks of the weight gradient), the weight gradient's
// split-K partial products Pp and their sum Acc.  floats: the end offset = the size (ws NULL: the size alone).
struct Ws { float *BmF, *BmB, *Zf, *Zb, *Y, *Pp, *Acc; int64_t floats; };
Ws carve(float* ws, const Geo& g) {
  const int64_t table = (int64_t)64 * 128 * 128, spectra = (int64_t)64 * g.ncolp * 128;
  Ws s = {};
  auto take = [&](int64_t n) { float* p = ws ? ws + s.floats : nullptr; s.floats += n; return p; };
  s.BmF = take(table), s.BmB = take(table);
  s.Zf = take(spectra), s.Zb = take(spectra), s.Y = take(spectra);
  s.Pp = take(WCH * table), s.Acc = take((int64_t)64 * 64 * 64 * 2);
  return s;
}

}  // namespace

// floats of the workspace of eav_conv64_fft_* (struct Ws)
extern "C" int64_t eav_conv64_fft_ws_floats(int B, int T) { return carve(nullptr, geometry(B, T, PADF)).floats; }

// rows of stat_part ([rows][128]: 64 sums, 64 sums of squares) eav_conv64_fft_fwd writes
extern "C" int eav_conv64_fft_nparts(int B, int T) { return pack_grid(geometry(B, T, PADF)) * 4; }

// out [B,64,T] = separableConv(in) (bwd = 0, 'same' padding 7 / 8; stat_part as eav_conv64_fwd's, may be NULL) or its data
// gradient (bwd = 1: in = d loss / d out, out = d loss / d in; bwd = 2: the same, re-using the filter spectra the forward
// call of this step prepared in ws - it prepares both tables); w [64,64,16] = separableConv.weight.
extern "C" int eav_conv64_fft_fwd(const float* in, const float* w, float* out, float* stat_part, float* ws, int B, int T,
                                  int bwd, void* stream) {
  EAV_REQUIRE(in && w && out && ws && B > 0 && T > 0, "eav_conv64_fft_fwd: bad arguments");
  EAV_REQUIRE(((uintptr_t)ws & 15) == 0, "eav_conv64_fft_fwd: the workspace must be 16-byte aligned");
  const Geo g = geometry(B, T, bwd ? PADB : PADF);
  EAV_REQUIRE(bwd >= 0 && bwd <= 2, "eav_conv64_fft_fwd: bwd must be 0, 1 or 2");
  hipStream_t st = (hipStream_t)stream;
  const Ws s = carve(ws, g);
  const bool prepared = bwd == 2;                        // 2: the forward call of this step left the table in ws
  if (bwd == 2) bwd = 1;
  float *Bm = bwd ? s.BmB : s.BmF, *Z = bwd ? s.Zb : s.Zf, *Y = s.Y;
  // forward: both tables (weights do not change between the forward and the backward of a step), as the leading
  // workgroups of the pack launch - a wave per (table, input channel)
  const int nspec = prepared ? 0 : (bwd ? NCH / 4 : 2 * NCH / 4);
  hipLaunchKernelGGL(c64_pack_fft_kernel, dim3(nspec + pack_grid(g)), dim3(256), 0, st, in, Z, g, 0, w, Bm, nspec, bwd);
  EAV_CHECK_LAUNCH("eav_conv64_fft_fwd(fft)");
  hipLaunchKernelGGL(c64_bin_gemm_kernel, dim3(64, std::min(GEMM_GW, g.ncolp / 32)), dim3(256), 0, st, Z, Bm, Y, g.ncolp);
  EAV_CHECK_LAUNCH("eav_conv64_fft_fwd(gemm)");
  hipLaunchKernelGGL(c64_ifft_unpack_kernel, dim3(pack_grid(g)), dim3(256), 0, st, Y, out, stat_part, g);
  EAV_CHECK_LAUNCH("eav_conv64_fft_fwd(ifft)");
  return EAV_OK;
}

// dW [64,64,16] = d loss / d separableConv.weight (WRITTEN, no partials to reduce) from du = d loss / d(conv output)
// [B,64,T].  The forward input's spectra must still be in `ws`: call after eav_conv64_fft_fwd(in, ..., ws, B, T, 0) of the
// same step (a data-gradient call in between does not disturb them).  Bit-reproducible.
extern "C" int eav_conv64_fft_wgrad(const float* du, float* dW, float* ws, int B, int T, void* stream) {
  EAV_REQUIRE(du && dW && ws && B > 0 && T > 0, "eav_conv64_fft_wgrad: bad arguments");
  const Geo g = geometry(B, T, PADF);
  hipStream_t st = (hipStream_t)stream;
  const Ws s = carve(ws, g);
  float *Z = s.Zf, *D = s.Y, *Pp = s.Pp, *Acc = s.Acc;
  hipLaunchKernelGGL(c64_pack_fft_kernel, dim3(pack_grid(g)), dim3(256), 0, st, du, D, g, 1, nullptr, nullptr, 0, 0);
  EAV_CHECK_LAUNCH("eav_conv64_fft_wgrad(fft)");
  static_assert(128 % (WCH * WKB) == 0, "the padded columns split into WCH chunks of whole K-blocks");
  const int cpc = g.ncolp / WCH;                            // columns per chunk: a multiple of WKB
  hipLaunchKernelGGL(c64_bin_wgemm_kernel, dim3(WCH, 64), dim3(256), 0, st, D, Z, Pp, g.ncolp, cpc);
  EAV_CHECK_LAUNCH("eav_conv64_fft_wgrad(gemm)");
  hipLaunchKernelGGL(c64_wsum_kernel, dim3(64, 64), dim3(64), 0, st, Pp, Acc, WCH);
  EAV_CHECK_LAUNCH("eav_conv64_fft_wgrad(sum)");
  hipLaunchKernelGGL(c64_wfinish_kernel, dim3(NCH), dim3(64), 0, st, Acc, dW);
  EAV_CHECK_LAUNCH("eav_conv64_fft_wgrad(finish)");
  return EAV_OK;
}

// The whole separableConv backward of a step from ONE pack launch: dx [B,64,T] = d loss / d(conv input) (what
// eav_conv64_fft_fwd(bwd = 2) gives) and dW [64,64,16] (what eav_conv64_fft_wgrad gives), bit for bit.  ws: the workspace
// the forward call of this step (eav_conv64_fft_fwd, bwd = 0) left its filter spectra and input spectra in.
//   du != NULL: du [B,64,T] = d loss / d(conv output) is read;
//   du == NULL: it is formed while loading, du = eav_bn_elu_pool_bwd_apply(dp, u, bn, m12, P = 8) with the same dropout
//               arguments (dp [B,64,T/8], u [B,64,T] = the conv output, bn = mean, invstd, scale, shift, m12 = m1, m2) -
//               that launch and the du tensor disappear.
// The weight gradient's du spectra and the data gradient's GEMM output share the workspace's third spectra buffer: the
// weight-gradient GEMM runs first.
extern "C" int eav_conv64_fft_bwd(const float* du, const float* dp, const float* u, const float* bn, const float* m12,
                                  float drop_p, uint64_t seed, const uint8_t* mask, const uint64_t* seed_dev, float* dx,
                                  float* dW, float* ws, int B, int T, void* stream) {
  EAV_REQUIRE(dx && dW && ws && B > 0 && T > 0, "eav_conv64_fft_bwd: bad arguments");
  EAV_REQUIRE(du || (dp && u && bn && m12), "eav_conv64_fft_bwd: neither du nor (dp, u, bn, m12)");
  EAV_REQUIRE(du || T >= 8, "eav_conv64_fft_bwd: T %d < the pooling window", T);
  EAV_REQUIRE(drop_p > -1.f && drop_p < 1.f, "eav_conv64_fft_bwd: dropout %f outside (-1,1)", drop_p);
  EAV_REQUIRE(((uintptr_t)ws & 15) == 0, "eav_conv64_fft_bwd: the workspace must be 16-byte aligned");
  const Geo g = geometry(B, T, PADB);
  hipStream_t st = (hipStream_t)stream;
  const Ws s = carve(ws, g);
  float *Bm = s.BmB, *Z = s.Zf, *Zb = s.Zb, *D = s.Y, *Pp = s.Pp, *Acc = s.Acc;      // D: du spectra, then the GEMM output
  const DuSrc src = {dp, u, bn, m12, drop_p, seed, mask, seed_dev};
  if (du)
    hipLaunchKernelGGL(c64_pack_bwd_kernel<false>, dim3(pack_grid(g)), dim3(256), 0, st, du, src, Zb, D, g);
  else
    hipLaunchKernelGGL(c64_pack_bwd_kernel<true>, dim3(pack_grid(g)), dim3(256), 0, st, du, src, Zb, D, g);
  EAV_CHECK_LAUNCH("eav_conv64_fft_bwd(fft)");
  const int cpc = g.ncolp / WCH;
  hipLaunchKernelGGL(c64_bin_wgemm_kernel, dim3(WCH, 64), dim3(256), 0, st, D, Z, Pp, g.ncolp, cpc);
  EAV_CHECK_LAUNCH("eav_conv64_fft_bwd(wgemm)");
  hipLaunchKernelGGL(c64_bin_gemm_kernel, dim3(64, std::min(GEMM_GW, g.ncolp / 32)), dim3(256), 0, st, Zb, Bm, D, g.ncolp);
  EAV_CHECK_LAUNCH("eav_conv64_fft_bwd(gemm)");
  hipLaunchKernelGGL(c64_ifft_unpack_kernel, dim3(pack_grid(g)), dim3(256), 0, st, D, dx, nullptr, g);
  EAV_CHECK_LAUNCH("eav_conv64_fft_bwd(ifft)");
  hipLaunchKernelGGL(c64_wsum_kernel, dim3(64, 64), dim3(64), 0, st, Pp, Acc, WCH);
  EAV_CHECK_LAUNCH("eav_conv64_fft_bwd(sum)");
  hipLaunchKernelGGL(c64_wfinish_kernel, dim3(NCH), dim3(64), 0, st, Acc, dW);
  EAV_CHECK_LAUNCH("eav_conv64_fft_bwd(finish)");
  return EAV_OK;
}
