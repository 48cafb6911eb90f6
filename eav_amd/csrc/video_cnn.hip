// The video CNN of CNN_torch/CNN_Vision.py (VideoModel: torchvision's ResNet-50 trunk + a channel-attention head) on the
// gfx950 fp32 matrix cores (v_mfma_f32_32x32x2_f32: an exact k-ordered f32 fma chain, so parity with CPU torch is limited
// by summation order only).
//
// Activations are NHWC fp32: rows [B*H*W][C].  1x1 stride-1 convs are plain GEMMs (eav_gemm_f32 / eav_gemm_f32_splitk);
// every other conv of the network (7x7/2 on 3 channels, 3x3/1, 3x3/2, 1x1/2) and both of its gradients are
//
//   igemm_kernel<MODE>   implicit GEMM, workgroup tile 64 rows x 64 columns (2 x 2 waves of 32 x 32), contraction in
//       chunks of 32 staged in LDS.  MODE_FWD: rows = output pixels, columns = output channels, k = (tap, input channel),
//       B = the weight re-laid as wf [Cout][kh][kw][Cin].  MODE_DGRAD: rows = input pixels, columns = input channels,
//       k = (tap, output channel) gathered from the output gradient where (ih + pad - kh) is a multiple of the stride,
//       B = wd [Cin][kh][kw][Cout]; optional `add` operand (the residual branch's gradient) in the epilogue.
//   wgrad_kernel         dW[co][ci][kh][kw] = sum over output pixels of dout[r][co] x in[r's window (kh, kw)][ci], split
//       over 32-pixel chunks q = part, part + nparts, ... into partials summed in fixed order by eav_reduce_partials.
//
// BatchNorm (train and eval) is the existing eav_bn_finalize / eav_bn_bwd_finalize / eav_bn_rows_bwd around three passes
// of this file: per-channel sum / sum-of-squares partials, the apply (scale / shift, optional residual with its own
// scale / shift, ReLU) and the backward sums (ReLU' gate from the stored output, sums of g and g * xhat).  MaxPool 3x3/2
// stores a uint8 window argmax and its backward is a gather.  The head pools over the final map.
//
// No float atomics: every output element is written by exactly one lane, every sum has a fixed order (bit-reproducible).
#include "eav_common.h"
#include "../../include/eav_hip.h"

namespace {

constexpr int TM = 64, TN = 64, KC = 32;
constexpr int LDK = KC + 1;          // odd LDS row stride: the 32 lanes of a half-wave read 32 distinct banks

enum { MODE_FWD = 0, MODE_DGRAD = 1 };

struct ConvGeom {
  int B, H, W, C;          // input image [B][H][W][C] (NHWC, or the strides below)
  int OH, OW, N;           // output map and output channels
  int KH, KW, S, P;
  int64_t sB, sH, sW, sC;  // element strides of the input image (FWD / WGRAD)
};

struct IgemmArgs {
  ConvGeom g;
  const float* x;    // FWD: input image; DGRAD: output gradient [B][OH][OW][N]
  const float* wt;   // re-laid weight: FWD wf [N][KH*KW*C]; DGRAD wd [C][KH*KW*N]
  const float* add;  // DGRAD: optional [B*H*W][C] added in the epilogue
  float* out;        // FWD [B*OH*OW][N]; DGRAD [B*H*W][C]
};

// A[m][k] for k = k0 .. k0 + 7 into v[8].  FWD: m = (b, oh, ow), k = (kh, kw, c) over the input image.
// DGRAD: m = (b, ih, iw), k = (kh, kw, n) over the output gradient.
template <int MODE>
__device__ __forceinline__ void load_a8(const IgemmArgs& a, int b, int y, int x, bool mok, int k0, int K, float v[8]) {
  const ConvGeom& g = a.g;
  const int CC = MODE == MODE_FWD ? g.C : g.N;   // contraction channels per tap
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = 0.f;
  if (!mok) return;
  const bool vec = MODE == MODE_DGRAD ? (CC % 8 == 0) : (CC % 8 == 0 && g.sC == 1);
  if (vec) {
    if (k0 >= K) return;
    const int tap = k0 / CC, c = k0 - tap * CC, kh = tap / g.KW, kw = tap - kh * g.KW;
    const float* src = nullptr;
    if (MODE == MODE_FWD) {
      const int ih = y * g.S - g.P + kh, iw = x * g.S - g.P + kw;
      if (ih >= 0 && ih < g.H && iw >= 0 && iw < g.W) src = a.x + b * g.sB + ih * g.sH + iw * g.sW + c;
    } else {
      const int th = y + g.P - kh, tw = x + g.P - kw;
      if (th >= 0 && tw >= 0 && th % g.S == 0 && tw % g.S == 0) {
        const int oh = th / g.S, ow = tw / g.S;
        if (oh < g.OH && ow < g.OW) src = a.x + (((int64_t)b * g.OH + oh) * g.OW + ow) * g.N + c;
      }
    }
    if (src) {
      const float4 p0 = *reinterpret_cast<const float4*>(src), p1 = *reinterpret_cast<const float4*>(src + 4);
      v[0] = p0.x; v[1] = p0.y; v[2] = p0.z; v[3] = p0.w; v[4] = p1.x; v[5] = p1.y; v[6] = p1.z; v[7] = p1.w;
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = k0 + j;
    if (k >= K) break;
    const int tap = k / CC, c = k - tap * CC, kh = tap / g.KW, kw = tap - kh * g.KW;
    if (MODE == MODE_FWD) {
      const int ih = y * g.S - g.P + kh, iw = x * g.S - g.P + kw;
      if (ih >= 0 && ih < g.H && iw >= 0 && iw < g.W) v[j] = a.x[b * g.sB + ih * g.sH + iw * g.sW + c * g.sC];
    } else {
      const int th = y + g.P - kh, tw = x + g.P - kw;
      if (th >= 0 && tw >= 0 && th % g.S == 0 && tw % g.S == 0) {
        const int oh = th / g.S, ow = tw / g.S;
        if (oh < g.OH && ow < g.OW) v[j] = a.x[(((int64_t)b * g.OH + oh) * g.OW + ow) * g.N + c];
      }
    }
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void igemm_kernel(IgemmArgs a) {
  __shared__ float As[TM][LDK];
  __shared__ float Bs[TN][LDK];
  const ConvGeom& g = a.g;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5, wm = wave >> 1, wn = wave & 1;
  // rows: FWD output pixels (OH x OW maps), DGRAD input pixels (H x W maps); columns: FWD N, DGRAD C
  const int RH = MODE == MODE_FWD ? g.OH : g.H, RW = MODE == MODE_FWD ? g.OW : g.W;
  const int M = g.B * RH * RW, NC = MODE == MODE_FWD ? g.N : g.C;
  const int K = g.KH * g.KW * (MODE == MODE_FWD ? g.C : g.N);
  const int m0 = blockIdx.x * TM, n0 = blockIdx.y * TN;
  // this thread's staging slot: row / column (t >> 2) of the tile, contraction offsets 8 (t & 3) .. + 7
  const int sr = threadIdx.x >> 2, sk = (threadIdx.x & 3) * 8;
  const int m = m0 + sr;
  const bool mok = m < M;
  const int mm = mok ? m : 0;
  const int pb = mm / (RH * RW), prem = mm - pb * RH * RW, py = prem / RW, px = prem - py * RW;
  const int nb = n0 + sr;
  const bool nok = nb < NC;
  const bool bvec = (K % 8) == 0;
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;

  for (int k0 = 0; k0 < K; k0 += KC) {
    float va[8], vb[8];
    load_a8<MODE>(a, pb, py, px, mok, k0 + sk, K, va);
#pragma unroll
    for (int j = 0; j < 8; ++j) vb[j] = 0.f;
    if (nok) {
      const float* src = a.wt + (int64_t)nb * K + k0 + sk;
      if (bvec) {
        if (k0 + sk < K) {
          const float4 p0 = *reinterpret_cast<const float4*>(src), p1 = *reinterpret_cast<const float4*>(src + 4);
          vb[0] = p0.x; vb[1] = p0.y; vb[2] = p0.z; vb[3] = p0.w; vb[4] = p1.x; vb[5] = p1.y; vb[6] = p1.z; vb[7] = p1.w;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (k0 + sk + j < K) vb[j] = src[j];
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      As[sr][sk + j] = va[j];
      Bs[sr][sk + j] = vb[j];
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < KC / 2; ++s) {
      const int k = 2 * s + h;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[wm * 32 + r][k], Bs[wn * 32 + r][k], acc, 0, 0, 0);
    }
  }

  // D: column (lane & 31), row (i & 3) + 8 (i >> 2) + 4 h
  const int n = n0 + wn * 32 + r;
  if (n < NC) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int mo = m0 + wm * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
      if (mo < M) {
        const int64_t o = (int64_t)mo * NC + n;
        a.out[o] = (MODE == MODE_DGRAD && a.add) ? acc[i] + a.add[o] : acc[i];
      }
    }
  }
}

// dW partials.  Tile: 64 output channels (rows) x 64 weight columns n = (kh, kw, ci); contraction over output pixels in
// chunks of 32; chunk q of the M = B*OH*OW pixels goes to part q % nparts.
struct WgradArgs {
  ConvGeom g;
  const float* dout;   // [B*OH*OW][N]
  const float* x;      // input image (strides in g)
  float* part;         // [nparts][N * C * KH * KW], torchvision layout [co][ci][kh][kw]
  int nparts;
};

__global__ __launch_bounds__(256) void wgrad_kernel(WgradArgs a) {
  __shared__ float Ds[TM][LDK];   // [co][pixel]
  __shared__ float Xs[TN][LDK];   // [n][pixel]
  const ConvGeom& g = a.g;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5, wm = wave >> 1, wn = wave & 1;
  const int M = g.B * g.OH * g.OW, KK = g.KH * g.KW, NW = KK * g.C;
  const int co0 = blockIdx.y * TM, n0 = blockIdx.x * TN, p = blockIdx.z;
  const int nq = (M + KC - 1) / KC;
  // staging slot: pixel j = t >> 3 of the chunk, 8 consecutive columns from 8 (t & 7)
  const int sj = threadIdx.x >> 3, sc = (threadIdx.x & 7) * 8;
  const bool dvec = g.N % 8 == 0, xvec = g.C % 8 == 0 && g.sC == 1;
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;

  for (int q = p; q < nq; q += a.nparts) {
    const int pix = q * KC + sj;
    float vd[8], vx[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { vd[j] = 0.f; vx[j] = 0.f; }
    if (pix < M) {
      const float* ds = a.dout + (int64_t)pix * g.N + co0 + sc;
      if (dvec) {
        if (co0 + sc < g.N) {
          const float4 p0 = *reinterpret_cast<const float4*>(ds), p1 = *reinterpret_cast<const float4*>(ds + 4);
          vd[0] = p0.x; vd[1] = p0.y; vd[2] = p0.z; vd[3] = p0.w; vd[4] = p1.x; vd[5] = p1.y; vd[6] = p1.z; vd[7] = p1.w;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (co0 + sc + j < g.N) vd[j] = ds[j];
      }
      const int b = pix / (g.OH * g.OW), rem = pix - b * g.OH * g.OW, oh = rem / g.OW, ow = rem - oh * g.OW;
      const int nn = n0 + sc;
      if (xvec) {
        if (nn < NW) {
          const int tap = nn / g.C, c = nn - tap * g.C, kh = tap / g.KW, kw = tap - kh * g.KW;
          const int ih = oh * g.S - g.P + kh, iw = ow * g.S - g.P + kw;
          if (ih >= 0 && ih < g.H && iw >= 0 && iw < g.W) {
            const float* xs = a.x + b * g.sB + ih * g.sH + iw * g.sW + c;
            const float4 p0 = *reinterpret_cast<const float4*>(xs), p1 = *reinterpret_cast<const float4*>(xs + 4);
            vx[0] = p0.x; vx[1] = p0.y; vx[2] = p0.z; vx[3] = p0.w; vx[4] = p1.x; vx[5] = p1.y; vx[6] = p1.z; vx[7] = p1.w;
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int n = nn + j;
          if (n < NW) {
            const int tap = n / g.C, c = n - tap * g.C, kh = tap / g.KW, kw = tap - kh * g.KW;
            const int ih = oh * g.S - g.P + kh, iw = ow * g.S - g.P + kw;
            if (ih >= 0 && ih < g.H && iw >= 0 && iw < g.W) vx[j] = a.x[b * g.sB + ih * g.sH + iw * g.sW + c * g.sC];
          }
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      Ds[sc + j][sj] = vd[j];
      Xs[sc + j][sj] = vx[j];
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < KC / 2; ++s) {
      const int k = 2 * s + h;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ds[wm * 32 + r][k], Xs[wn * 32 + r][k], acc, 0, 0, 0);
    }
  }

  const int n = n0 + wn * 32 + r;
  if (n < NW) {
    const int tap = n / g.C, c = n - tap * g.C;
    float* dst = a.part + (int64_t)p * g.N * NW + (int64_t)c * KK + tap;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int co = co0 + wm * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
      if (co < g.N) dst[(int64_t)co * NW] = acc[i];
    }
  }
}

// w [Co][Ci][KK] -> wf [Co][KK][Ci] (forward B operand) and wd [Ci][KK][Co] (data-gradient B operand); one thread per
// weight element, either output may be null.
__global__ __launch_bounds__(256) void relayout_kernel(const float* __restrict__ w, float* __restrict__ wf,
                                                       float* __restrict__ wd, int Co, int Ci, int KK) {
  const int64_t n = (int64_t)Co * Ci * KK;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int tap = (int)(i % KK);
    const int64_t t = i / KK;
    const int ci = (int)(t % Ci), co = (int)(t / Ci);
    const float v = w[i];
    if (wf) wf[((int64_t)co * KK + tap) * Ci + ci] = v;
    if (wd) wd[((int64_t)ci * KK + tap) * Co + co] = v;
  }
}

// ---------------------------------------------------------------------------------------------------- BatchNorm
// Per-channel partials over row chunks of RCH rows: block = 64 channels x 4 row lanes; each lane sums its rows in fp64 in
// row order, the four lanes are added in lane order (fixed order).  Chunk p writes TWO partial rows, 2p = float(sum) and
// 2p + 1 = float(sum - float(sum)): the finalisers add their fp32 partial rows in fp64, so the pair carries the chunk's
// fp64 sum to ~48 bits.  (One fp32 row per chunk rounds sum x^2 to 2^-24 of itself, and var = E[x^2] - mean^2 then loses
// 2^-24 mean^2 / var - a relative 1e-3 on a deep-layer channel whose 16 batch values sit far from zero.)
constexpr int RCH = 256, BCH = 64;

__device__ __forceinline__ void bn_part_store(double s, double q, float* part, int p, int C, int c, bool cok) {
  __shared__ double sh[2][4][BCH];
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  sh[0][rl][cl] = s;
  sh[1][rl][cl] = q;
  __syncthreads();
  if (rl == 0 && cok) {
    const double ts = ((sh[0][0][cl] + sh[0][1][cl]) + sh[0][2][cl]) + sh[0][3][cl];
    const double tq = ((sh[1][0][cl] + sh[1][1][cl]) + sh[1][2][cl]) + sh[1][3][cl];
    const float hs = (float)ts, hq = (float)tq;
    float* row = part + (int64_t)(2 * p) * 2 * C;
    row[c] = hs;
    row[C + c] = hq;
    row[2 * C + c] = (float)(ts - (double)hs);
    row[3 * C + c] = (float)(tq - (double)hq);
  }
}

__global__ __launch_bounds__(256) void bn_stats_kernel(const float* __restrict__ x, float* __restrict__ part, int64_t M,
                                                       int C) {
  const int c = blockIdx.x * BCH + (threadIdx.x & 63), rl = threadIdx.x >> 6, p = blockIdx.y;
  const bool cok = c < C;
  double s = 0.0, q = 0.0;
  if (cok) {
    const int64_t r1 = min((int64_t)(p + 1) * RCH, M);
    for (int64_t row = (int64_t)p * RCH + rl; row < r1; row += 4) {
      const double v = x[row * C + c];
      s += v;
      q += v * v;
    }
  }
  bn_part_store(s, q, part, p, C, c, cok);
}

// g = dy gated by ReLU' of the stored output y (zero where y <= 0: threshold_backward, a NaN output passes); part: sum g,
// sum g * xhat with xhat = (x - mean) * invstd from bn = [mean | invstd | ...].
__global__ __launch_bounds__(256) void bn_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                     const float* __restrict__ x, const float* __restrict__ bn,
                                                     float* __restrict__ g_out, float* __restrict__ part, int64_t M,
                                                     int C) {
  const int c = blockIdx.x * BCH + (threadIdx.x & 63), rl = threadIdx.x >> 6, p = blockIdx.y;
  const bool cok = c < C;
  double s = 0.0, q = 0.0;
  if (cok) {
    const float mean = bn[c], invstd = bn[C + c];
    const int64_t r1 = min((int64_t)(p + 1) * RCH, M);
    for (int64_t row = (int64_t)p * RCH + rl; row < r1; row += 4) {
      const int64_t o = row * C + c;
      float gv = dy[o];
      if (y && y[o] <= 0.f) gv = 0.f;
      if (g_out) g_out[o] = gv;
      const float xh = (x[o] - mean) * invstd;
      s += (double)gv;
      q += (double)(gv * xh);
    }
  }
  bn_part_store(s, q, part, p, C, c, cok);
}

// out = [ReLU](x * scale + shift [+ (res * rscale + rshift | res)])
// (x, res and out carry no __restrict__: out may alias x or res - every element is read and written by one lane)
__global__ __launch_bounds__(256) void bn_apply_kernel(const float* x, const float* __restrict__ scale,
                                                       const float* __restrict__ shift, const float* res,
                                                       const float* __restrict__ rscale, const float* __restrict__ rshift,
                                                       float* out, int64_t n, int C, int relu) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C);
    float v = x[i] * scale[c] + shift[c];
    if (res) v += rscale ? res[i] * rscale[c] + rshift[c] : res[i];
    if (relu) v = v < 0.f ? 0.f : v;
    out[i] = v;
  }
}

// ---------------------------------------------------------------------------------------------------- MaxPool
// torch's CPU max_pool2d: the window is scanned in (kh, kw) order over its valid positions, `v > max || isnan(v)` takes
// the new value - ties keep the first index, a NaN propagates (the last NaN's index).  idx = kh * K + kw.
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                          uint8_t* __restrict__ idx, int B, int H, int W, int C, int OH,
                                                          int OW, int K, int S, int P) {
  const int64_t n = (int64_t)B * OH * OW * C;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C);
    int64_t t = i / C;
    const int ow = (int)(t % OW); t /= OW;
    const int oh = (int)(t % OH);
    const int b = (int)(t / OH);
    float m = 0.f;
    int mi = -1;
    for (int kh = 0; kh < K; ++kh) {
      const int ih = oh * S - P + kh;
      if (ih < 0 || ih >= H) continue;
      for (int kw = 0; kw < K; ++kw) {
        const int iw = ow * S - P + kw;
        if (iw < 0 || iw >= W) continue;
        const float v = x[(((int64_t)b * H + ih) * W + iw) * C + c];
        if (mi < 0 || v > m || v != v) { m = v; mi = kh * K + kw; }
      }
    }
    out[i] = m;
    idx[i] = (uint8_t)(mi < 0 ? 0 : mi);
  }
}

// dx[b][ih][iw][c] = sum over the windows (oh, ow) that contain (ih, iw), in ascending (oh, ow) order, of dout where the
// window's argmax is (ih, iw) - the order of torch's CPU scatter, as a gather (no atomics).
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* __restrict__ dout, const uint8_t* __restrict__ idx,
                                                          float* __restrict__ dx, int B, int H, int W, int C, int OH,
                                                          int OW, int K, int S, int P) {
  const int64_t n = (int64_t)B * H * W * C;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C);
    int64_t t = i / C;
    const int iw = (int)(t % W); t /= W;
    const int ih = (int)(t % H);
    const int b = (int)(t / H);
    // window oh contains ih when oh * S - P <= ih <= oh * S - P + K - 1
    const int lh = ih + P - K + 1, lw = iw + P - K + 1;
    const int oh0 = lh > 0 ? (lh + S - 1) / S : 0, ow0 = lw > 0 ? (lw + S - 1) / S : 0;
    float s = 0.f;
    for (int oh = oh0; oh < OH && oh * S - P <= ih; ++oh) {
      const int kh = ih - (oh * S - P);
      for (int ow = ow0; ow < OW && ow * S - P <= iw; ++ow) {
        const int kw = iw - (ow * S - P);
        const int64_t o = (((int64_t)b * OH + oh) * OW + ow) * C + c;
        if (idx[o] == kh * K + kw) s += dout[o];
      }
    }
    dx[i] = s;
  }
}

// ---------------------------------------------------------------------------------------------------- head
// y [B][HW][C]: pooled[b][c] = mean over hw (sum in hw order, then / HW), pooled[B + b][c] = max with argmax (the
// max-pool rule above), one thread per (b, c).
__global__ __launch_bounds__(256) void head_pool_kernel(const float* __restrict__ y, float* __restrict__ pooled,
                                                        uint8_t* __restrict__ idx, int B, int HW, int C) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * C) return;
  const int b = i / C, c = i - b * C;
  const float* src = y + (int64_t)b * HW * C + c;
  float s = 0.f, m = 0.f;
  int mi = 0;
  for (int k = 0; k < HW; ++k) {
    const float v = src[(int64_t)k * C];
    s += v;
    if (k == 0 || v > m || v != v) { m = v; mi = k; }
  }
  pooled[i] = s / (float)HW;
  pooled[(int64_t)B * C + i] = m;
  idx[i] = (uint8_t)mi;
}

// attn = A[b] + A[B + b] (the two fc2 outputs), z[b][c] = mean over hw of y * attn
__global__ __launch_bounds__(256) void head_scale_pool_kernel(const float* __restrict__ y, const float* __restrict__ A,
                                                              float* __restrict__ attn, float* __restrict__ z, int B,
                                                              int HW, int C) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * C) return;
  const int b = i / C;
  const float at = A[i] + A[(int64_t)B * C + i];
  const float* src = y + (int64_t)b * HW * C + (i - b * C);
  float s = 0.f;
  for (int k = 0; k < HW; ++k) s += src[(int64_t)k * C] * at;
  attn[i] = at;
  z[i] = s / (float)HW;
}

// d attn[b][c] = sum over hw of (dz / HW) * y, written to both halves of dA [2B][C] (the avg and max rows of the fc chain)
__global__ __launch_bounds__(256) void head_attn_bwd_kernel(const float* __restrict__ y, const float* __restrict__ dz,
                                                            float* __restrict__ dA, int B, int HW, int C) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * C) return;
  const int b = i / C;
  const float gz = dz[i] / (float)HW;
  const float* src = y + (int64_t)b * HW * C + (i - b * C);
  float s = 0.f;
  for (int k = 0; k < HW; ++k) s += gz * src[(int64_t)k * C];
  dA[i] = s;
  dA[(int64_t)B * C + i] = s;
}

// dy[b][hw][c] = (dz / HW) * attn + dP[b][c] / HW + (hw == argmax ? dP[B + b][c] : 0)
__global__ __launch_bounds__(256) void head_feat_bwd_kernel(const float* __restrict__ dz, const float* __restrict__ attn,
                                                            const float* __restrict__ dP, const uint8_t* __restrict__ idx,
                                                            float* __restrict__ dy, int B, int HW, int C) {
  const int64_t n = (int64_t)B * HW * C;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C);
    const int64_t t = i / C;
    const int k = (int)(t % HW), b = (int)(t / HW);
    const int bc = b * C + c;
    float v = (dz[bc] / (float)HW) * attn[bc] + dP[bc] / (float)HW;
    if (idx[bc] == k) v += dP[(int64_t)B * C + bc];
    dy[i] = v;
  }
}

__global__ void counters_inc_kernel(int64_t* c, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) c[i] += 1;
}

inline int ew_blocks(int64_t n) {
  const int64_t b = (n + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 16384 ? 16384 : b));
}

constexpr int MAXCH = 4096, MAXHW = 4096, MAXK = 15;

int geom_ok(const char* who, int B, int C, int H, int W, int N, int KH, int KW, int S, int P, int OH, int OW) {
  if (!(B > 0 && C > 0 && C <= MAXCH && N > 0 && N <= MAXCH && H > 0 && H <= MAXHW && W > 0 && W <= MAXHW &&
        KH > 0 && KH <= MAXK && KW > 0 && KW <= MAXK && S > 0 && S <= 4 && P >= 0 && P < KH && P < KW))
    return eav_set_error(EAV_EINVAL, "%s: bad geometry (B %d, C %d, H %d, W %d, N %d, kernel %dx%d, stride %d, pad %d)",
                         who, B, C, H, W, N, KH, KW, S, P);
  const int oh = (H + 2 * P - KH) / S + 1, ow = (W + 2 * P - KW) / S + 1;
  if (H + 2 * P < KH || W + 2 * P < KW || OH != oh || OW != ow)
    return eav_set_error(EAV_EINVAL, "%s: output map %dx%d, the geometry gives %dx%d", who, OH, OW, oh, ow);
  if ((int64_t)B * H * W * C >= (1LL << 31) || (int64_t)B * OH * OW * N >= (1LL << 31) ||
      (int64_t)B * H * W >= (1LL << 31) / 2)
    return eav_set_error(EAV_EINVAL, "%s: tensors of 2^31 elements or more", who);
  return EAV_OK;
}

ConvGeom make_geom(int B, int C, int H, int W, int N, int KH, int KW, int S, int P, int OH, int OW, int nchw) {
  ConvGeom g{B, H, W, C, OH, OW, N, KH, KW, S, P, 0, 0, 0, 0};
  if (nchw) { g.sC = (int64_t)H * W; g.sW = 1; g.sH = W; g.sB = (int64_t)C * H * W; }
  else { g.sC = 1; g.sW = C; g.sH = (int64_t)W * C; g.sB = (int64_t)H * W * C; }
  return g;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int eav_video_conv_relayout(const float* w, float* wf, float* wd, int Co, int Ci, int KK, void* stream) {
  EAV_REQUIRE(w && (wf || wd), "eav_video_conv_relayout: null tensor");
  EAV_REQUIRE(Co > 0 && Co <= MAXCH && Ci > 0 && Ci <= MAXCH && KK > 0 && KK <= MAXK * MAXK,
              "eav_video_conv_relayout: bad sizes (Co %d, Ci %d, KK %d)", Co, Ci, KK);
  hipLaunchKernelGGL(relayout_kernel, dim3(ew_blocks((int64_t)Co * Ci * KK)), dim3(256), 0, (hipStream_t)stream, w, wf,
                     wd, Co, Ci, KK);
  EAV_CHECK_LAUNCH("eav_video_conv_relayout");
  return EAV_OK;
}

extern "C" int eav_video_conv_fwd(const float* x, const float* wf, float* out, int B, int C, int H, int W, int N, int KH,
                                  int KW, int S, int P, int OH, int OW, int nchw, void* stream) {
  EAV_REQUIRE(x && wf && out, "eav_video_conv_fwd: null tensor");
  if (int rc = geom_ok("eav_video_conv_fwd", B, C, H, W, N, KH, KW, S, P, OH, OW)) return rc;
  EAV_REQUIRE(nchw == 0 || nchw == 1, "eav_video_conv_fwd: nchw %d", nchw);
  // 16-byte alignment only where the kernel loads float4: an NHWC input with C % 8 == 0, a weight row of K % 8 == 0
  EAV_REQUIRE((nchw || C % 8 || aligned16(x)) && ((KH * KW * C) % 8 || aligned16(wf)),
              "eav_video_conv_fwd: operands must be 16-byte aligned");
  IgemmArgs a{make_geom(B, C, H, W, N, KH, KW, S, P, OH, OW, nchw), x, wf, nullptr, out};
  hipLaunchKernelGGL(igemm_kernel<MODE_FWD>, dim3(cdiv(B * OH * OW, TM), cdiv(N, TN)), dim3(256), 0,
                     (hipStream_t)stream, a);
  EAV_CHECK_LAUNCH("eav_video_conv_fwd");
  return EAV_OK;
}

extern "C" int eav_video_conv_dgrad(const float* dout, const float* wd, const float* add, float* din, int B, int C,
                                    int H, int W, int N, int KH, int KW, int S, int P, int OH, int OW, void* stream) {
  EAV_REQUIRE(dout && wd && din, "eav_video_conv_dgrad: null tensor");
  if (int rc = geom_ok("eav_video_conv_dgrad", B, C, H, W, N, KH, KW, S, P, OH, OW)) return rc;
  EAV_REQUIRE((N % 8 || aligned16(dout)) && ((KH * KW * N) % 8 || aligned16(wd)),
              "eav_video_conv_dgrad: operands must be 16-byte aligned");
  IgemmArgs a{make_geom(B, C, H, W, N, KH, KW, S, P, OH, OW, 0), dout, wd, add, din};
  hipLaunchKernelGGL(igemm_kernel<MODE_DGRAD>, dim3(cdiv(B * H * W, TM), cdiv(C, TN)), dim3(256), 0,
                     (hipStream_t)stream, a);
  EAV_CHECK_LAUNCH("eav_video_conv_dgrad");
  return EAV_OK;
}

extern "C" int eav_video_wgrad_nparts(int N, int C, int KK, int64_t M) {
  if (N <= 0 || C <= 0 || KK <= 0 || M <= 0) return 0;
  const int tiles = cdiv(N, TM) * cdiv(KK * C, TN);
  const int64_t nq = cdiv64(M, KC);
  int np = cdiv(1024, tiles);            // ~4 workgroups per CU over the 256 CUs
  return np < 1 ? 1 : (np > nq ? (int)nq : np);
}

extern "C" int eav_video_conv_wgrad(const float* dout, const float* x, float* part, int B, int C, int H, int W, int N,
                                    int KH, int KW, int S, int P, int OH, int OW, int nchw, int nparts, void* stream) {
  EAV_REQUIRE(dout && x && part, "eav_video_conv_wgrad: null tensor");
  if (int rc = geom_ok("eav_video_conv_wgrad", B, C, H, W, N, KH, KW, S, P, OH, OW)) return rc;
  EAV_REQUIRE(nchw == 0 || nchw == 1, "eav_video_conv_wgrad: nchw %d", nchw);
  EAV_REQUIRE((N % 8 || aligned16(dout)) && (nchw || C % 8 || aligned16(x)),
              "eav_video_conv_wgrad: operands must be 16-byte aligned");
  const int np = eav_video_wgrad_nparts(N, C, KH * KW, (int64_t)B * OH * OW);
  EAV_REQUIRE(nparts == np, "eav_video_conv_wgrad: nparts %d, eav_video_wgrad_nparts gives %d", nparts, np);
  WgradArgs a{make_geom(B, C, H, W, N, KH, KW, S, P, OH, OW, nchw), dout, x, part, nparts};
  hipLaunchKernelGGL(wgrad_kernel, dim3(cdiv(KH * KW * C, TN), cdiv(N, TM), nparts), dim3(256), 0, (hipStream_t)stream,
                     a);
  EAV_CHECK_LAUNCH("eav_video_conv_wgrad");
  return EAV_OK;
}

extern "C" int eav_video_bn_nparts(int64_t M) { return M > 0 ? 2 * (int)cdiv64(M, RCH) : 0; }

extern "C" int eav_video_bn_stats(const float* x, float* part, int64_t M, int C, void* stream) {
  EAV_REQUIRE(x && part, "eav_video_bn_stats: null tensor");
  EAV_REQUIRE(M > 0 && C > 0 && C <= MAXCH && cdiv64(M, RCH) <= 65535 && M * C < (1LL << 31),
              "eav_video_bn_stats: bad sizes (M %lld, C %d)", (long long)M, C);
  hipLaunchKernelGGL(bn_stats_kernel, dim3(cdiv(C, BCH), (int)cdiv64(M, RCH)), dim3(256), 0, (hipStream_t)stream, x,
                     part, M, C);
  EAV_CHECK_LAUNCH("eav_video_bn_stats");
  return EAV_OK;
}

extern "C" int eav_video_bn_apply(const float* x, const float* scale, const float* shift, const float* res,
                                  const float* rscale, const float* rshift, float* out, int64_t M, int C, int relu,
                                  void* stream) {
  EAV_REQUIRE(x && scale && shift && out, "eav_video_bn_apply: null tensor");
  EAV_REQUIRE(M > 0 && C > 0 && C <= MAXCH && M * C < (1LL << 31), "eav_video_bn_apply: bad sizes (M %lld, C %d)",
              (long long)M, C);
  EAV_REQUIRE(!rscale == !rshift && (!rscale || res), "eav_video_bn_apply: residual scale and shift go together");
  EAV_REQUIRE(relu == 0 || relu == 1, "eav_video_bn_apply: relu %d", relu);
  hipLaunchKernelGGL(bn_apply_kernel, dim3(ew_blocks(M * C)), dim3(256), 0, (hipStream_t)stream, x, scale, shift, res,
                     rscale, rshift, out, M * C, C, relu);
  EAV_CHECK_LAUNCH("eav_video_bn_apply");
  return EAV_OK;
}

extern "C" int eav_video_bn_bwd(const float* dy, const float* y, const float* x, const float* bn, float* g, float* part,
                                int64_t M, int C, void* stream) {
  EAV_REQUIRE(dy && x && bn && part, "eav_video_bn_bwd: null tensor");
  EAV_REQUIRE(!y || g, "eav_video_bn_bwd: the gated gradient needs an output buffer");
  EAV_REQUIRE(M > 0 && C > 0 && C <= MAXCH && cdiv64(M, RCH) <= 65535 && M * C < (1LL << 31),
              "eav_video_bn_bwd: bad sizes (M %lld, C %d)", (long long)M, C);
  hipLaunchKernelGGL(bn_bwd_kernel, dim3(cdiv(C, BCH), (int)cdiv64(M, RCH)), dim3(256), 0, (hipStream_t)stream, dy, y,
                     x, bn, g, part, M, C);
  EAV_CHECK_LAUNCH("eav_video_bn_bwd");
  return EAV_OK;
}

static int pool_ok(const char* who, int B, int H, int W, int C, int OH, int OW, int K, int S, int P) {
  if (!(B > 0 && H > 0 && W > 0 && C > 0 && C <= MAXCH && K > 0 && K <= MAXK && S > 0 && P >= 0 && 2 * P <= K &&
        H + 2 * P >= K && W + 2 * P >= K && (int64_t)B * H * W * C < (1LL << 31)))
    return eav_set_error(EAV_EINVAL, "%s: bad sizes (B %d, H %d, W %d, C %d, kernel %d, stride %d, pad %d)", who, B, H, W,
                         C, K, S, P);
  if (OH != (H + 2 * P - K) / S + 1 || OW != (W + 2 * P - K) / S + 1)
    return eav_set_error(EAV_EINVAL, "%s: output map %dx%d, the geometry gives %dx%d", who, OH, OW,
                         (H + 2 * P - K) / S + 1, (W + 2 * P - K) / S + 1);
  return EAV_OK;
}

extern "C" int eav_video_maxpool_fwd(const float* x, float* out, uint8_t* idx, int B, int H, int W, int C, int OH,
                                     int OW, int K, int S, int P, void* stream) {
  EAV_REQUIRE(x && out && idx, "eav_video_maxpool_fwd: null tensor");
  if (int rc = pool_ok("eav_video_maxpool_fwd", B, H, W, C, OH, OW, K, S, P)) return rc;
  hipLaunchKernelGGL(maxpool_fwd_kernel, dim3(ew_blocks((int64_t)B * OH * OW * C)), dim3(256), 0, (hipStream_t)stream,
                     x, out, idx, B, H, W, C, OH, OW, K, S, P);
  EAV_CHECK_LAUNCH("eav_video_maxpool_fwd");
  return EAV_OK;
}

extern "C" int eav_video_maxpool_bwd(const float* dout, const uint8_t* idx, float* dx, int B, int H, int W, int C,
                                     int OH, int OW, int K, int S, int P, void* stream) {
  EAV_REQUIRE(dout && idx && dx, "eav_video_maxpool_bwd: null tensor");
  if (int rc = pool_ok("eav_video_maxpool_bwd", B, H, W, C, OH, OW, K, S, P)) return rc;
  hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(ew_blocks((int64_t)B * H * W * C)), dim3(256), 0, (hipStream_t)stream,
                     dout, idx, dx, B, H, W, C, OH, OW, K, S, P);
  EAV_CHECK_LAUNCH("eav_video_maxpool_bwd");
  return EAV_OK;
}

#define HEAD_OK(who)                                                                                          \
  EAV_REQUIRE(B > 0 && HW > 0 && HW <= 256 && C > 0 && C <= MAXCH && (int64_t)B * C < (1LL << 24),          \
              who ": bad sizes (B %d, HW %d, C %d; the argmax is a byte: HW <= 256)", B, HW, C)

extern "C" int eav_video_head_pool(const float* y, float* pooled, uint8_t* idx, int B, int HW, int C, void* stream) {
  EAV_REQUIRE(y && pooled && idx, "eav_video_head_pool: null tensor");
  HEAD_OK("eav_video_head_pool");
  hipLaunchKernelGGL(head_pool_kernel, dim3(cdiv(B * C, 256)), dim3(256), 0, (hipStream_t)stream, y, pooled, idx, B, HW,
                     C);
  EAV_CHECK_LAUNCH("eav_video_head_pool");
  return EAV_OK;
}

extern "C" int eav_video_head_scale_pool(const float* y, const float* A, float* attn, float* z, int B, int HW, int C,
                                         void* stream) {
  EAV_REQUIRE(y && A && attn && z, "eav_video_head_scale_pool: null tensor");
  HEAD_OK("eav_video_head_scale_pool");
  hipLaunchKernelGGL(head_scale_pool_kernel, dim3(cdiv(B * C, 256)), dim3(256), 0, (hipStream_t)stream, y, A, attn, z, B,
                     HW, C);
  EAV_CHECK_LAUNCH("eav_video_head_scale_pool");
  return EAV_OK;
}

extern "C" int eav_video_head_attn_bwd(const float* y, const float* dz, float* dA, int B, int HW, int C, void* stream) {
  EAV_REQUIRE(y && dz && dA, "eav_video_head_attn_bwd: null tensor");
  HEAD_OK("eav_video_head_attn_bwd");
  hipLaunchKernelGGL(head_attn_bwd_kernel, dim3(cdiv(B * C, 256)), dim3(256), 0, (hipStream_t)stream, y, dz, dA, B, HW,
                     C);
  EAV_CHECK_LAUNCH("eav_video_head_attn_bwd");
  return EAV_OK;
}

extern "C" int eav_video_head_feat_bwd(const float* dz, const float* attn, const float* dP, const uint8_t* idx,
                                       float* dy, int B, int HW, int C, void* stream) {
  EAV_REQUIRE(dz && attn && dP && idx && dy, "eav_video_head_feat_bwd: null tensor");
  HEAD_OK("eav_video_head_feat_bwd");
  hipLaunchKernelGGL(head_feat_bwd_kernel, dim3(ew_blocks((int64_t)B * HW * C)), dim3(256), 0, (hipStream_t)stream, dz,
                     attn, dP, idx, dy, B, HW, C);
  EAV_CHECK_LAUNCH("eav_video_head_feat_bwd");
  return EAV_OK;
}

extern "C" int eav_video_counters_inc(int64_t* c, int n, void* stream) {
  EAV_REQUIRE(c && n > 0 && n <= 4096, "eav_video_counters_inc: bad arguments");
  hipLaunchKernelGGL(counters_inc_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, c, n);
  EAV_CHECK_LAUNCH("eav_video_counters_inc");
  return EAV_OK;
}
