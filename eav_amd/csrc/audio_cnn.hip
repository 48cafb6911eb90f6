// The audio CNN of CNN_torch/CNN_audio.py (AudioModel) on the gfx950 fp32 matrix cores (v_mfma_f32_32x32x2_f32: an exact
// k-ordered f32 fma chain, so parity with CPU torch is limited by summation order only).
//
//   features: Conv1d(1,256,5,p2) ReLU Conv1d(256,128,5,p2) ReLU Dropout(0.1) MaxPool1d(8)
//             Conv1d(128,128,5,p2) ReLU Conv1d(128,128,5,p2) ReLU Dropout(0.5)      -> Linear(128*22, C)
//
// Every convolution of the network (kernel 5, padding 2) and both of its gradients are one of three kernels:
//
//   conv5_kernel<CI, TRANS, EPI>  implicit GEMM  out[b][n][t] = sum_{c,tap} W(n,c,tap) in[b][c][t+tap-2]
//       rows = 32 output positions, columns = 128 output channels (4 waves x 32), contraction = (tap, channel) in chunks
//       of CI channels staged in LDS.  TRANS = 0: the layer's forward (W = w[n][c][tap]); TRANS = 1: its data gradient
//       (W = w[c][n][4-tap], in = d out).  Epilogues: bias + ReLU (+ dropout) store; bias + ReLU + dropout + MaxPool(8)
//       with the window argmax (conv2); ReLU' gate (the data gradients of conv4 and conv2); MaxPool / dropout / ReLU
//       backward scattered into the dense conv2 output gradient (the data gradient of conv3).
//   conv5_wgrad_kernel            dW[m][c*5+tap] = sum_{b,t} dout[b][m][t] act[b][c][t+tap-2] and db[m] = sum dout,
//       split over (sample, 32-position chunk) into `nparts` partials, summed in fixed order by eav_reduce_partials.
//
// No float atomics: every output element is written by exactly one lane, every sum has a fixed order (bit-reproducible).
// The classifier runs on the existing eav_dense_softmax_fwd / _bwd, the loss on eav_ce_fwd_bwd.
#include "eav_common.h"
#include "../../include/eav_hip.h"

namespace {

constexpr int TM = 32;     // output positions per workgroup
constexpr int TN = 128;    // output channels per workgroup (4 waves x 32)
constexpr int XW = TM + 4; // staged input positions (the 5-tap halo)

enum { EPI_RELU = 0, EPI_POOL = 1, EPI_GATE = 2, EPI_SCATTER = 3 };

struct ConvArgs {
  const float* in;        // [B][C][Lin]
  const float* gate_in;   // optional [B][C][Lin]: in is multiplied by (gate_in > 0 ? gscale_in : 0) as it is staged
  const float* w;         // the layer's weight [Cout][Cin][5]
  const float* bias;      // [N] (forward only)
  float* out;
  uint8_t* idx_out;       // EPI_POOL: argmax within each window
  const uint8_t* idx_in;  // EPI_SCATTER: the forward's argmax
  const float* aux;       // EPI_GATE: activation whose ReLU' gates the output; EPI_SCATTER: the pooled forward output
  const uint8_t* mask;    // explicit dropout keep-mask [B][N][Lin] (testing hook) or null
  const uint64_t* seed_dev;
  uint64_t seed;
  float drop_p;
  float gscale_in, gscale_out;
  int C, N, Lin, Lout;    // contraction channels, output channels, input length, computed output positions
};

// ReLU as torch computes it (a NaN stays a NaN) and the gate of its backward (threshold_backward: zero where the
// output is <= 0, so a NaN output passes the gradient)
__device__ __forceinline__ float relu_f(float v) { return v < 0.f ? 0.f : v; }

template <int CI, bool TRANS, int EPI>
__global__ __launch_bounds__(256) void conv5_kernel(ConvArgs a) {
  constexpr int KS = (CI * 5 + 1) / 2;   // MFMA k-steps per chunk (k = tap * CI + channel)
  constexpr int WLD = 2 * KS + 1;        // odd LDS row stride: the 32 lanes of a half-wave read 32 banks
  __shared__ float xs[CI][XW];
  __shared__ float ws[TN][WLD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int t0 = blockIdx.x * TM, n0 = blockIdx.y * TN, b = blockIdx.z;
  const int64_t inb = (int64_t)b * a.C * a.Lin;
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;

  for (int c0 = 0; c0 < a.C; c0 += CI) {
    __syncthreads();
    for (int e = threadIdx.x; e < CI * XW; e += 256) {
      const int c = e / XW, j = e - c * XW, t = t0 + j - 2;
      float v = 0.f;
      if (c0 + c < a.C && t >= 0 && t < a.Lin) {
        const int64_t o = inb + (int64_t)(c0 + c) * a.Lin + t;
        v = a.in[o];
        if (a.gate_in) v = a.gate_in[o] > 0.f ? v * a.gscale_in : 0.f;
      }
      xs[c][j] = v;
    }
    if (!TRANS) {   // w[n][c][tap]: the chunk is CI*5 consecutive floats of every row n
      for (int e = threadIdx.x; e < TN * 2 * KS; e += 256) {
        const int n = e / (2 * KS), g = e - n * (2 * KS), c = g / 5, tap = g - 5 * c;
        float v = 0.f;
        if (g < CI * 5 && n0 + n < a.N && c0 + c < a.C) v = a.w[((int64_t)(n0 + n) * a.C + c0 + c) * 5 + tap];
        if (g < CI * 5) ws[n][tap * CI + c] = v;
        else ws[n][g] = 0.f;
      }
    } else {        // w[c][n][tap] (c: the layer's output channel = this product's contraction channel), flipped taps
      for (int e = threadIdx.x; e < CI * TN * 5; e += 256) {
        const int c = e / (TN * 5), g = e - c * (TN * 5), n = g / 5, tap = g - 5 * n;
        float v = 0.f;
        if (n0 + n < a.N && c0 + c < a.C) v = a.w[((int64_t)(c0 + c) * a.N + n0 + n) * 5 + tap];
        ws[n][(4 - tap) * CI + c] = v;
      }
      if (CI * 5 < 2 * KS)
        for (int n = threadIdx.x; n < TN; n += 256) ws[n][2 * KS - 1] = 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int k = 2 * s + h, tap = k / CI, c = k - tap * CI;
      const float av = tap < 5 ? xs[c][r + tap] : 0.f;         // A[row = position r][k]
      const float bv = ws[wave * 32 + r][k];                     // B[k][column = channel r]
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
    }
  }

  // D: column (lane & 31) = output channel, row (reg & 3) + 8 (reg >> 2) + 4 h = output position
  const int n = n0 + wave * 32 + r;
  const bool nok = n < a.N;
  const int64_t row = ((int64_t)b * a.N + (nok ? n : 0));
  if (EPI == EPI_RELU) {
    const float bs = nok ? a.bias[n] : 0.f;
    const uint64_t sd = dropout_seed(a.seed, a.seed_dev);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int t = t0 + (i & 3) + 8 * (i >> 2) + 4 * h;
      if (nok && t < a.Lout) {
        float v = relu_f(acc[i] + bs);
        if (a.drop_p > 0.f) v *= dropout_mult(a.drop_p, sd, a.mask, (uint64_t)(row * a.Lin + t));
        a.out[row * a.Lout + t] = v;
      }
    }
  } else if (EPI == EPI_POOL) {
    // ReLU -> Dropout -> MaxPool1d(8): window q of this tile is rows 8q..8q+7; lane half 0 holds 8q..8q+3, half 1 the
    // rest.  torch's CPU max-pool scans the window in order and takes `v > max || isnan(v)`: ties keep the first index,
    // a NaN propagates.
    const float bs = nok ? a.bias[n] : 0.f;
    const uint64_t sd = dropout_seed(a.seed, a.seed_dev);
    const int nwin = a.Lout / 8;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float m = 0.f;
      int mi = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int t = t0 + 8 * q + 4 * h + j;
        float v = relu_f(acc[4 * q + j] + bs);
        if (a.drop_p > 0.f && nok && t < a.Lin)
          v *= dropout_mult(a.drop_p, sd, a.mask, (uint64_t)(row * a.Lin + t));
        if (j == 0 || v > m || v != v) { m = v; mi = 4 * h + j; }
      }
      const float m1 = __shfl_xor(m, 32, 64);
      const int i1 = __shfl_xor(mi, 32, 64);
      if (h == 0) {
        if (m1 > m || m1 != m1) { m = m1; mi = i1; }
        const int wdx = t0 / 8 + q;
        if (nok && wdx < nwin) {
          a.out[row * nwin + wdx] = m;
          a.idx_out[row * nwin + wdx] = (uint8_t)mi;
        }
      }
    }
  } else if (EPI == EPI_GATE) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int t = t0 + (i & 3) + 8 * (i >> 2) + 4 * h;
      if (nok && t < a.Lout) {
        const int64_t o = row * a.Lout + t;
        a.out[o] = (a.aux && a.aux[o] <= 0.f) ? 0.f : acc[i];
      }
    }
  } else {   // EPI_SCATTER: d pooled -> d conv2 output (dense, 8 Lout per row): the gradient lands on the window's argmax,
             // times the dropout scale, where the pooled value (ReLU then dropout of that position) is positive
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int t = t0 + (i & 3) + 8 * (i >> 2) + 4 * h;
      if (nok && t < a.Lout) {
        const int64_t o = row * a.Lout + t;
        const float g = a.aux[o] > 0.f ? acc[i] * a.gscale_out : 0.f;
        const int am = a.idx_in[o];
        float4* dst = reinterpret_cast<float4*>(a.out + (row * a.Lout + t) * 8);
        dst[0] = make_float4(am == 0 ? g : 0.f, am == 1 ? g : 0.f, am == 2 ? g : 0.f, am == 3 ? g : 0.f);
        dst[1] = make_float4(am == 4 ? g : 0.f, am == 5 ? g : 0.f, am == 6 ? g : 0.f, am == 7 ? g : 0.f);
      }
    }
  }
}

// dW partials.  Workgroup tile: 64 output channels (rows m) x 64 weight columns (n = c*5 + tap), 2 x 2 waves of 32 x 32;
// contraction over positions t, 32 per chunk, chunks (sample, position block) q = part, part + nparts, ...
constexpr int WM = 64, WN = 64, WT = 32;
constexpr int ACI = WN / 5 + 2;    // activation rows a 64-column tile touches (at most 14)

struct WgradArgs {
  const float* dout;     // [B][M][Lout]
  const float* gate;     // optional [B][M][Lout]: dout multiplied by (gate > 0 ? gscale : 0)
  const float* act;      // [B][Cact][Lact]
  float* part;           // [nparts][M * Cact * 5 + M]
  float gscale;
  int B, M, Cact, Lact, Lout, nparts;
};

__global__ __launch_bounds__(256) void conv5_wgrad_kernel(WgradArgs a) {
  __shared__ float ds[WM][WT + 1];
  __shared__ float as[ACI][WT + 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5, wm = wave >> 1, wn = wave & 1;
  const int NC = a.Cact * 5;
  const int n0 = blockIdx.x * WN, m0 = blockIdx.y * WM, p = blockIdx.z;
  const int cbase = n0 / 5;
  const int n = n0 + wn * 32 + r;                 // this lane's B column
  const int nc = n < NC ? n / 5 - cbase : 0, ntap = n < NC ? n - 5 * (n / 5) : 0;
  const bool bias_tile = blockIdx.x == 0;
  const int nct = (a.Lout + WT - 1) / WT, nq = a.B * nct;
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  float bsum = 0.f;

  for (int q = p; q < nq; q += a.nparts) {
    const int b = q / nct, t0 = (q - b * nct) * WT;
    __syncthreads();
    for (int e = threadIdx.x; e < WM * WT; e += 256) {
      const int m = e / WT, j = e - m * WT, t = t0 + j;
      float v = 0.f;
      if (m0 + m < a.M && t < a.Lout) {
        const int64_t o = ((int64_t)b * a.M + m0 + m) * a.Lout + t;
        v = a.dout[o];
        if (a.gate) v = a.gate[o] > 0.f ? v * a.gscale : 0.f;
      }
      ds[m][j] = v;
    }
    for (int e = threadIdx.x; e < ACI * (WT + 4); e += 256) {
      const int c = e / (WT + 4), j = e - c * (WT + 4), t = t0 + j - 2;
      float v = 0.f;
      if (cbase + c < a.Cact && t >= 0 && t < a.Lact) v = a.act[((int64_t)b * a.Cact + cbase + c) * a.Lact + t];
      as[c][j] = v;
    }
    __syncthreads();
    if (bias_tile && threadIdx.x < WM) {
#pragma unroll 8
      for (int j = 0; j < WT; ++j) bsum += ds[threadIdx.x][j];
    }
#pragma unroll
    for (int s = 0; s < WT / 2; ++s) {
      const int k = 2 * s + h;
      const float av = ds[wm * 32 + r][k];          // A[row = output channel r][k = position]
      const float bv = as[nc][k + ntap];            // B[k][column n = (c, tap)]
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
    }
  }

  const int64_t stride = (int64_t)a.M * NC + a.M;
  float* dst = a.part + p * stride;
  if (n < NC) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int m = m0 + wm * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
      if (m < a.M) dst[(int64_t)m * NC + n] = acc[i];
    }
  }
  if (bias_tile && threadIdx.x < WM && m0 + threadIdx.x < a.M) dst[(int64_t)a.M * NC + m0 + threadIdx.x] = bsum;
}

template <int CI, bool TRANS, int EPI>
int launch_conv(const ConvArgs& a, int B, hipStream_t st) {
  hipLaunchKernelGGL((conv5_kernel<CI, TRANS, EPI>), dim3(cdiv(a.Lout, TM), cdiv(a.N, TN), B), dim3(256), 0, st, a);
  return 0;
}

constexpr int MAXCH = 4096;

}  // namespace

extern "C" int eav_audio_conv5_fwd(const float* in, const float* w, const float* bias, float* out, uint8_t* idx, int B,
                                   int C, int N, int Lin, int Lout, int pool, float drop_p, uint64_t seed,
                                   const uint8_t* mask, const uint64_t* seed_dev, void* stream) {
  EAV_REQUIRE(in && w && bias && out, "eav_audio_conv5_fwd: null tensor");
  EAV_REQUIRE(B > 0 && B <= 65535 && C > 0 && C <= MAXCH && N > 0 && N <= MAXCH && Lin > 0 && Lout > 0,
              "eav_audio_conv5_fwd: bad sizes (B %d, C %d, N %d, Lin %d, Lout %d)", B, C, N, Lin, Lout);
  EAV_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "eav_audio_conv5_fwd: dropout probability %g outside [0, 1)", drop_p);
  EAV_REQUIRE(C == 1 || C % 16 == 0, "eav_audio_conv5_fwd: %d input channels (1 or a multiple of 16)", C);
  ConvArgs a{};
  a.in = in; a.w = w; a.bias = bias; a.out = out; a.idx_out = idx; a.mask = mask; a.seed_dev = seed_dev; a.seed = seed;
  a.drop_p = drop_p; a.C = C; a.N = N; a.Lin = Lin; a.Lout = Lout;
  const hipStream_t st = (hipStream_t)stream;
  if (pool) {
    // MaxPool1d(8) of a length-preserving conv: floor(Lin / 8) windows, and the classifier of CNN_audio.py fixes their
    // number - Lout = 8 x windows is what the caller's model needs, so any other input length is refused here
    EAV_REQUIRE(idx, "eav_audio_conv5_fwd: pool needs the argmax buffer");
    EAV_REQUIRE(Lout % 8 == 0 && Lin / 8 == Lout / 8,
                "eav_audio_conv5_fwd: input length T = %d gives %d pooled positions, the classifier needs %d "
                "(T in %d...%d)", Lin, Lin / 8, Lout / 8, Lout, Lout + 7);
    EAV_REQUIRE(C % 16 == 0, "eav_audio_conv5_fwd: pool form needs a multiple of 16 input channels");
    launch_conv<16, false, EPI_POOL>(a, B, st);
  } else {
    EAV_REQUIRE(Lout == Lin, "eav_audio_conv5_fwd: a padding-2 conv keeps the length (Lin %d, Lout %d)", Lin, Lout);
    if (C == 1) launch_conv<1, false, EPI_RELU>(a, B, st);
    else launch_conv<16, false, EPI_RELU>(a, B, st);
  }
  EAV_CHECK_LAUNCH("eav_audio_conv5_fwd");
  return EAV_OK;
}

extern "C" int eav_audio_conv5_dgrad(const float* dout, const float* gate_in, float gscale_in, const float* w,
                                     float* din, const float* aux, const uint8_t* idx, float gscale_out, int B, int C,
                                     int N, int Lin, int Lout, int mode, void* stream) {
  EAV_REQUIRE(dout && w && din, "eav_audio_conv5_dgrad: null tensor");
  EAV_REQUIRE(B > 0 && B <= 65535 && C > 0 && C <= MAXCH && C % 16 == 0 && N > 0 && N <= MAXCH && Lin > 0 && Lout > 0,
              "eav_audio_conv5_dgrad: bad sizes (B %d, C %d, N %d, Lin %d, Lout %d)", B, C, N, Lin, Lout);
  EAV_REQUIRE(mode == 0 || mode == 1, "eav_audio_conv5_dgrad: mode %d", mode);
  EAV_REQUIRE(mode == 0 || (aux && idx), "eav_audio_conv5_dgrad: the pool scatter needs the pooled output and argmax");
  ConvArgs a{};
  a.in = dout; a.gate_in = gate_in; a.gscale_in = gscale_in; a.w = w; a.out = din; a.aux = aux; a.idx_in = idx;
  a.gscale_out = gscale_out; a.C = C; a.N = N; a.Lin = Lin; a.Lout = Lout;
  const hipStream_t st = (hipStream_t)stream;
  if (mode == 1) launch_conv<16, true, EPI_SCATTER>(a, B, st);
  else launch_conv<16, true, EPI_GATE>(a, B, st);
  EAV_CHECK_LAUNCH("eav_audio_conv5_dgrad");
  return EAV_OK;
}

extern "C" int eav_audio_wgrad_nparts(int B, int Cact, int M, int Lout) {
  if (B <= 0 || Cact <= 0 || M <= 0 || Lout <= 0) return 0;
  const int tiles = cdiv(Cact * 5, WN) * cdiv(M, WM);
  const int nq = B * cdiv(Lout, WT);
  int np = cdiv(768, tiles);            // ~3 workgroups per CU over the 256 CUs
  return np < 1 ? 1 : (np > nq ? nq : np);
}

extern "C" int eav_audio_conv5_wgrad(const float* dout, const float* gate, float gscale, const float* act, float* part,
                                     int B, int Cact, int M, int Lact, int Lout, int nparts, void* stream) {
  EAV_REQUIRE(dout && act && part, "eav_audio_conv5_wgrad: null tensor");
  EAV_REQUIRE(B > 0 && Cact > 0 && Cact <= MAXCH && M > 0 && M <= MAXCH && Lact > 0 && Lout > 0,
              "eav_audio_conv5_wgrad: bad sizes (B %d, Cact %d, M %d, Lact %d, Lout %d)", B, Cact, M, Lact, Lout);
  EAV_REQUIRE(nparts == eav_audio_wgrad_nparts(B, Cact, M, Lout),
              "eav_audio_conv5_wgrad: nparts %d, eav_audio_wgrad_nparts gives %d", nparts,
              eav_audio_wgrad_nparts(B, Cact, M, Lout));
  WgradArgs a{dout, gate, act, part, gscale, B, M, Cact, Lact, Lout, nparts};
  hipLaunchKernelGGL(conv5_wgrad_kernel, dim3(cdiv(Cact * 5, WN), cdiv(M, WM), nparts), dim3(256), 0,
                     (hipStream_t)stream, a);
  EAV_CHECK_LAUNCH("eav_audio_conv5_wgrad");
  return EAV_OK;
}
