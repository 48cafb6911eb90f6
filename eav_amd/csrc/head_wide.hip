// The wide classification head: nn.Linear(hidden, classes) and nn.CrossEntropyLoss for more classes than the 16 that
// eav_dense_softmax_* / eav_ce_fwd_bwd (head_optim.hip) keep in registers - the 527 AudioSet labels of the stock AST
// checkpoint (Transformer_Audio.py:22 loads it before the head is swapped), ImageNet's 1000, ImageNet-21k's 21 843.
//
//   eav_dense_wide_fwd   logits[B,NC] = in[B,NF] . w[NC,NF]^T + bias
//   eav_dense_wide_bwd   dw[NC,NF] = dlogits^T . in,  dbias = column sums of dlogits,  din[B,NF] = dlogits . w
//   eav_ce_wide_fwd_bwd  mean cross-entropy, its gradient and the hit count, one wave per row
//
// The three products run on v_mfma_f32_32x32x2_f32 (an exact k-ordered fp32 fma chain) through one tile kernel that takes
// its operands by strides.  With 8..128 batch rows the products are short of tiles, not of flops, so the kernel has two
// shapes of block: 64 x 64 outputs with one wave per 32 x 32 quarter where that fills the machine, and 32 x 32 outputs
// with the four waves splitting the contraction (their accumulators added through LDS in wave order) where it does not.
// Which one runs, and where the contraction of din is cut, depends on the shape alone: there are no atomics, and two runs
// give the same bits.
#include "eav_common.h"
#include "../../include/eav_hip.h"

namespace {

struct WideArgs {
  const float* A;         // A(m, k) at A[m sAm + k sAk]
  const float* Bm;        // B(n, k) at Bm[n sBn + k sBk]
  float* C;               // C[z][m ldc + n], z = blockIdx.z (slices of the contraction, kper each)
  const float* bias;      // + bias[n] (or null)
  float* colsum;          // colsum[m] = sum_k A(m, k) in k order (or null), written by the blocks of column tile 0
  int M, N, K, ldc, kper;
  int64_t sAm, sAk, sBn, sBk, sCz;
};

constexpr int WKS = 32;   // contraction elements per wave per LDS chunk (16 MFMAs)

// WM x WN x WK = 4 waves: WM x WN tiles of 32 x 32 outputs, WK slices of every chunk of the contraction.
// AK / BK: the operand is contiguous along k (else along its row index) - picks the coalesced order of the staging loads.
template <int WM, int WN, int WK, bool AK, bool BK>
__global__ __launch_bounds__(256) void wide_gemm_kernel(WideArgs a) {
  static_assert(WM * WN * WK == 4 && (WK == 1 || WM * WN == 1), "four waves; the k-split block owns one 32 x 32 tile");
  constexpr int TM = 32 * WM, TN = 32 * WN, KT = WKS * WK, LD = KT + 1;     // odd row stride: 32 rows hit 32 banks
  constexpr int NA = TM * KT / 256, NB = TN * KT / 256;
  __shared__ float As[TM][LD];
  __shared__ float Bs[TN][LD];
  __shared__ float red[WK > 1 ? WK * 1024 : 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int wk = wave % WK, wn = (wave / WK) % WN, wm = wave / (WK * WN);
  const int m0 = blockIdx.y * TM, n0 = blockIdx.x * TN;
  const int kbeg = blockIdx.z * a.kper, kend = min(a.K, kbeg + a.kper);
  const bool sums = a.colsum && blockIdx.x == 0 && tid < TM;

  // element e of a staged tile: (row, k) with the contiguous index fastest
  auto arow = [](int e) { return AK ? e / KT : e % TM; };
  auto acol = [](int e) { return AK ? e % KT : e / TM; };
  auto brow = [](int e) { return BK ? e / KT : e % TN; };
  auto bcol = [](int e) { return BK ? e % KT : e / TN; };
  float pa[NA], pb[NB];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int e = tid + 256 * i, m = m0 + arow(e), k = k0 + acol(e);
      pa[i] = (m < a.M && k < kend) ? a.A[(int64_t)m * a.sAm + (int64_t)k * a.sAk] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int e = tid + 256 * i, n = n0 + brow(e), k = k0 + bcol(e);
      pb[i] = (n < a.N && k < kend) ? a.Bm[(int64_t)n * a.sBn + (int64_t)k * a.sBk] : 0.f;
    }
  };

  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  float cs = 0.f;
  fetch(kbeg);
  for (int k0 = kbeg; k0 < kend; k0 += KT) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NA; ++i) As[arow(tid + 256 * i)][acol(tid + 256 * i)] = pa[i];
#pragma unroll
    for (int i = 0; i < NB; ++i) Bs[brow(tid + 256 * i)][bcol(tid + 256 * i)] = pb[i];
    __syncthreads();
    if (k0 + KT < kend) fetch(k0 + KT);       // the next chunk travels while this one multiplies
    if (sums)
      for (int k = 0; k < KT; ++k) cs += As[tid][k];
#pragma unroll
    for (int s = 0; s < WKS / 2; ++s) {
      const int k = wk * WKS + 2 * s + h;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[wm * 32 + r][k], Bs[wn * 32 + r][k], acc, 0, 0, 0);
    }
  }
  if (sums && m0 + tid < a.M) a.colsum[m0 + tid] = cs;

  // D: column (lane & 31), row (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  float* C = a.C + (int64_t)blockIdx.z * a.sCz;
  if constexpr (WK > 1) {
#pragma unroll
    for (int i = 0; i < 16; ++i) red[(wk * 16 + i) * 64 + lane] = acc[i];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int o = tid + 256 * j, i = o >> 6, l = o & 63;
      float v = red[o];
#pragma unroll
      for (int q = 1; q < WK; ++q) v += red[q * 1024 + o];
      const int m = m0 + (i & 3) + 8 * (i >> 2) + 4 * (l >> 5), n = n0 + (l & 31);
      if (m < a.M && n < a.N) C[(int64_t)m * a.ldc + n] = a.bias ? v + a.bias[n] : v;
    }
  } else {
    const int n = n0 + wn * 32 + r;
    if (n < a.N) {
      const float bs = a.bias ? a.bias[n] : 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int m = m0 + wm * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
        if (m < a.M) C[(int64_t)m * a.ldc + n] = a.bias ? acc[i] + bs : acc[i];
      }
    }
  }
}

// The block shape and the cut of the contraction for a product of M x N outputs over K, from the shape alone.
// zmax: the most slices the caller can take (1: the product writes its result itself).
struct WidePlan {
  bool big;     // 64 x 64 blocks
  int z, kper;
};

WidePlan wide_plan(int M, int N, int K, int zmax) {
  WidePlan p;
  const int tiles64 = cdiv(M, 64) * cdiv(N, 64);
  p.big = M > 32 && (int64_t)tiles64 * zmax >= 256;
  const int tiles = p.big ? tiles64 : cdiv(M, 32) * cdiv(N, 32);
  const int kt = p.big ? WKS : 4 * WKS;
  int z = cdiv(1024, tiles);
  if (z > zmax) z = zmax;
  p.kper = cdiv(cdiv(K, z), kt) * kt;
  p.z = cdiv(K, p.kper);
  return p;
}

template <bool AK, bool BK>
void wide_launch(const WideArgs& a, const WidePlan& p, hipStream_t st) {
  if (p.big)
    hipLaunchKernelGGL((wide_gemm_kernel<2, 2, 1, AK, BK>), dim3(cdiv(a.N, 64), cdiv(a.M, 64), p.z), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((wide_gemm_kernel<1, 1, 4, AK, BK>), dim3(cdiv(a.N, 32), cdiv(a.M, 32), p.z), dim3(256), 0, st, a);
}

int din_zmax(int NC) { return cdiv(NC, 256); }

bool wide_shape_ok(int B, int NF, int NC) {
  return B > 0 && NF > 0 && (NF & 3) == 0 && NF <= 1024 && NC > 0 && NC <= EAV_HEAD_MAX_CLASSES &&
         (int64_t)B * NC < (1ll << 31) && (int64_t)B * NF < (1ll << 31);
}

// ---- cross-entropy ---------------------------------------------------------------------------------------------------
// (value, index) of the larger value, the smaller index on a tie
__device__ __forceinline__ void argmax_merge(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

// One wave per row (four rows per block): maximum and first arg-maximum, log-sum-exp and the gradient row, every read and
// write of the row coalesced over the 64 lanes.  terms[b] = the row's loss term, terms[B + b] = 1 for a hit.
__global__ __launch_bounds__(256) void ce_wide_rows_kernel(const float* __restrict__ in, const int64_t* __restrict__ y,
                                                           float* __restrict__ din, int* __restrict__ bad_label,
                                                           float* __restrict__ terms, int B, int NC) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  // the mean's divisor: every wave counts the valid labels itself (integers: any order gives the same count)
  int cnt = 0;
  for (int i = lane; i < B; i += 64) {
    const int64_t yl = y[i];
    cnt += (yl >= 0 && yl < NC) ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  const float nvalid = (float)cnt;

  const float* r = in + (int64_t)b * NC;
  float mx = -__builtin_inff();
  int am = 0x7fffffff;
  for (int j = lane; j < NC; j += 64) {
    const float v = r[j];
    if (v > mx) { mx = v; am = j; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(mx, o, 64);
    const int oi = __shfl_xor(am, o, 64);
    argmax_merge(mx, am, ov, oi);
  }
  float s = 0.f;
  for (int j = lane; j < NC; j += 64) s += expf(r[j] - mx);
  s = wave_sum(s);
  // log-softmax as (r - max) - log(sum), torch's form: mx + log(sum) first would round at the magnitude of the logits
  const float ls = logf(s);
  const int64_t yl = y[b];
  const bool ok = yl >= 0 && yl < NC;            // never index with a label outside [0, NC)
  if (lane == 0) {
    if (!ok && yl != -100 && bad_label)
      *bad_label = yl >= 0 ? (int)min(yl, (int64_t)0x7ffffffe) + 1 : (int)max(yl, (int64_t)-0x7fffffff);
    const int yy = ok ? (int)yl : -1;
    terms[b] = ok ? ls - (r[yy] - mx) : 0.f;
    terms[B + b] = (am == yy) ? 1.f : 0.f;
  }
  if (din) {
    const int yy = ok ? (int)yl : -1;
    float* d = din + (int64_t)b * NC;
    for (int j = lane; j < NC; j += 64) d[j] = ok ? (expf((r[j] - mx) - ls) - (j == yy ? 1.f : 0.f)) / nvalid : 0.f;
  }
}

// The per-row terms added in row order: 64 consecutive rows per trip (a wave sum), the trips one after another.
__global__ __launch_bounds__(64) void ce_wide_finish_kernel(const float* __restrict__ terms, const int64_t* __restrict__ y,
                                                            float* __restrict__ loss, int* __restrict__ ncorrect, int B,
                                                            int NC) {
  const int lane = threadIdx.x;
  float tot = 0.f;
  int hits = 0, cnt = 0;
  for (int b0 = 0; b0 < B; b0 += 64) {
    const int b = b0 + lane;
    tot += wave_sum(b < B ? terms[b] : 0.f);
    hits += (b < B && terms[B + b] != 0.f) ? 1 : 0;
    if (b < B) {
      const int64_t yl = y[b];
      cnt += (yl >= 0 && yl < NC) ? 1 : 0;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    hits += __shfl_xor(hits, o, 64);
    cnt += __shfl_xor(cnt, o, 64);
  }
  // all targets ignored: torch returns nan (0 / 0)
  if (lane == 0 && loss) *loss = cnt > 0 ? tot / (float)cnt : __builtin_nanf("");
  if (lane == 1 && ncorrect) *ncorrect += hits;
}

}  // namespace

extern "C" int eav_dense_wide_fwd(const float* in, const float* w, const float* bias, float* logits, int B, int NF, int NC,
                                  void* stream) {
  EAV_REQUIRE(in && w && bias && logits && wide_shape_ok(B, NF, NC),
              "eav_dense_wide_fwd: bad arguments (features a multiple of 4 up to 1024, classes <= %d)", EAV_HEAD_MAX_CLASSES);
  WideArgs a{in, w, logits, bias, nullptr, B, NC, NF, NC, 0, NF, 1, NF, 1, 0};
  const WidePlan p = wide_plan(B, NC, NF, 1);
  a.kper = p.kper;
  wide_launch<true, true>(a, p, (hipStream_t)stream);
  EAV_CHECK_LAUNCH("eav_dense_wide_fwd");
  return EAV_OK;
}

extern "C" int64_t eav_dense_wide_bwd_ws_floats(int B, int NF, int NC) {
  if (!wide_shape_ok(B, NF, NC)) return 0;
  const WidePlan p = wide_plan(B, NF, NC, din_zmax(NC));
  return p.z > 1 ? (int64_t)p.z * B * NF : 0;
}

extern "C" int eav_dense_wide_bwd(const float* dlogits, const float* in, const float* w, float* dw, float* dbias,
                                  float* din, float* ws, int B, int NF, int NC, void* stream) {
  EAV_REQUIRE(dlogits && in && w && dw && dbias && wide_shape_ok(B, NF, NC),
              "eav_dense_wide_bwd: bad arguments (features a multiple of 4 up to 1024, classes <= %d)", EAV_HEAD_MAX_CLASSES);
  // dw[c, f] = sum_b dlogits[b, c] in[b, f]; the blocks of the first feature tile leave dbias[c] = sum_b dlogits[b, c]
  WideArgs g{dlogits, in, dw, nullptr, dbias, NC, NF, B, NF, 0, 1, NC, 1, NF, 0};
  const WidePlan pg = wide_plan(NC, NF, B, 1);
  g.kper = pg.kper;
  wide_launch<false, false>(g, pg, (hipStream_t)stream);
  EAV_CHECK_LAUNCH("eav_dense_wide_bwd");
  if (!din) return EAV_OK;
  // din[b, f] = sum_c dlogits[b, c] w[c, f]: the classes cut into p.z slices, the slices' partial results added in slice order
  const WidePlan p = wide_plan(B, NF, NC, din_zmax(NC));
  EAV_REQUIRE(p.z == 1 || ws, "eav_dense_wide_bwd: workspace of eav_dense_wide_bwd_ws_floats() floats needed");
  WideArgs d{dlogits, w, p.z > 1 ? ws : din, nullptr, nullptr, B, NF, NC, NF, p.kper, NC, 1, 1, NF, (int64_t)B * NF};
  wide_launch<true, false>(d, p, (hipStream_t)stream);
  EAV_CHECK_LAUNCH("eav_dense_wide_bwd");
  if (p.z > 1) return eav_reduce_partials(ws, p.z, (int64_t)B * NF, B * NF, 1.f, din, stream);
  return EAV_OK;
}

extern "C" int64_t eav_ce_wide_ws_floats(int B) { return B > 0 ? 2 * (int64_t)B : 0; }

extern "C" int eav_ce_wide_fwd_bwd(const float* in, const int64_t* y, float* loss, float* din, int* ncorrect,
                                   int* bad_label, float* ws, int B, int NC, void* stream) {
  EAV_REQUIRE(in && y && ws && B > 0 && NC > 0 && (int64_t)B * NC < (1ll << 31), "eav_ce_wide_fwd_bwd: bad arguments");
  hipLaunchKernelGGL(ce_wide_rows_kernel, dim3(cdiv(B, 4)), dim3(256), 0, (hipStream_t)stream, in, y, din, bad_label, ws, B,
                     NC);
  EAV_CHECK_LAUNCH("eav_ce_wide_fwd_bwd");
  if (loss || ncorrect) {
    hipLaunchKernelGGL(ce_wide_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, ws, y, loss, ncorrect, B, NC);
    EAV_CHECK_LAUNCH("eav_ce_wide_fwd_bwd");
  }
  return EAV_OK;
}
