// Attention probabilities of the fused attention (head_dim 64) written out after the fact, and attention rollout.
// HF returns softmax(Q K^T hd^-0.5) per layer under output_attentions=True (modeling_vit.py / modeling_audio_spectrogram_
// transformer.py, eager_attention_forward's second result); attention.hip and attention_sp.hip are flash-style and keep only
// lse [B*H, N].  These kernels read the operands the layer's own attention kernel consumed and the lse it wrote, and form
//   P[b, h, q, k] = exp2(log2(e) (scale q.k - lse[b, h, q]))
// the way the backward of the same precision does (attn_bwd_q_kernel / attn_bwd_q_sp_kernel): same operand order of the
// score MFMAs, same scaling, the native v_exp_f32 - up to rounding the probabilities the model used, not a second softmax
// (no row maximum, no row sum: one pass).
//
// Work split: one workgroup (4 waves) per (image, 32-query tile, 128-key tile); wave w owns the keys 32 w .. 32 w + 31 of
// the tile and all 32 queries.  The workgroup walks the H heads in order 0 .. H-1: the head mean accumulates in registers in
// that order (no atomics, the same bits on every run) and is written once at the end.
//
// Stores are what the kernel costs (ViT B = 128: 238 MB per layer).  In the accumulator layout a lane owns one query and
// 4- or 8-key runs of it, i.e. a store instruction would touch 32 different rows with 16- / 32-byte pieces.  Instead the
// [32 q][128 key] tile of a head is staged in LDS (row stride 129 floats) and leaves row by row: every store instruction of a
// wave writes 64 consecutive floats (256 contiguous bytes) of ONE row, two instructions per row.  The stores are dwords on
// purpose: a row of P starts at a multiple of 4 N bytes, which at N = 197 or 1214 is not a multiple of 16 for most rows, so
// a dwordx4 store would need a per-row peel; 64 lanes x 4 bytes already fill whole 128-byte lines wherever the row covers them.
// Ragged edges: queries >= N are never written; keys >= N are staged as zero rows (fp32) / the clamped last row (split, as
// the forward does) and never written.
// LDS: 8 + 32 KB of operands, the 16.5 KB output tile over them; three workgroups per CU; no scratch (tools/kernel_resources.py).
#include "eav_common.h"
#include "../../include/eav_hip.h"

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned char u8;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));      // a 16-byte piece in registers

constexpr int HD = 64;          // head dim
constexpr int KS = HD + 1;      // LDS row stride of the staged Q / K rows (attention.hip)
constexpr int TQ = 32;          // queries per workgroup
constexpr int TK = 128;         // keys per workgroup (4 waves x 32)
constexpr int OS = TK + 1;      // LDS row stride of the output tile
constexpr float LOG2E = 1.44269504088896340736f;

// accumulator register r of lane (j, kk) <-> streamed row: attention.hip's order / attention_sp.hip's order
__device__ __forceinline__ int kappa(int r, int kk) { return (r & 3) + 8 * (r >> 2) + 4 * kk; }
__device__ __forceinline__ int sp_row(int r, int h2) { return (r & 7) + 8 * h2 + 16 * (r >> 3); }
__device__ __forceinline__ int pi_row(int j) { return (j & ~12) | ((j & 4) << 1) | ((j & 8) >> 1); }

// Operand staging, the same for both precisions: per head a workgroup needs 32 query rows and 128 key rows of 256 bytes (64
// fp32, or 8 x (8 hi + 8 lo) halves), 2560 16-byte pieces = 10 per thread.  16 consecutive lanes fetch one row (whole
// 256-byte segments per instruction; the per-lane fragment loads of a row-per-lane layout touch 64 different lines per
// instruction and made the first version of this kernel address-bound), the pieces wait in registers while the previous head
// is computed and stored, then go to LDS: fp32 rows with stride KS (attention.hip's image), split rows as attention_sp.hip's
// row tile, piece p of row r in 16-byte slot r * 16 + (p ^ (r & 15)) (conflict-free ds_read_b128 fragments).
constexpr int NPIECE = (TQ + TK) * 16 / 256;      // 10
template <bool SPLIT>
__device__ __forceinline__ void fetch_pieces(const u8* __restrict__ qbase, const u8* __restrict__ kbase, int64_t ldbytes,
                                             int q0, int k0, int N, u32x4 (&reg)[NPIECE]) {
#pragma unroll
  for (int i = 0; i < NPIECE; ++i) {
    const int f = threadIdx.x + 256 * i;
    const int r = (i < TQ / 16 ? f : f - TQ * 16) >> 4, p = f & 15;
    const int row = (i < TQ / 16 ? q0 : k0) + r;
    const u8* base = i < TQ / 16 ? qbase : kbase;
    if (SPLIT)            // beyond N: the last row again (as the forward clamps; such keys / queries are never written)
      reg[i] = *reinterpret_cast<const u32x4*>(base + (int64_t)min(row, N - 1) * ldbytes + 16 * p);
    else                  // beyond N: zero rows
      reg[i] = row < N ? *reinterpret_cast<const u32x4*>(base + (int64_t)row * ldbytes + 16 * p) : u32x4{0u, 0u, 0u, 0u};
  }
}
template <bool SPLIT>
__device__ __forceinline__ void commit_pieces(float* __restrict__ Qs, float* __restrict__ Ks, const u32x4 (&reg)[NPIECE]) {
#pragma unroll
  for (int i = 0; i < NPIECE; ++i) {
    const int f = threadIdx.x + 256 * i;
    const int r = (i < TQ / 16 ? f : f - TQ * 16) >> 4, p = f & 15;
    float* tile = i < TQ / 16 ? Qs : Ks;
    if (SPLIT) {
      reinterpret_cast<u32x4*>(tile)[r * 16 + (p ^ (r & 15))] = reg[i];
    } else {
      float* d = tile + r * KS + 4 * p;
      d[0] = __uint_as_float(reg[i].x); d[1] = __uint_as_float(reg[i].y);
      d[2] = __uint_as_float(reg[i].z); d[3] = __uint_as_float(reg[i].w);
    }
  }
}
// operand fragment of a split row tile: row `row`, head_dim 16 s + 8 h2 .. + 7, hi (hl = 0) or lo (attention_sp.hip, frag_row)
__device__ __forceinline__ f16x8 frag_row(const float* tile, int row, int s, int h2, int hl) {
  return *reinterpret_cast<const f16x8*>(reinterpret_cast<const u8*>(tile) + row * 256 +
                                         (((4 * s + 2 * h2 + hl) ^ (row & 15)) << 4));
}

// the staged [TQ][TK] tile -> rows q0 .. of out [N, N], keys k0 ..: wave w writes rows 8 w .. 8 w + 7, each as two runs of 64
// consecutive floats
__device__ __forceinline__ void store_tile(const float* __restrict__ tile, float* __restrict__ out, int q0, int k0, int N,
                                           int wave, int lane) {
#pragma unroll
  for (int rr = 0; rr < TQ / 4; ++rr) {
    const int row = wave * (TQ / 4) + rr;
    if (q0 + row >= N) break;
    float* dst = out + (int64_t)(q0 + row) * N + k0;
#pragma unroll
    for (int i = 0; i < TK / 64; ++i) {
      const int col = lane + 64 * i;
      if (k0 + col < N) dst[col] = tile[row * OS + col];
    }
  }
}

// SPLIT false: in = qkv [B*N, 3 H 64] fp32.  SPLIT true: in = the row planes [B*N][3 H 64 / 8][2][8] f16, slot their scale.
// grid (ceil(N / 128), ceil(N / 32), B), 256 threads.  probs [B, H, N, N] and / or mean [B, N, N].
template <bool SPLIT>
__global__ __launch_bounds__(256, 3) void attn_probs_kernel(const void* __restrict__ in, const float* __restrict__ slot,
                                                         const float* __restrict__ lse, float* __restrict__ probs,
                                                         float* __restrict__ mean, int N, int H, float scale) {
  constexpr int QF = SPLIT ? TQ * HD : TQ * KS, KF = SPLIT ? TK * HD : TK * KS;      // floats of the staged Q / K rows
  static_assert(TQ * OS <= QF + KF, "the output tile lies over the operand tiles");
  __shared__ __attribute__((aligned(16))) float smem[QF + KF];
  float* Qs = smem;
  float* Ks = smem + QF;
  float* Os = smem;               // over the operands, once every wave has taken its fragments: 40 KB, three workgroups per CU
  const int D = H * HD;
  const int k0 = blockIdx.x * TK, q0 = blockIdx.y * TQ, b = blockIdx.z;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 31, kk = lane >> 5;
  const int q = q0 + j;
  const bool live = k0 + 32 * wave < N;       // wave-uniform: a wave whose keys all lie beyond N only helps to stage and store
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  // both layouts hold a row of qkv in 3 D 4 bytes, Q | K | V, head h 256 bytes into its section
  const int64_t ldbytes = (int64_t)3 * D * 4;
  const u8* qbase = static_cast<const u8*>(in) + (int64_t)b * N * ldbytes;
  const u8* kbase = qbase + (int64_t)D * 4;
  const float c1 = SPLIT ? scale * LOG2E * slot[EAV_SLOT_ISIGMA] * slot[EAV_SLOT_ISIGMA] : scale * LOG2E;
  const int krow = 32 * wave + (SPLIT ? pi_row(j) : j);
  u32x4 reg[NPIECE];
  fetch_pieces<SPLIT>(qbase, kbase, ldbytes, q0, k0, N, reg);
  for (int h = 0; h < H; ++h) {
    const int64_t bh = (int64_t)b * H + h;
    const float lq = q < N ? LOG2E * lse[bh * N + q] : 0.f;
    __syncthreads();                           // the previous head's fragment reads and tile stores are done
    commit_pieces<SPLIT>(Qs, Ks, reg);
    __syncthreads();
    if (h + 1 < H)                             // the next head's operands travel while this head is computed and stored
      fetch_pieces<SPLIT>(qbase + (h + 1) * 256, kbase + (h + 1) * 256, ldbytes, q0, k0, N, reg);
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
    if (live) {
      if constexpr (SPLIT) {
#pragma unroll
        for (int st = 0; st < 4; ++st) {       // S^T[key][q] = K-tile . Q^T, the three terms in the forward's order
          const f16x8 kh = frag_row(Ks, krow, st, kk, 0), kl = frag_row(Ks, krow, st, kk, 1);
          const f16x8 qh = frag_row(Qs, j, st, kk, 0), ql = frag_row(Qs, j, st, kk, 1);
          s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, qh, s, 0, 0, 0);
          s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl, qh, s, 0, 0, 0);
          s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, ql, s, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = ex2(fmaf(s[r], c1, -lq));
      } else {
        const float* kp = Ks + krow * KS + kk;
        const float* qp = Qs + j * KS + kk;
#pragma unroll
        for (int ks = 0; ks < HD / 2; ++ks)    // Q pre-multiplied by scale log2(e), as the forward and its backward stage it
          s = __builtin_amdgcn_mfma_f32_32x32x2f32(kp[2 * ks], c1 * qp[2 * ks], s, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = ex2(s[r] - lq);
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] += s[r];
    if (probs) {                               // (kernel-uniform)
      __syncthreads();                         // every wave has its fragments: the operand tiles give way to the output tile
#pragma unroll
      for (int r = 0; r < 16; ++r) Os[j * OS + 32 * wave + (SPLIT ? sp_row(r, kk) : kappa(r, kk))] = s[r];
      __syncthreads();
      store_tile(Os, probs + bh * N * N, q0, k0, N, wave, lane);
    }
  }
  if (mean) {
    const float invh = 1.f / (float)H;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) Os[j * OS + 32 * wave + (SPLIT ? sp_row(r, kk) : kappa(r, kk))] = acc[r] * invh;
    __syncthreads();
    store_tile(Os, mean + (int64_t)b * N * N, q0, k0, N, wave, lane);
  }
}

// r_out[b, r, k] = 0.5 sum_q r_in[b, r, q] abar[b, q, k] + 0.5 r_in[b, r, k]: one thread per output, q ascending (one fp32
// accumulator, fused multiply-adds: a fixed order); lanes run along k, so every read of abar is a contiguous row segment.
// grid (ceil(N / 256), R, B).
__global__ __launch_bounds__(256) void rollout_step_kernel(const float* __restrict__ r_in, const float* __restrict__ abar,
                                                           float* __restrict__ r_out, int R, int N) {
  const int k = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y, b = blockIdx.z;
  if (k >= N) return;
  const float* rin = r_in + ((int64_t)b * R + r) * N;
  const float* a = abar + (int64_t)b * N * N + k;
  float t = 0.f;
#pragma unroll 4
  for (int q = 0; q < N; ++q) t = fmaf(rin[q], a[(int64_t)q * N], t);
  r_out[((int64_t)b * R + r) * N + k] = 0.5f * t + 0.5f * rin[k];
}

template <bool SPLIT>
int attn_probs_launch(const void* in, const float* slot, const float* lse, float* probs, float* probs_mean, int B, int H,
                      int N, int head_dim, float scale, void* stream, const char* who) {
  EAV_REQUIRE(in && lse && (!SPLIT || slot) && B > 0 && H > 0 && N > 0, "%s: bad arguments", who);
  EAV_REQUIRE(probs || probs_mean, "%s: neither probs nor probs_mean given", who);
  EAV_REQUIRE(head_dim == HD, "%s: head_dim %d unsupported (needs %d)", who, head_dim, HD);
  EAV_REQUIRE(cdiv(N, TQ) <= 65535 && B <= 65535, "%s: grid too large (N %d, B %d)", who, N, B);
  hipLaunchKernelGGL(attn_probs_kernel<SPLIT>, dim3(cdiv(N, TK), cdiv(N, TQ), B), dim3(256), 0, (hipStream_t)stream, in,
                     slot, lse, probs, probs_mean, N, H, scale);
  EAV_CHECK_LAUNCH(who);
  return EAV_OK;
}

}  // namespace

extern "C" int eav_attn_probs(const float* qkv, const float* lse, float* probs, float* probs_mean, int B, int H, int N,
                              int head_dim, float scale, void* stream) {
  return attn_probs_launch<false>(qkv, nullptr, lse, probs, probs_mean, B, H, N, head_dim, scale, stream, "eav_attn_probs");
}

extern "C" int eav_attn_probs_sp(const void* rowp, const float* slot, const float* lse, float* probs, float* probs_mean,
                                 int B, int H, int N, int head_dim, float scale, void* stream) {
  return attn_probs_launch<true>(rowp, slot, lse, probs, probs_mean, B, H, N, head_dim, scale, stream, "eav_attn_probs_sp");
}

extern "C" int eav_rollout_step(const float* r_in, const float* abar, float* r_out, int B, int R, int N, void* stream) {
  EAV_REQUIRE(r_in && abar && r_out && r_in != r_out && B > 0 && R > 0 && N > 0, "eav_rollout_step: bad arguments");
  EAV_REQUIRE(R <= 65535 && B <= 65535, "eav_rollout_step: grid too large (R %d, B %d)", R, B);
  hipLaunchKernelGGL(rollout_step_kernel, dim3(cdiv(N, 256), R, B), dim3(256), 0, (hipStream_t)stream, r_in, abar, r_out, R,
                     N);
  EAV_CHECK_LAUNCH("eav_rollout_step");
  return EAV_OK;
}
