// Patch dropout of the AST / ViT encoders (timm.layers.PatchDropout, Liu et al. 2022): in training mode every sample keeps a
// random subset of K of its P patch tokens; the readout tokens are always kept.  The dropped patches leave before the
// projection: their im2col rows are never formed.  Five kernels, all in gather form - every output element is written by
// the one thread that owns it, no atomics, the same bits on every run - and all usable inside a captured step (nothing is
// read back, the plan's randomness comes from a device-resident counter as in tf_dropout.hip).
//
//   eav_patch_keep_plan      keep [B, K] / inv [B, P] of a forward: the K smallest of the total order (key, p) per sample,
//                            key = eav_hash32(seed + 2 counter, b P + p) or an explicit uint32 array (tests plant ties)
//   eav_patch_keep_invert    inv from an explicit keep (Encoder.set_patch_keep)
//   eav_im2col_keep          the rows eav_im2col forms for the kept patches, [B K, C patch patch]
//   eav_embed_finish_keep    eav_embed_finish with the position row of slot s taken from pos[nextra + keep[b][s]]
//   eav_embed_bwd_keep       demb rows of the kept patches and the full-grid position gradient (+0.0 where nobody kept)
//
// The plan ranks by counting: a sample's P <= 2046 composite keys (key << 32 | p, unique because p is) sit in 16 KB of LDS,
// every thread owns two of them and counts how many of the P are smaller - P broadcast reads per thread, no data-dependent
// control flow and no exchange network whose stage count depends on padding P to a power of two.  rank < K is the kept
// set; a block-wide exclusive scan of the kept flags gives each kept patch its slot, which is what makes keep[b] ascending.
#include "eav_common.h"
#include "../../include/eav_hip.h"

namespace {

constexpr int PLAN_THREADS = 1024;                 // two patches per thread
constexpr int PLAN_MAX_P = 2 * PLAN_THREADS;       // >= EAV_MAX_TOKENS - 1

// blocks of a grid-stride loop over n elements (every caller has n > 0)
inline int grid_for(int64_t n) { return (int)(cdiv64(n, 256) < 8192 ? cdiv64(n, 256) : 8192); }

__global__ __launch_bounds__(PLAN_THREADS) void patch_keep_plan_kernel(int* __restrict__ keep, int* __restrict__ inv, int P,
                                                                       int K, uint64_t seed_in,
                                                                       const uint64_t* __restrict__ seed_dev,
                                                                       const uint32_t* __restrict__ keys) {
  __shared__ uint64_t comp[PLAN_MAX_P];
  __shared__ int wave_tot[PLAN_THREADS / 64];
  const int b = blockIdx.x, t = threadIdx.x;
  const uint64_t seed = dropout_seed(seed_in, seed_dev);
  const int p0 = 2 * t, p1 = 2 * t + 1;
  uint64_t mine[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int p = p0 + e;
    uint64_t c = ~0ull;
    if (p < P) {
      const uint64_t i = (uint64_t)b * P + p;
      const uint32_t key = keys ? keys[i] : eav_hash32(seed, i);
      c = ((uint64_t)key << 32) | (uint32_t)p;
    }
    mine[e] = c;
    comp[p] = c;
  }
  __syncthreads();
  int r0 = 0, r1 = 0;
#pragma unroll 4
  for (int q = 0; q < P; ++q) {
    const uint64_t c = comp[q];
    r0 += c < mine[0];
    r1 += c < mine[1];
  }
  const int f0 = (p0 < P && r0 < K) ? 1 : 0, f1 = (p1 < P && r1 < K) ? 1 : 0;
  // exclusive scan of the flags in patch order: in-wave inclusive scan, then the totals of the waves before this one
  const int lane = t & 63, wave = t >> 6;
  const int c = f0 + f1;
  int incl = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  if (lane == 63) wave_tot[wave] = incl;
  __syncthreads();
  int excl = incl - c;
  for (int w = 0; w < wave; ++w) excl += wave_tot[w];
  int* kb = keep + (int64_t)b * K;
  int* ib = inv + (int64_t)b * P;
  if (p0 < P) {
    if (f0 && excl < K) kb[excl] = p0;
    ib[p0] = f0 ? excl : -1;
  }
  if (p1 < P) {
    if (f1 && excl + f0 < K) kb[excl + f0] = p1;
    ib[p1] = f1 ? excl + f0 : -1;
  }
}

// inv[b][p] = the slot s with keep[b][s] == p, -1 when there is none: a binary search of the ascending row per element
__global__ __launch_bounds__(256) void patch_keep_invert_kernel(const int* __restrict__ keep, int* __restrict__ inv, int B,
                                                                int P, int K) {
  const int64_t total = (int64_t)B * P;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int p = (int)(idx % P), b = (int)(idx / P);
    const int* kb = keep + (int64_t)b * K;
    int lo = 0, hi = K;                            // first slot whose patch is >= p
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (kb[mid] < p) lo = mid + 1; else hi = mid;
    }
    inv[idx] = (lo < K && kb[lo] == p) ? lo : -1;
  }
}

// im2col_kernel (tf_kernels.hip) over the kept rows: row b K + s is the row of patch keep[b][s] of image b
__global__ __launch_bounds__(256) void im2col_keep_kernel(const float* __restrict__ x, float* __restrict__ col,
                                                          const int* __restrict__ keep, int B, int C, int H, int W, int P,
                                                          int sy, int sx, int ny, int nx, int transposed, int K) {
  const int KP = C * P * P;
  const int64_t total = (int64_t)B * K * KP;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += stride) {
    const int k = (int)(idx % KP);
    const int64_t r = idx / KP;
    const int b = (int)(r / K);
    const int patch = keep[r];
    float v = 0.f;
    if ((unsigned)patch < (unsigned)(ny * nx)) {   // (a table outside the grid reads nothing)
      const int px = patch % nx, py = patch / nx;
      const int j = k % P, i = (k / P) % P, c = k / (P * P);
      const int h = py * sy + i, w = px * sx + j;
      const int64_t src = transposed ? ((int64_t)b * C + c) * H * W + (int64_t)w * H + h
                                     : (((int64_t)b * C + c) * H + h) * W + w;
      v = x[src];
    }
    col[idx] = v;
  }
}

// h[b,t,:] = (t < nextra ? tokens[t,:] + pos[t,:] : h[b,t,:] + pos[nextra + keep[b][t - nextra],:])
__global__ __launch_bounds__(256) void embed_finish_keep_kernel(float* __restrict__ h, const float* __restrict__ cls,
                                                                const float* __restrict__ dist,
                                                                const float* __restrict__ pos,
                                                                const int* __restrict__ keep, int B, int K, int D,
                                                                int nextra) {
  const int ntok = nextra + K, D4 = D >> 2;
  const int64_t total = (int64_t)B * ntok * D4;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += stride) {
    const int q = (int)(idx % D4);
    const int64_t row = idx / D4;
    const int t = (int)(row % ntok), b = (int)(row / ntok);
    float4 v;
    int prow = t;
    if (t < nextra) {
      v = reinterpret_cast<const float4*>(t == 0 ? cls : dist)[q];
    } else {
      v = reinterpret_cast<float4*>(h)[idx];
      prow = nextra + keep[(int64_t)b * K + (t - nextra)];
    }
    const float4 p = reinterpret_cast<const float4*>(pos)[(int64_t)prow * D4 + q];
    reinterpret_cast<float4*>(h)[idx] = make_float4(v.x + p.x, v.y + p.y, v.z + p.z, v.w + p.w);
  }
}

// dpos[r,:] (r < nextra) = sum_b dh[b,r,:];  dpos[nextra + p,:] = sum over the samples that kept p, ascending b, of
// dh[b, nextra + inv[b][p], :] (+0.0 when nobody did);  demb[b K + s,:] = dh[b, nextra + s, :]
__global__ __launch_bounds__(256) void embed_bwd_keep_kernel(const float* __restrict__ dh, float* __restrict__ dpos,
                                                             float* __restrict__ demb, const int* __restrict__ inv, int B,
                                                             int P, int K, int D, int nextra) {
  const int ntok = nextra + K, D4 = D >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t total_pos = (int64_t)(nextra + P) * D4;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total_pos; idx += stride) {
    const int q = (int)(idx % D4), r = (int)(idx / D4);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int b = 0; b < B; ++b) {
      int t = r;
      if (r >= nextra) {
        const int slot = inv[(int64_t)b * P + (r - nextra)];
        if ((unsigned)slot >= (unsigned)K) continue;
        t = nextra + slot;
      }
      const float4 v = reinterpret_cast<const float4*>(dh)[((int64_t)b * ntok + t) * D4 + q];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    reinterpret_cast<float4*>(dpos)[idx] = s;
  }
  const int64_t total_emb = (int64_t)B * K * D4;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total_emb; idx += stride) {
    const int q = (int)(idx % D4);
    const int64_t row = idx / D4;
    const int s = (int)(row % K), b = (int)(row / K);
    reinterpret_cast<float4*>(demb)[idx] = reinterpret_cast<const float4*>(dh)[((int64_t)b * ntok + nextra + s) * D4 + q];
  }
}

}  // namespace

#define EAV_KEEP_DIMS_OK(B, P, K) ((B) > 0 && (K) >= 1 && (K) <= (P) && (P) <= EAV_MAX_TOKENS - 1)

extern "C" int eav_patch_keep_plan(int* keep, int* inv, int B, int P, int K, uint64_t seed, const uint64_t* counter,
                                   const uint32_t* keys, void* stream) {
  static_assert(PLAN_MAX_P >= EAV_MAX_TOKENS - 1, "a sample's keys must fit the plan kernel's LDS array");
  EAV_REQUIRE(keep && inv && EAV_KEEP_DIMS_OK(B, P, K), "eav_patch_keep_plan: need 1 <= K <= P <= EAV_MAX_TOKENS - 1");
  hipLaunchKernelGGL(patch_keep_plan_kernel, dim3(B), dim3(PLAN_THREADS), 0, (hipStream_t)stream, keep, inv, P, K, seed,
                     counter, keys);
  EAV_CHECK_LAUNCH("eav_patch_keep_plan");
  return EAV_OK;
}

extern "C" int eav_patch_keep_invert(const int* keep, int* inv, int B, int P, int K, void* stream) {
  EAV_REQUIRE(keep && inv && EAV_KEEP_DIMS_OK(B, P, K), "eav_patch_keep_invert: need 1 <= K <= P <= EAV_MAX_TOKENS - 1");
  hipLaunchKernelGGL(patch_keep_invert_kernel, dim3(grid_for((int64_t)B * P)), dim3(256), 0, (hipStream_t)stream, keep,
                     inv, B, P, K);
  EAV_CHECK_LAUNCH("eav_patch_keep_invert");
  return EAV_OK;
}

extern "C" int eav_im2col_keep(const float* x, float* col, const int* keep, int B, int C, int H, int W, int P, int sy,
                               int sx, int transposed, int K, void* stream) {
  EAV_REQUIRE(x && col && keep && B > 0 && C > 0 && P > 0 && H >= P && W >= P && sy > 0 && sx > 0,
              "eav_im2col_keep: bad arguments");
  const int ny = (H - P) / sy + 1, nx = (W - P) / sx + 1;
  EAV_REQUIRE((int64_t)ny * nx <= EAV_MAX_TOKENS - 1 && K >= 1 && K <= ny * nx,
              "eav_im2col_keep: need 1 <= K <= patches of the grid <= EAV_MAX_TOKENS - 1");
  hipLaunchKernelGGL(im2col_keep_kernel, dim3(grid_for((int64_t)B * K * C * P * P)), dim3(256), 0, (hipStream_t)stream, x,
                     col, keep, B, C, H, W, P, sy, sx, ny, nx, transposed, K);
  EAV_CHECK_LAUNCH("eav_im2col_keep");
  return EAV_OK;
}

extern "C" int eav_embed_finish_keep(float* h, const float* cls, const float* dist, const float* pos, const int* keep,
                                     int B, int K, int D, int nextra, void* stream) {
  EAV_REQUIRE(h && cls && pos && keep && B > 0 && K >= 1 && K <= EAV_MAX_TOKENS - nextra && D > 0 && (D & 3) == 0 &&
                  nextra >= 1 && nextra <= 2 && (nextra == 1 || dist), "eav_embed_finish_keep: bad arguments");
  hipLaunchKernelGGL(embed_finish_keep_kernel, dim3(grid_for((int64_t)B * (nextra + K) * D / 4)), dim3(256), 0,
                     (hipStream_t)stream, h, cls, dist, pos, keep, B, K, D, nextra);
  EAV_CHECK_LAUNCH("eav_embed_finish_keep");
  return EAV_OK;
}

extern "C" int eav_embed_bwd_keep(const float* dh, float* dpos, float* demb, const int* inv, int B, int P, int K, int D,
                                  int nextra, void* stream) {
  EAV_REQUIRE(dh && dpos && demb && inv && EAV_KEEP_DIMS_OK(B, P, K) && D > 0 && (D & 3) == 0 && nextra >= 1 &&
                  nextra <= 2 && P <= EAV_MAX_TOKENS - nextra, "eav_embed_bwd_keep: bad arguments");
  const int64_t n = (int64_t)(nextra + P) * D / 4, m = (int64_t)B * K * D / 4;
  hipLaunchKernelGGL(embed_bwd_keep_kernel, dim3(grid_for(n > m ? n : m)), dim3(256), 0, (hipStream_t)stream, dh, dpos,
                     demb, inv, B, P, K, D, nextra);
  EAV_CHECK_LAUNCH("eav_embed_bwd_keep");
  return EAV_OK;
}
