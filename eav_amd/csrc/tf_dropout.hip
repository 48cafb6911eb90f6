// Dropout of the AST / ViT encoders (HF hidden_dropout_prob / attention_probs_dropout_prob): the element-wise sites and
// the materialised-score attention path.  Every keep decision is eav_hash32(seed', element index) through dropout_mult
// (eav_common.h); seed' = site seed + 2 * (device-resident forward counter), so a captured step draws fresh masks on every
// replay and the backward regenerates the forward's mask instead of reading a stored one.  An explicit uint8 keep-mask
// (tests) replaces the generator element for element.  The fused head_dim-64 forms live in attention.hip.
//
//   eav_tf_dropout_mask      the keep-mask the generator would produce (tests: forward and backward agree on it)
//   eav_tf_dropout_add       out = resid + Dropout(y)   (emb, attn_out, mlp_out; resid NULL: the gate of their backward)
//   eav_softmax_dropout_fwd  softmax in place (P, kept for the Jacobian) and Pd = M o P / (1 - p) for the P.V product
//   eav_softmax_dropout_bwd  dS = P o (M o dP / (1 - p) - rowsum(...)) in place over dP; regenerates Pd for dV = Pd^T dO
#include "eav_common.h"
#include "../../include/eav_hip.h"

namespace {

inline int ew_blocks(int64_t n) { return (int)(cdiv64(n, 256) < 8192 ? cdiv64(n, 256) : 8192); }

__global__ __launch_bounds__(256) void dropout_mask_kernel(uint8_t* __restrict__ out, int64_t n, float drop_p,
                                                           uint64_t seed_in, const uint64_t* __restrict__ seed_dev) {
  const uint64_t seed = dropout_seed(seed_in, seed_dev);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    out[i] = dropout_mult(drop_p, seed, nullptr, (uint64_t)i) != 0.f ? 1 : 0;
}

// (y and out may be the same buffer: every element is read once and written once by the same thread)
__global__ __launch_bounds__(256) void dropout_add_kernel(const float* y, const float* __restrict__ resid, float* out,
                                                          int64_t n4, float drop_p, uint64_t seed_in,
                                                          const uint8_t* __restrict__ mask,
                                                          const uint64_t* __restrict__ seed_dev) {
  const uint64_t seed = dropout_seed(seed_in, seed_dev);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    float4 v = reinterpret_cast<const float4*>(y)[i];
    v.x *= dropout_mult(drop_p, seed, mask, 4 * (uint64_t)i);
    v.y *= dropout_mult(drop_p, seed, mask, 4 * (uint64_t)i + 1);
    v.z *= dropout_mult(drop_p, seed, mask, 4 * (uint64_t)i + 2);
    v.w *= dropout_mult(drop_p, seed, mask, 4 * (uint64_t)i + 3);
    if (resid) {
      const float4 r = reinterpret_cast<const float4*>(resid)[i];
      v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
    }
    reinterpret_cast<float4*>(out)[i] = v;
  }
}

// one wave per row, row held in registers (the arithmetic of softmax_fwd_kernel, tf_kernels.hip); element (row, c) of the
// [rows, N] probabilities draws with index row * N + c - the [B, H, N, N] tensor of HF's eager attention, flattened
template <int NPL>
__global__ __launch_bounds__(256) void softmax_dropout_fwd_kernel(float* __restrict__ s, float* __restrict__ pd,
                                                                  int64_t rows, int N, int ld, float drop_p,
                                                                  uint64_t seed_in, const uint8_t* __restrict__ mask,
                                                                  const uint64_t* __restrict__ seed_dev) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const uint64_t seed = dropout_seed(seed_in, seed_dev);
  float* p = s + row * ld;
  float* d = pd + row * ld;
  float v[NPL];
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < NPL; ++i) {
    const int c = lane + 64 * i;
    v[i] = c < N ? p[c] : -INFINITY;
    mx = fmaxf(mx, v[i]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < NPL; ++i) {
    v[i] = (lane + 64 * i) < N ? expf(v[i] - mx) : 0.f;
    sum += v[i];
  }
  const float inv = 1.0f / wave_sum(sum);
#pragma unroll
  for (int i = 0; i < NPL; ++i) {
    const int c = lane + 64 * i;
    if (c < N) {
      const float pr = v[i] * inv;
      p[c] = pr;
      d[c] = pr * dropout_mult(drop_p, seed, mask, (uint64_t)row * N + c);
    }
  }
}

template <int NPL>
__global__ __launch_bounds__(256) void softmax_dropout_bwd_kernel(const float* __restrict__ P, float* __restrict__ dP,
                                                                  float* __restrict__ pd, int64_t rows, int N, int ld,
                                                                  float drop_p, uint64_t seed_in,
                                                                  const uint8_t* __restrict__ mask,
                                                                  const uint64_t* __restrict__ seed_dev) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const uint64_t seed = dropout_seed(seed_in, seed_dev);
  const float* p = P + row * ld;
  float* d = dP + row * ld;
  float pv[NPL], dv[NPL];
  float dot = 0.f;
#pragma unroll
  for (int i = 0; i < NPL; ++i) {
    const int c = lane + 64 * i;
    pv[i] = c < N ? p[c] : 0.f;
    dv[i] = 0.f;
    if (c < N) {
      const float m = dropout_mult(drop_p, seed, mask, (uint64_t)row * N + c);
      dv[i] = d[c] * m;                      // dP = (dO V^T) o M / (1 - p)
      if (pd) pd[row * ld + c] = pv[i] * m;  // the forward's dropped probabilities, for dV
    }
    dot += pv[i] * dv[i];                    // = rowsum(dO o O) with the dropped O
  }
  dot = wave_sum(dot);
#pragma unroll
  for (int i = 0; i < NPL; ++i) {
    const int c = lane + 64 * i;
    if (c < N) d[c] = pv[i] * (dv[i] - dot);
  }
}

}  // namespace

#define EAV_DROP_ARGS_OK(p) ((p) >= 0.f && (p) < 1.f)

extern "C" int eav_tf_dropout_mask(uint8_t* mask, int64_t n, float drop_p, uint64_t seed, const uint64_t* seed_dev,
                                   void* stream) {
  EAV_REQUIRE(mask && n > 0 && EAV_DROP_ARGS_OK(drop_p), "eav_tf_dropout_mask: bad arguments");
  hipLaunchKernelGGL(dropout_mask_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, mask, n, drop_p, seed,
                     seed_dev);
  EAV_CHECK_LAUNCH("eav_tf_dropout_mask");
  return EAV_OK;
}

extern "C" int eav_tf_dropout_add(const float* y, const float* resid, float* out, int64_t n, float drop_p, uint64_t seed,
                                  const uint8_t* mask, const uint64_t* seed_dev, void* stream) {
  EAV_REQUIRE(y && out && n > 0 && (n & 3) == 0 && EAV_DROP_ARGS_OK(drop_p), "eav_tf_dropout_add: bad arguments");
  hipLaunchKernelGGL(dropout_add_kernel, dim3(ew_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, y, resid, out, n / 4,
                     drop_p, seed, mask, seed_dev);
  EAV_CHECK_LAUNCH("eav_tf_dropout_add");
  return EAV_OK;
}

extern "C" int eav_softmax_dropout_fwd(float* s, float* pd, int64_t rows, int N, int ld, float drop_p, uint64_t seed,
                                       const uint8_t* mask, const uint64_t* seed_dev, void* stream) {
  EAV_REQUIRE(s && pd && s != pd && rows > 0 && N > 0 && ld >= N && N <= 2048 && EAV_DROP_ARGS_OK(drop_p),
              "eav_softmax_dropout_fwd: need N <= 2048, 0 <= p < 1 and distinct buffers");
  const dim3 grid((unsigned)cdiv64(rows, 4));
  hipStream_t st = (hipStream_t)stream;
  if (N <= 256)
    hipLaunchKernelGGL(softmax_dropout_fwd_kernel<4>, grid, dim3(256), 0, st, s, pd, rows, N, ld, drop_p, seed, mask, seed_dev);
  else if (N <= 1280)
    hipLaunchKernelGGL(softmax_dropout_fwd_kernel<20>, grid, dim3(256), 0, st, s, pd, rows, N, ld, drop_p, seed, mask, seed_dev);
  else
    hipLaunchKernelGGL(softmax_dropout_fwd_kernel<32>, grid, dim3(256), 0, st, s, pd, rows, N, ld, drop_p, seed, mask, seed_dev);
  EAV_CHECK_LAUNCH("eav_softmax_dropout_fwd");
  return EAV_OK;
}

extern "C" int eav_softmax_dropout_bwd(const float* P, float* dP, float* pd, int64_t rows, int N, int ld, float drop_p,
                                       uint64_t seed, const uint8_t* mask, const uint64_t* seed_dev, void* stream) {
  EAV_REQUIRE(P && dP && P != dP && pd != dP && pd != P && rows > 0 && N > 0 && ld >= N && N <= 2048 &&
                  EAV_DROP_ARGS_OK(drop_p),
              "eav_softmax_dropout_bwd: need N <= 2048, 0 <= p < 1 and distinct buffers");
  const dim3 grid((unsigned)cdiv64(rows, 4));
  hipStream_t st = (hipStream_t)stream;
  if (N <= 256)
    hipLaunchKernelGGL(softmax_dropout_bwd_kernel<4>, grid, dim3(256), 0, st, P, dP, pd, rows, N, ld, drop_p, seed, mask, seed_dev);
  else if (N <= 1280)
    hipLaunchKernelGGL(softmax_dropout_bwd_kernel<20>, grid, dim3(256), 0, st, P, dP, pd, rows, N, ld, drop_p, seed, mask, seed_dev);
  else
    hipLaunchKernelGGL(softmax_dropout_bwd_kernel<32>, grid, dim3(256), 0, st, P, dP, pd, rows, N, ld, drop_p, seed, mask, seed_dev);
  EAV_CHECK_LAUNCH("eav_softmax_dropout_bwd");
  return EAV_OK;
}
