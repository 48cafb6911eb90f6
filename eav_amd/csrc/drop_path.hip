// Stochastic depth of the AST / ViT encoders (timm.layers.DropPath, scale_by_keep): in training mode every sample drops the
// whole residual branch of a layer with probability p_i = rate * i / (L - 1), the kept ones are scaled by 1 / (1 - p_i).  Two
// kernels, both in gather form - every output element is written by the one thread that owns it, no atomics, the same bits
// on every run - and usable inside a captured step (nothing is read back, the randomness comes from the device-resident
// forward counter as in tf_dropout.hip).
//
//   eav_drop_path_plan   the scale table [L, 2, B] of a forward (row 2 i: the attention branch of layer i, row 2 i + 1 its MLP
//                        branch): 0 or 1 / (1 - p_i) per sample, from the hash or from an explicit uint8 keep table (tests)
//   eav_drop_path_add    out[b, :] = resid[b, :] + y[b, :] * scale_row[b]   (resid NULL: the gate of the backward)
//
// The product is rounded before the sum (no fma contraction): the result is numpy's float32 resid + y * s bit for bit, a
// dropped sample leaves resid itself (y finite), NaN / Inf in a dropped y give NaN as x * 0 does in torch.
#include "eav_common.h"
#include "../../include/eav_hip.h"

namespace {

inline int ew_blocks(int64_t n) { return (int)(cdiv64(n, 256) < 8192 ? cdiv64(n, 256) : 8192); }

// Row r = 2 i + branch draws with the seed of site id (first id + r): seed + (r << 40) (encoder_dropout.site_seed), sample b
// with element index b - dropout_keep of eav_common.h.  p_i is formed in double and rounded once.
__global__ __launch_bounds__(256) void drop_path_plan_kernel(float* __restrict__ scale, int L, int B, double rate,
                                                             uint64_t seed_in, const uint64_t* __restrict__ seed_dev,
                                                             const uint8_t* __restrict__ keep) {
  const int64_t total = (int64_t)2 * L * B;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int b = (int)(idx % B), r = (int)(idx / B);
    const int i = r >> 1;
    const float p = L > 1 ? (float)(rate * (double)i / (double)(L - 1)) : 0.f;
    float s = 1.f;
    if (p > 0.f) {
      const uint64_t seed = dropout_seed(seed_in + ((uint64_t)r << 40), seed_dev);
      const bool kept = keep ? (keep[idx] != 0) : dropout_keep(p, seed, nullptr, (uint64_t)b);
      s = kept ? dropout_scale(p) : 0.f;
    }
    scale[idx] = s;
  }
}

// (y and out may be the same buffer: every element is read once and written once by the same thread.  A float4 never
// straddles two samples: per_sample % 4 == 0.)
__global__ __launch_bounds__(256) void drop_path_add_kernel(const float* y, const float* __restrict__ resid, float* out,
                                                            const float* __restrict__ scale_row, int64_t n4, int64_t per4) {
#pragma clang fp contract(off)
  const bool narrow = n4 <= 0x7fffffff;          // (a 32-bit division where the index allows)
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const int64_t b = narrow ? (int64_t)((uint32_t)i / (uint32_t)per4) : i / per4;
    const float s = scale_row[b];
    float4 v = reinterpret_cast<const float4*>(y)[i];
    v.x = v.x * s; v.y = v.y * s; v.z = v.z * s; v.w = v.w * s;
    if (resid) {
      const float4 r = reinterpret_cast<const float4*>(resid)[i];
      v.x = r.x + v.x; v.y = r.y + v.y; v.z = r.z + v.z; v.w = r.w + v.w;
    }
    reinterpret_cast<float4*>(out)[i] = v;
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int eav_drop_path_plan(float* scale, int L, int B, double rate, uint64_t seed, const uint64_t* counter,
                                  const uint8_t* keep, void* stream) {
  EAV_REQUIRE(scale && L > 0 && B > 0 && rate >= 0.0 && rate < 1.0, "eav_drop_path_plan: need L, B > 0 and 0 <= rate < 1");
  hipLaunchKernelGGL(drop_path_plan_kernel, dim3(ew_blocks((int64_t)2 * L * B)), dim3(256), 0, (hipStream_t)stream, scale,
                     L, B, rate, seed, counter, keep);
  EAV_CHECK_LAUNCH("eav_drop_path_plan");
  return EAV_OK;
}

extern "C" int eav_drop_path_add(const float* y, const float* resid, float* out, const float* scale_row, int B,
                                 int64_t per_sample, void* stream) {
  EAV_REQUIRE(y && out && scale_row && B > 0 && per_sample > 0 && (per_sample & 3) == 0 && resid != out,
              "eav_drop_path_add: need B > 0, per_sample a positive multiple of 4 and resid apart from out");
  EAV_REQUIRE(aligned16(y) && aligned16(resid) && aligned16(out), "eav_drop_path_add: pointers must be 16-byte aligned");
  const int64_t n4 = (int64_t)B * (per_sample / 4);
  hipLaunchKernelGGL(drop_path_add_kernel, dim3(ew_blocks(n4)), dim3(256), 0, (hipStream_t)stream, y, resid, out, scale_row,
                     n4, per_sample / 4);
  EAV_CHECK_LAUNCH("eav_drop_path_add");
  return EAV_OK;
}
