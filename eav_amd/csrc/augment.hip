// Batch assembly with input augmentation: the gather of eav_gather_rows with mixup, a horizontal flip and up to two
// row bands and two column bands of SpecAugment-style masking applied on the way, and the mixed soft targets with it.
//
// A sample of the device-resident split x [N, R, C] is a matrix of R rows of C contiguous columns: an AST clip is
// [time, mel], a ViT frame [3, H, W] is viewed as [3 H, W].  Output sample b is described by record b of `table`,
// EAV_AUGMENT_RECORD_INTS int32 words:
//   0 i      source sample           4,5   [r0, r1) first row band        8,9    [c0, c1) first column band
//   1 j      partner sample          6,7   [r0, r1) second row band       10,11  [c0, c1) second column band
//   2 lambda (the bits of an fp32)   3     flip (non-zero: columns reversed)
//   out[b, r, c] = fill inside any band, else lambda x[i, r, c'] + (1 - lambda) x[j, r, c'],  c' = flip ? C - 1 - c : c
// lambda == 1 never reads the partner and hands the source's bits through, so a record (i, *, 1.0, 0, empty bands) is
// eav_gather_rows.  A band is a pair of comparisons: empty (r0 >= r1), full-range, overlapping and out-of-range bands are
// all legal.  i and j are trusted like the indices of eav_gather_rows.
//   tout[b, :] (optional) = lambda onehot(y[i]) + (1 - lambda) onehot(y[j]), 1 where the two labels coincide; a label
//   outside [0, NC) contributes nothing.
//
// Bandwidth-bound: one 16-byte access per thread and trip where C % 4 == 0 (a flip reverses the order of the vectors of a
// row and the four floats inside each), a scalar path otherwise; the grid is sized by the elements - every sample gets as
// many blocks as its elements ask for (up to 256, then the threads stride), so a few large samples spread over the machine
// like many small ones - and a block serves one sample, whose record it reads through scalar loads.  No atomics.
#include "eav_common.h"
#include "../../include/eav_hip.h"

namespace {

constexpr int REC = EAV_AUGMENT_RECORD_INTS;

struct AugRecord {
  int64_t i, j;
  float lam;
  bool flip;
  int r0a, r1a, r0b, r1b, c0a, c1a, c0b, c1b;
};

__device__ __forceinline__ AugRecord load_record(const int32_t* __restrict__ table, int b) {
  const int32_t* q = table + (int64_t)b * REC;
  AugRecord a;
  a.i = q[0]; a.j = q[1];
  a.lam = __int_as_float(q[2]);
  a.flip = q[3] != 0;
  a.r0a = q[4]; a.r1a = q[5]; a.r0b = q[6]; a.r1b = q[7];
  a.c0a = q[8]; a.c1a = q[9]; a.c0b = q[10]; a.c1b = q[11];
  return a;
}

__device__ __forceinline__ bool row_masked(const AugRecord& a, int r) {
  return (r >= a.r0a && r < a.r1a) || (r >= a.r0b && r < a.r1b);
}
__device__ __forceinline__ bool col_masked(const AugRecord& a, int c) {
  return (c >= a.c0a && c < a.c1a) || (c >= a.c0b && c < a.c1b);
}

__device__ __forceinline__ float mix(float lam, float a, float b) {
#pragma clang fp contract(off)
  return lam * a + (1.f - lam) * b;
}

// One unit = VEC consecutive columns of one row of an output sample; unit e of a sample is row e / cw, columns
// VEC (e % cw) ... with cw = C / VEC units per row.  blockIdx.y is the sample - its record is uniform over the block -
// and the blocks of a sample stride over its R cw units.
template <int VEC>
__global__ __launch_bounds__(256) void augment_gather_kernel(const float* __restrict__ x, const int64_t* __restrict__ y,
                                                             const int32_t* __restrict__ table, float fill,
                                                             float* __restrict__ out, float* __restrict__ tout, int B,
                                                             int R, int C, int NC) {
  const int cw = C / VEC, per = R * cw, b = blockIdx.y;
  const int64_t sample = (int64_t)R * C;
  const AugRecord a = load_record(table, b);       // the same for the whole block: scalar loads
  const int stride = gridDim.x * 256, first = blockIdx.x * 256 + threadIdx.x;
  for (int64_t e64 = first; e64 < per; e64 += stride) {
    const int e = (int)e64, r = e / cw, c0 = (e - r * cw) * VEC;
    float* o = out + (int64_t)b * sample + (int64_t)r * C + c0;
    bool m[VEC];
    bool all = row_masked(a, r);
    if (!all) {
      all = true;
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        m[k] = col_masked(a, c0 + k);
        all = all && m[k];
      }
    } else {
#pragma unroll
      for (int k = 0; k < VEC; ++k) m[k] = true;
    }
    float v[VEC];
    if (all) {                // nothing of the sources shows: they are not read
#pragma unroll
      for (int k = 0; k < VEC; ++k) v[k] = fill;
    } else {
      // the source columns of c0 .. c0 + VEC - 1: the same vector, or the mirrored one read backwards
      const int s0 = a.flip ? C - VEC - c0 : c0;
      const float* pa = x + a.i * sample + (int64_t)r * C + s0;
      float va[VEC], vb[VEC];
      if constexpr (VEC == 4) {
        const float4 q = *reinterpret_cast<const float4*>(pa);
        va[0] = q.x; va[1] = q.y; va[2] = q.z; va[3] = q.w;
      } else {
        va[0] = pa[0];
      }
      if (a.lam != 1.f) {
        const float* pb = x + a.j * sample + (int64_t)r * C + s0;
        if constexpr (VEC == 4) {
          const float4 q = *reinterpret_cast<const float4*>(pb);
          vb[0] = q.x; vb[1] = q.y; vb[2] = q.z; vb[3] = q.w;
        } else {
          vb[0] = pb[0];
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) va[k] = mix(a.lam, va[k], vb[k]);
      }
#pragma unroll
      for (int k = 0; k < VEC; ++k) v[k] = m[k] ? fill : va[a.flip ? VEC - 1 - k : k];
    }
    if constexpr (VEC == 4) *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
    else o[0] = v[0];
  }
  if (tout && blockIdx.x == 0) {       // the sample's row of soft targets: its first block
    const int64_t yi = y[a.i], yj = y[a.j];
    for (int c = threadIdx.x; c < NC; c += 256) {
      float v = 0.f;
      if (yi == c) v = (yj == c) ? 1.f : a.lam;
      else if (yj == c) v = 1.f - a.lam;
      tout[(int64_t)b * NC + c] = v;
    }
  }
}

}  // namespace

extern "C" int eav_augment_gather(const float* x, const int64_t* y, const int32_t* table, float fill, float* out,
                                  float* tout, int B, int R, int C, int NC, void* stream) {
  EAV_REQUIRE(x && table && out && B > 0 && R > 0 && C > 0 && (int64_t)R * C < (1ll << 31), "eav_augment_gather: bad arguments");
  EAV_REQUIRE(!tout || (y && NC > 0 && (int64_t)B * NC < (1ll << 31)),
              "eav_augment_gather: soft targets need the labels and a class count");
  const bool vec = (C % 4 == 0) && ((((uintptr_t)x | (uintptr_t)out) & 15) == 0);
  // blocks per sample from its element count, up to 256 (beyond, a thread strides): 8 AST clips of [1024, 128] are 1024
  // blocks, a sample of a few elements is one
  const int64_t units = (int64_t)R * (vec ? C / 4 : C);
  const int gx = (int)(cdiv64(units, 256) > 256 ? 256 : cdiv64(units, 256));
  EAV_REQUIRE(B <= 65535, "eav_augment_gather: at most 65535 samples per batch");
  if (vec)
    hipLaunchKernelGGL(augment_gather_kernel<4>, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, x, y, table, fill, out, tout,
                       B, R, C, NC);
  else
    hipLaunchKernelGGL(augment_gather_kernel<1>, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, x, y, table, fill, out, tout,
                       B, R, C, NC);
  EAV_CHECK_LAUNCH("eav_augment_gather");
  return EAV_OK;
}
