// An AST position table fitted to another number of time patches, and the exact adjoint of that fit.
//
// pos [nextra + ny*nx0, D] -> out [nextra + ny*nx, D]: the first nextra rows (cls, distillation) are copied; the patch rows,
// frequency-major (row nextra + f*nx + t), are out[f, t] = sum_a w[t][a] pos[f, idx[t][a]] with at most two taps per output
// time index, the same for every frequency row (eav_amd/pos_time.py builds the table: one tap of weight 1 for a centre cut,
// the two taps of a linear interpolation for a longer input, float64 rounded to fp32 once).  The frequency axis is untouched.
// D is innermost: one workgroup per output row, one float4 lane per thread.  The adjoint is a gather as well - one workgroup
// per SOURCE row walking the transposed (CSR) tap list of its time index in stored order - so it has no atomics, a fixed
// summation order, and writes every element of dpos (a source row no output reads gets zeros).  A few hundred KB of traffic
// per call: nothing here is tuned.
//
// A tap whose weight is zero is skipped and the first term is a plain product, so a cut copies bit for bit (-0 included) in
// both directions.  Table entries are clamped to their valid range before they index anything.
#include "eav_common.h"
#include "../../include/eav_hip.h"

namespace {

__device__ __forceinline__ float4 fma4(float w, const float4 a, const float4 acc) {
  return make_float4(__builtin_fmaf(w, a.x, acc.x), __builtin_fmaf(w, a.y, acc.y), __builtin_fmaf(w, a.z, acc.z),
                     __builtin_fmaf(w, a.w, acc.w));
}

__device__ __forceinline__ float4 mul4(float w, const float4 a) { return make_float4(w * a.x, w * a.y, w * a.z, w * a.w); }

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// grid: nextra + ny*nx rows; block: 64 .. 256 threads over the D/4 float4 lanes
__global__ void pos_time_fwd_kernel(const float* __restrict__ pos, float* __restrict__ out, int ny, int nx0, int nx, int D4,
                                    int nextra, const int* __restrict__ idx, const float* __restrict__ w) {
  const int row = blockIdx.x;
  const float4* src = reinterpret_cast<const float4*>(pos);
  float4* dst = reinterpret_cast<float4*>(out) + (int64_t)row * D4;
  if (row < nextra) {
    for (int d = threadIdx.x; d < D4; d += blockDim.x) dst[d] = src[(int64_t)row * D4 + d];
    return;
  }
  const int f = (row - nextra) / nx, t = (row - nextra) - f * nx;
  const int s0 = clampi(idx[2 * t], 0, nx0 - 1), s1 = clampi(idx[2 * t + 1], 0, nx0 - 1);
  const float c0 = w[2 * t], c1 = w[2 * t + 1];
  const float4* line = src + ((int64_t)nextra + (int64_t)f * nx0) * D4;
  for (int d = threadIdx.x; d < D4; d += blockDim.x) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    // (the first term is a plain product: 0 + w v would turn a -0 into +0)
    if (c0 != 0.f) acc = mul4(c0, line[(int64_t)s0 * D4 + d]);
    if (c1 != 0.f) {
      const float4 v = line[(int64_t)s1 * D4 + d];
      acc = (c0 != 0.f) ? fma4(c1, v, acc) : mul4(c1, v);
    }
    dst[d] = acc;
  }
}

// grid: nextra + ny*nx0 source rows.  ptr [nx0 + 1]: CSR row pointers of the transposed operator; oidx the output time
// indices, w the weights, nnz their length.
__global__ void pos_time_bwd_kernel(const float* __restrict__ dout, float* __restrict__ dpos, int ny, int nx0, int nx, int D4,
                                    int nextra, const int* __restrict__ ptr, const int* __restrict__ oidx,
                                    const float* __restrict__ w, int nnz) {
  const int row = blockIdx.x;
  const float4* src = reinterpret_cast<const float4*>(dout);
  float4* dst = reinterpret_cast<float4*>(dpos) + (int64_t)row * D4;
  if (row < nextra) {
    for (int d = threadIdx.x; d < D4; d += blockDim.x) dst[d] = src[(int64_t)row * D4 + d];
    return;
  }
  const int f = (row - nextra) / nx0, s = (row - nextra) - f * nx0;
  const int a0 = clampi(ptr[s], 0, nnz), a1 = clampi(ptr[s + 1], a0, nnz);
  const float4* line = src + ((int64_t)nextra + (int64_t)f * nx) * D4;
  for (int d = threadIdx.x; d < D4; d += blockDim.x) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    bool first = true;
    for (int a = a0; a < a1; ++a) {
      const float c = w[a];
      if (c == 0.f) continue;
      const float4 v = line[(int64_t)clampi(oidx[a], 0, nx - 1) * D4 + d];
      acc = first ? mul4(c, v) : fma4(c, v, acc);
      first = false;
    }
    dst[d] = acc;
  }
}

inline int lanes_block(int D4) { return D4 <= 64 ? 64 : (D4 <= 128 ? 128 : 256); }

inline bool geometry_ok(int ny, int nx0, int nx, int D, int nextra) {
  return ny >= 1 && nx0 >= 1 && nx >= 1 && ny <= 2048 && nx0 <= 2048 && nx <= 2048 && D > 0 && (D & 3) == 0 && nextra >= 0 &&
         nextra <= 2;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int eav_pos_time_fwd(const float* pos, float* out, int ny, int nx0, int nx, int D, int nextra, const int* idx,
                                const float* w, void* stream) {
  EAV_REQUIRE(pos && out && pos != out && idx && w && geometry_ok(ny, nx0, nx, D, nextra) && aligned16(pos) && aligned16(out),
              "eav_pos_time_fwd: need ny, nx0, nx in 1 .. 2048, D %% 4 == 0, nextra <= 2, 16-byte aligned distinct pos / out "
              "and the two tap tables");
  const int rows = nextra + ny * nx;
  hipLaunchKernelGGL(pos_time_fwd_kernel, dim3(rows), dim3(lanes_block(D / 4)), 0, (hipStream_t)stream, pos, out, ny, nx0, nx,
                     D / 4, nextra, idx, w);
  EAV_CHECK_LAUNCH("eav_pos_time_fwd");
  return EAV_OK;
}

extern "C" int eav_pos_time_bwd(const float* dout, float* dpos, int ny, int nx0, int nx, int D, int nextra, const int* ptr,
                                const int* oidx, const float* w, int nnz, void* stream) {
  EAV_REQUIRE(dout && dpos && dout != dpos && ptr && oidx && w && nnz >= 0 && nnz <= 2 * 2048 &&
                  geometry_ok(ny, nx0, nx, D, nextra) && aligned16(dout) && aligned16(dpos),
              "eav_pos_time_bwd: need ny, nx0, nx in 1 .. 2048, D %% 4 == 0, nextra <= 2, 16-byte aligned distinct dout / "
              "dpos and the transposed tap list (at most 2 taps per output)");
  const int rows = nextra + ny * nx0;
  hipLaunchKernelGGL(pos_time_bwd_kernel, dim3(rows), dim3(lanes_block(D / 4)), 0, (hipStream_t)stream, dout, dpos, ny, nx0,
                     nx, D / 4, nextra, ptr, oidx, w, nnz);
  EAV_CHECK_LAUNCH("eav_pos_time_bwd");
  return EAV_OK;
}
