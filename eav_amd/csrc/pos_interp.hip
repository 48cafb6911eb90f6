// Bicubic resampling of a ViT position table (HF ViTEmbeddings.interpolate_pos_encoding: F.interpolate(mode="bicubic",
// align_corners=False), no antialiasing) and its exact adjoint.
//
// pos [nextra + g*g, D] -> out [nextra + ny*nx, D]: the first nextra rows (cls) are copied, the patch rows are
// out = (Wy (x) Wx) pos with the separable 4-tap operator of the host tables (eav_amd/pos_interp.py: float64, border taps
// folded onto their clamped source index, rounded to fp32 once).  D is innermost: one workgroup per output row, one float4
// lane per thread.  The adjoint is a gather as well - one workgroup per SOURCE row walking the per-axis transposed (CSR) tap
// lists in their stored order - so it has no atomics, a fixed summation order, and writes every element of dpos (a source
// row no output reads gets zeros).  A few hundred KB of traffic per call: nothing here is tuned.
//
// A tap whose weight is zero is skipped, so an identity resampling (n_out == n_in: weights 0, 1, 0, 0) copies bit for bit.
// Table entries are clamped to their valid range before they index anything.
#include "eav_common.h"
#include "../../include/eav_hip.h"

namespace {

__device__ __forceinline__ float4 fma4(float w, const float4 a, const float4 acc) {
  return make_float4(__builtin_fmaf(w, a.x, acc.x), __builtin_fmaf(w, a.y, acc.y), __builtin_fmaf(w, a.z, acc.z),
                     __builtin_fmaf(w, a.w, acc.w));
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// grid: nextra + ny*nx rows; block: 64 .. 256 threads over the D/4 float4 lanes
__global__ void pos_bicubic_fwd_kernel(const float* __restrict__ pos, float* __restrict__ out, int g, int ny, int nx, int D4,
                                       int nextra, const int* __restrict__ iy, const float* __restrict__ wy,
                                       const int* __restrict__ ix, const float* __restrict__ wx) {
  const int row = blockIdx.x;
  const float4* src = reinterpret_cast<const float4*>(pos);
  float4* dst = reinterpret_cast<float4*>(out) + (int64_t)row * D4;
  if (row < nextra) {
    for (int d = threadIdx.x; d < D4; d += blockDim.x) dst[d] = src[(int64_t)row * D4 + d];
    return;
  }
  const int oy = (row - nextra) / nx, ox = (row - nextra) - oy * nx;
  int sy[4], sx[4];
  float cy[4], cx[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    sy[a] = clampi(iy[4 * oy + a], 0, g - 1);
    cy[a] = wy[4 * oy + a];
    sx[a] = clampi(ix[4 * ox + a], 0, g - 1);
    cx[a] = wx[4 * ox + a];
  }
  for (int d = threadIdx.x; d < D4; d += blockDim.x) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    bool first_row = true;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      if (cy[a] == 0.f) continue;
      const float4* line = src + ((int64_t)nextra + (int64_t)sy[a] * g) * D4 + d;
      float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
      bool first = true;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        if (cx[b] == 0.f) continue;
        const float4 v = line[(int64_t)sx[b] * D4];
        // (the first term is a plain product: 0 + w v would turn a -0 into +0)
        r = first ? make_float4(cx[b] * v.x, cx[b] * v.y, cx[b] * v.z, cx[b] * v.w) : fma4(cx[b], v, r);
        first = false;
      }
      acc = first_row ? make_float4(cy[a] * r.x, cy[a] * r.y, cy[a] * r.z, cy[a] * r.w) : fma4(cy[a], r, acc);
      first_row = false;
    }
    dst[d] = acc;
  }
}

// grid: nextra + g*g source rows.  ypt / xpt [g + 1]: CSR row pointers of the transposed per-axis operators; yidx / xidx the
// output indices, yw / xw the weights, nnzy / nnzx their lengths.
__global__ void pos_bicubic_bwd_kernel(const float* __restrict__ dout, float* __restrict__ dpos, int g, int ny, int nx,
                                       int D4, int nextra, const int* __restrict__ ypt, const int* __restrict__ yidx,
                                       const float* __restrict__ yw, int nnzy, const int* __restrict__ xpt,
                                       const int* __restrict__ xidx, const float* __restrict__ xw, int nnzx) {
  const int row = blockIdx.x;
  const float4* src = reinterpret_cast<const float4*>(dout);
  float4* dst = reinterpret_cast<float4*>(dpos) + (int64_t)row * D4;
  if (row < nextra) {
    for (int d = threadIdx.x; d < D4; d += blockDim.x) dst[d] = src[(int64_t)row * D4 + d];
    return;
  }
  const int py = (row - nextra) / g, px = (row - nextra) - py * g;
  const int y0 = clampi(ypt[py], 0, nnzy), y1 = clampi(ypt[py + 1], y0, nnzy);
  const int x0 = clampi(xpt[px], 0, nnzx), x1 = clampi(xpt[px + 1], x0, nnzx);
  for (int d = threadIdx.x; d < D4; d += blockDim.x) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int a = y0; a < y1; ++a) {
      const int oy = clampi(yidx[a], 0, ny - 1);
      const float cy = yw[a];
      const float4* line = src + ((int64_t)nextra + (int64_t)oy * nx) * D4 + d;
      float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int b = x0; b < x1; ++b) {
        const float4 v = line[(int64_t)clampi(xidx[b], 0, nx - 1) * D4];
        const float cx = xw[b];
        r = (b == x0) ? make_float4(cx * v.x, cx * v.y, cx * v.z, cx * v.w) : fma4(cx, v, r);
      }
      acc = (a == y0) ? make_float4(cy * r.x, cy * r.y, cy * r.z, cy * r.w) : fma4(cy, r, acc);
    }
    dst[d] = acc;
  }
}

inline int lanes_block(int D4) { return D4 <= 64 ? 64 : (D4 <= 128 ? 128 : 256); }

inline bool geometry_ok(int g, int ny, int nx, int D, int nextra) {
  return g >= 1 && ny >= 1 && nx >= 1 && D > 0 && (D & 3) == 0 && nextra >= 0 && nextra <= 2 && g <= 2048 && ny <= 2048 &&
         nx <= 2048;
}

}  // namespace

extern "C" int eav_pos_bicubic_fwd(const float* pos, float* out, int g, int ny, int nx, int D, int nextra, const int* iy,
                                   const float* wy, const int* ix, const float* wx, void* stream) {
  EAV_REQUIRE(pos && out && pos != out && iy && wy && ix && wx && geometry_ok(g, ny, nx, D, nextra) &&
                  ((uintptr_t)pos & 15) == 0 && ((uintptr_t)out & 15) == 0,
              "eav_pos_bicubic_fwd: need g, ny, nx in 1 .. 2048, D %% 4 == 0, nextra <= 2, 16-byte aligned distinct pos / out "
              "and the four tap tables");
  const int rows = nextra + ny * nx;
  hipLaunchKernelGGL(pos_bicubic_fwd_kernel, dim3(rows), dim3(lanes_block(D / 4)), 0, (hipStream_t)stream, pos, out, g, ny,
                     nx, D / 4, nextra, iy, wy, ix, wx);
  EAV_CHECK_LAUNCH("eav_pos_bicubic_fwd");
  return EAV_OK;
}

extern "C" int eav_pos_bicubic_bwd(const float* dout, float* dpos, int g, int ny, int nx, int D, int nextra,
                                   const int* ypt, const int* yidx, const float* yw, int nnzy, const int* xpt,
                                   const int* xidx, const float* xw, int nnzx, void* stream) {
  EAV_REQUIRE(dout && dpos && dout != dpos && ypt && yidx && yw && xpt && xidx && xw && nnzy >= 0 && nnzx >= 0 &&
                  nnzy <= 4 * 2048 && nnzx <= 4 * 2048 && geometry_ok(g, ny, nx, D, nextra) && ((uintptr_t)dout & 15) == 0 &&
                  ((uintptr_t)dpos & 15) == 0,
              "eav_pos_bicubic_bwd: need g, ny, nx in 1 .. 2048, D %% 4 == 0, nextra <= 2, 16-byte aligned distinct dout / "
              "dpos and the transposed tap lists (at most 4 taps per output)");
  const int rows = nextra + g * g;
  hipLaunchKernelGGL(pos_bicubic_bwd_kernel, dim3(rows), dim3(lanes_block(D / 4)), 0, (hipStream_t)stream, dout, dpos, g, ny,
                     nx, D / 4, nextra, ypt, yidx, yw, nnzy, xpt, xidx, xw, nnzx);
  EAV_CHECK_LAUNCH("eav_pos_bicubic_bwd");
  return EAV_OK;
}
