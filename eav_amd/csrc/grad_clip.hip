// Global-norm gradient clipping and gradient accumulation over job tables (torch.nn.utils.clip_grad_norm_ with
// norm_type 2 and error_if_nonfinite False; the `(loss / k).backward()` k times idiom as an explicit weighted fold).
//
// A job table is a device array of njobs rows {pointer, element count} (int64 pairs) of fp32 ranges that are only
// guaranteed 4-byte aligned.  Every job is cut into chunks of CHUNK elements counted from ITS first element (the last
// one short); the chunks of job 0, then job 1, ... are numbered 0 .. nchunks - 1.  One workgroup of 256 handles a chunk
// at a time and walks the chunks with a grid stride; the fp64 sum of squares of chunk c goes to partials[c].  Which
// elements a thread adds, and in which order, follows from the chunk's address and length alone - never from the grid -
// and the partials are added in a fixed order by one workgroup: no atomics, two runs give the same bits, and so does the
// same memory presented as one job or cut into several at chunk boundaries.
//
// Inside a chunk: up to 3 scalar head elements until the address is 16-byte aligned (lanes 0-2), then 16-byte vectors
// (vector i to thread i % 256, up to VPT per thread, all loads issued before the first use), then up to 3 scalar tail
// elements.  A thread adds head, body, tail in that order in fp64; the wave totals come from a __shfl_xor butterfly,
// the four wave totals are added through LDS as (w0 + w1) + (w2 + w3).  The kernels are bound by their one pass over
// the ranges; the fp64 arithmetic hides under it.
#include "eav_common.h"
#include "job_table.h"
#include "../../include/eav_hip.h"

namespace {

constexpr int VPT = JOB_VPT;                  // 16-byte vectors per thread and chunk (job_table.h, shared with adam_jobs.hip)
constexpr int CHUNK = JOB_CHUNK;              // 8192 elements = 32 KB

__device__ __forceinline__ double sq(float x) { return (double)x * (double)x; }
__device__ __forceinline__ double sq4(const float4& a) { return ((sq(a.x) + sq(a.y)) + sq(a.z)) + sq(a.w); }

// The workgroup's total in thread 0 (every lane of a wave holds the wave's total after the butterfly).
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();                 // the previous chunk's reader is done with red
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void sumsq_kernel(const int64_t* __restrict__ jobs, int njobs, int64_t nchunks,
                                                    double* __restrict__ partials) {
  __shared__ double red[4];
  const int t = threadIdx.x;
  int j = 0;
  int64_t base = 0;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    if (!job_locate<2, 1>(jobs, njobs, c, j, base)) return;
    const int64_t off = (c - base) * CHUNK;
    const float* p = reinterpret_cast<const float*>(jobs[2 * j]) + off;
    const int len = (int)min((int64_t)CHUNK, jobs[2 * j + 1] - off);
    const JobCut k = job_cut_chunk(p, len);
    const float4* pv = reinterpret_cast<const float4*>(p + k.h);
    float4 v[VPT];
#pragma unroll
    for (int u = 0; u < VPT; ++u) {
      const int i = t + 256 * u;
      v[u] = i < k.nvec ? pv[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    double acc = t < k.h ? sq(p[t]) : 0.0;
#pragma unroll
    for (int u = 0; u < VPT; ++u) acc += sq4(v[u]);
    if (t < k.r) acc += sq(p[k.h + 4 * k.nvec + t]);
    const double s = block_sum_f64(acc, red);
    if (t == 0) partials[c] = s;
  }
}

// acc = first ? w g : fma(w, g, acc); the chunk is cut by the ACCUMULATOR's address, so that the partials are those
// sumsq_kernel forms over the accumulator afterwards; g is read in 16-byte vectors where its address allows that too.
template <bool FIRST>
__global__ __launch_bounds__(256) void fold_kernel(const int64_t* __restrict__ jobs_g, const int64_t* __restrict__ jobs_a,
                                                   int njobs, int64_t nchunks, const float* __restrict__ weight,
                                                   double* __restrict__ partials) {
  __shared__ double red[4];
  const int t = threadIdx.x;
  const float w = *weight;
  int j = 0;
  int64_t base = 0;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    if (!job_locate<2, 1>(jobs_g, njobs, c, j, base)) return;
    const int64_t off = (c - base) * CHUNK;
    const float* g = reinterpret_cast<const float*>(jobs_g[2 * j]) + off;
    float* a = reinterpret_cast<float*>(jobs_a[2 * j]) + off;
    const int len = (int)min((int64_t)CHUNK, jobs_g[2 * j + 1] - off);
    const JobCut k = job_cut_chunk(a, len);
    const bool gvec = (((uintptr_t)(g + k.h)) & 15) == 0;
    float4* av = reinterpret_cast<float4*>(a + k.h);
    const float* gb = g + k.h;
    float4 gv[VPT], ov[VPT];
#pragma unroll
    for (int u = 0; u < VPT; ++u) {
      const int i = t + 256 * u;
      gv[u] = i < k.nvec ? job_ld4(gb + 4 * (int64_t)i, gvec) : make_float4(0.f, 0.f, 0.f, 0.f);
      if (!FIRST) ov[u] = i < k.nvec ? av[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    double acc = 0.0;
    if (t < k.h) {
      const float x = FIRST ? w * g[t] : __builtin_fmaf(w, g[t], a[t]);
      a[t] = x;
      acc = sq(x);
    }
#pragma unroll
    for (int u = 0; u < VPT; ++u) {
      const int i = t + 256 * u;
      float4 x;
      if (FIRST) {
        x = make_float4(w * gv[u].x, w * gv[u].y, w * gv[u].z, w * gv[u].w);
      } else {
        x = make_float4(__builtin_fmaf(w, gv[u].x, ov[u].x), __builtin_fmaf(w, gv[u].y, ov[u].y),
                        __builtin_fmaf(w, gv[u].z, ov[u].z), __builtin_fmaf(w, gv[u].w, ov[u].w));
      }
      if (i < k.nvec) {
        av[i] = x;
        acc += sq4(x);
      }
    }
    if (t < k.r) {
      const int e = k.h + 4 * k.nvec + t;
      const float x = FIRST ? w * g[e] : __builtin_fmaf(w, g[e], a[e]);
      a[e] = x;
      acc += sq(x);
    }
    if (partials) {                  // uniform
      const double s = block_sum_f64(acc, red);
      if (t == 0) partials[c] = s;
    }
  }
}

// g *= *scalar in place; nothing is written when the scalar is exactly 1 (scale_by_scalar_kernel's rule)
__global__ __launch_bounds__(256) void scale_ranges_kernel(const int64_t* __restrict__ jobs, int njobs, int64_t nchunks,
                                                           const float* __restrict__ scalar) {
  const float s = *scalar;
  if (s == 1.f) return;
  const int t = threadIdx.x;
  int j = 0;
  int64_t base = 0;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    if (!job_locate<2, 1>(jobs, njobs, c, j, base)) return;
    const int64_t off = (c - base) * CHUNK;
    float* p = reinterpret_cast<float*>(jobs[2 * j]) + off;
    const int len = (int)min((int64_t)CHUNK, jobs[2 * j + 1] - off);
    const JobCut k = job_cut_chunk(p, len);
    float4* pv = reinterpret_cast<float4*>(p + k.h);
    float4 v[VPT];
#pragma unroll
    for (int u = 0; u < VPT; ++u) {
      const int i = t + 256 * u;
      v[u] = i < k.nvec ? pv[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (t < k.h) p[t] *= s;
#pragma unroll
    for (int u = 0; u < VPT; ++u) {
      const int i = t + 256 * u;
      if (i < k.nvec) pv[i] = make_float4(v[u].x * s, v[u].y * s, v[u].z * s, v[u].w * s);
    }
    if (t < k.r) p[k.h + 4 * k.nvec + t] *= s;
  }
}

// One workgroup: thread t adds partials t, t + 256, ... in index order, the 256 sums are added like a chunk's.
//   out2[0] = (float)sqrt(sum);  out2[1] = clamp(max_norm / (out2[0] + 1e-6f), max = 1)  - torch's clip_grad_norm_:
// an IEEE fp32 division (hipcc's default), a NaN norm gives a NaN coefficient, an infinite norm 0.
__global__ __launch_bounds__(256) void clip_finish_kernel(const double* __restrict__ partials, int64_t nchunks,
                                                          float max_norm, float* __restrict__ out2) {
  __shared__ double red[4];
  double acc = 0.0;
#pragma unroll 8
  for (int64_t i = threadIdx.x; i < nchunks; i += 256) acc += partials[i];      // loads ahead, adds in index order
  const double s = block_sum_f64(acc, red);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(s);
    const float coef = max_norm / (norm + 1e-6f);
    out2[0] = norm;
    out2[1] = coef > 1.f ? 1.f : coef;          // a NaN stays a NaN
  }
}

}  // namespace

extern "C" int64_t eav_grad_chunk_elems(void) { return CHUNK; }

// chunks of ONE job of n elements; a table has the sum over its jobs
extern "C" int64_t eav_grad_nchunks(int64_t n) { return n > 0 ? cdiv64(n, CHUNK) : 0; }

extern "C" int eav_grad_sumsq(const void* jobs, int njobs, int64_t nchunks, double* partials, void* stream) {
  EAV_REQUIRE(jobs && partials && njobs > 0 && nchunks > 0, "eav_grad_sumsq: bad arguments (table, partials, njobs > 0, nchunks > 0)");
  hipLaunchKernelGGL(sumsq_kernel, dim3(job_grid_for(nchunks)), dim3(256), 0, (hipStream_t)stream, (const int64_t*)jobs, njobs,
                     nchunks, partials);
  EAV_CHECK_LAUNCH("eav_grad_sumsq");
  return EAV_OK;
}

extern "C" int eav_grad_fold(const void* jobs_g, const void* jobs_acc, int njobs, int64_t nchunks, const float* weight,
                             int first, double* partials, void* stream) {
  EAV_REQUIRE(jobs_g && jobs_acc && weight && njobs > 0 && nchunks > 0,
              "eav_grad_fold: bad arguments (two tables, weight, njobs > 0, nchunks > 0)");
  if (first)
    hipLaunchKernelGGL(fold_kernel<true>, dim3(job_grid_for(nchunks)), dim3(256), 0, (hipStream_t)stream,
                       (const int64_t*)jobs_g, (const int64_t*)jobs_acc, njobs, nchunks, weight, partials);
  else
    hipLaunchKernelGGL(fold_kernel<false>, dim3(job_grid_for(nchunks)), dim3(256), 0, (hipStream_t)stream,
                       (const int64_t*)jobs_g, (const int64_t*)jobs_acc, njobs, nchunks, weight, partials);
  EAV_CHECK_LAUNCH("eav_grad_fold");
  return EAV_OK;
}

extern "C" int eav_grad_clip_finish(const double* partials, int64_t nchunks, float max_norm, float* out2, void* stream) {
  EAV_REQUIRE(partials && out2 && nchunks > 0, "eav_grad_clip_finish: bad arguments (partials, out2, nchunks > 0)");
  EAV_REQUIRE(max_norm > 0.f, "eav_grad_clip_finish: max_norm must be positive, got %g", (double)max_norm);
  hipLaunchKernelGGL(clip_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, nchunks, max_norm, out2);
  EAV_CHECK_LAUNCH("eav_grad_clip_finish");
  return EAV_OK;
}

extern "C" int eav_scale_ranges(const void* jobs, int njobs, int64_t nchunks, const float* scalar, void* stream) {
  EAV_REQUIRE(jobs && scalar && njobs > 0 && nchunks > 0, "eav_scale_ranges: bad arguments (table, scalar, njobs > 0, nchunks > 0)");
  hipLaunchKernelGGL(scale_ranges_kernel, dim3(job_grid_for(nchunks)), dim3(256), 0, (hipStream_t)stream, (const int64_t*)jobs,
                     njobs, nchunks, scalar);
  EAV_CHECK_LAUNCH("eav_scale_ranges");
  return EAV_OK;
}
