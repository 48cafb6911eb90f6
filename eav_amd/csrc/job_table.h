// Device job tables: how grad_clip.hip and adam_jobs.hip cut the fp32 ranges of a table into chunks and walk them.
//
// A table is a device array of njobs rows of STRIDE int64 words; word COUNT of a row is the job's element count.  Every
// job is cut into chunks of JOB_CHUNK elements counted from ITS first element (the last one short); the chunks of job 0,
// then job 1, ... are numbered 0 .. nchunks - 1.  One workgroup of 256 handles a chunk at a time and walks the chunks with
// a grid stride of at most JOB_MAX_BLOCKS workgroups.  Inside a chunk: up to 3 scalar head elements until the address is
// 16-byte aligned, then 16-byte vectors (vector i to thread i % 256, up to JOB_VPT per thread), then up to 3 tail elements.
#pragma once
#include "eav_common.h"

constexpr int JOB_VPT = 8;                        // 16-byte vectors per thread and chunk
constexpr int JOB_CHUNK = 256 * 4 * JOB_VPT;      // 8192 elements = 32 KB
constexpr int JOB_MAX_BLOCKS = 2048;              // 256 CUs x 8 workgroups: the grid of a streaming kernel

__device__ __forceinline__ int64_t job_chunks(int64_t n) { return n > 0 ? (n + JOB_CHUNK - 1) / JOB_CHUNK : 0; }

// The job that holds chunk c.  (j, base) = a job and the number of its first chunk, carried from the workgroup's previous
// chunk: c only grows.  Wave-uniform: the table is read through the scalar cache.
template <int STRIDE, int COUNT>
__device__ __forceinline__ bool job_locate(const int64_t* __restrict__ jobs, int njobs, int64_t c, int& j, int64_t& base) {
  while (j < njobs) {
    const int64_t nc = job_chunks(jobs[STRIDE * j + COUNT]);
    if (c < base + nc) return true;
    base += nc;
    ++j;
  }
  return false;       // nchunks larger than the table holds: nothing is touched
}

// How the `len` elements at p are cut: h head elements, nvec 16-byte vectors, r tail elements.
struct JobCut {
  int h, nvec, r;
};
__device__ __forceinline__ JobCut job_cut_chunk(const float* p, int len) {
  JobCut c;
  c.h = min(len, (int)((4u - (unsigned)(((uintptr_t)p >> 2) & 3u)) & 3u));
  c.nvec = (len - c.h) >> 2;
  c.r = (len - c.h) & 3;
  return c;
}

// four consecutive floats: one 16-byte load where the address allows it (vec), four 4-byte loads otherwise
__device__ __forceinline__ float4 job_ld4(const float* p, bool vec) {
  if (vec) return *reinterpret_cast<const float4*>(p);
  return make_float4(p[0], p[1], p[2], p[3]);
}
__device__ __forceinline__ void job_st4(float* p, bool vec, const float4& x) {
  if (vec) {
    *reinterpret_cast<float4*>(p) = x;
  } else {
    p[0] = x.x; p[1] = x.y; p[2] = x.z; p[3] = x.w;
  }
}

static inline int job_grid_for(int64_t nchunks) { return (int)(nchunks < JOB_MAX_BLOCKS ? nchunks : JOB_MAX_BLOCKS); }
