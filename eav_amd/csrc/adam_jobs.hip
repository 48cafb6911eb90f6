// Multi-tensor Adam / AdamW over a device job table: per-tensor learning rate, weight decay and step count, and a
// learning-rate schedule whose state lives in device memory - one optimiser step is two launches however many tensors and
// hyper-parameter groups there are, nothing is read back, and the step can be captured in a hipGraph and replayed.
//
// A job row is EAV_ADAM_JOB_WORDS (10) int64 words = 80 bytes (include/eav_hip.h):
//   0 p   1 g   2 m   3 v        fp32 ranges of `numel` elements, 4-byte aligned at least
//   4 numel
//   5 base_lr                    the bits of a double
//   6 step                       pointer to the device int64 step count the job reads
//   7 weight_decay               fp32 bits in the low half
//   8 lr | bc1 << 32             fp32 bits, written by eav_adam_jobs_begin: lr = (float)(base_lr * factor),
//   9 bc2s                       bc1 = 1 - b1^step, bc2s = sqrt(1 - b2^step) (adam_bias_corrections, eav_common.h)
// The schedule record is EAV_ADAM_SCHED_WORDS (4) int64 words: 0 t (optimiser steps completed since the schedule was
// attached), 1 the factor of the last step (double), 2 (float)(report_lr * factor) of the last step (fp32, low half), 3 unused.
//
// eav_adam_jobs_begin is one workgroup: it advances the step counts, evaluates the schedule factor in fp64 from t, advances
// t and fills words 8-9 of every row.  eav_adam_step_jobs walks the chunks of the table as grad_clip.hip does (job_table.h:
// chunks of 8192 elements counted from each job's first element, a grid stride of at most 2048 workgroups of 256): inside
// a chunk up to 3 scalar head elements until p is 16-byte aligned, 16-byte vectors, up to 3 tail elements; g, m and v are
// accessed as vectors where their own addresses allow it and element-wise otherwise.  Every load of a chunk - 4 x 8 vectors
// and up to 2 x 4 scalars per thread - is issued before the first use; 16 B are read and 12 B written per element.  The
// element update is adam_update (eav_common.h), the one adam_kernel of head_optim.hip runs: same bits.  No atomics; the rows
// are read with wave-uniform indices, through the scalar cache.
//
// Weight averaging (EMA / SWA) rides in the same two launches.  The averaging record is EAV_ADAM_AVG_WORDS (4) int64 words:
// 0 s (optimiser steps seen since averaging was attached), 1 n (n_averaged), 2 c | mode << 32 (the fp32 coefficient of the
// current step and EAV_AVG_SKIP / COPY / LERP), 3 unused.  eav_adam_jobs_begin_avg is eav_adam_jobs_begin plus, in the same
// workgroup, s += 1, the mode of this step and c (fp64, rounded once).  eav_adam_step_jobs_avg is the same walk with a
// parallel array of avg pointers: skip touches no average (the mode is wave-uniform), copy stores the new p, lerp loads the
// chunk's averages with the other loads - 8 more vectors per thread - and stores fmaf(c, p_new - avg, avg): 20 B read and
// 16 B written per element.  eav_swap_jobs exchanges the p and avg ranges of such a table.
#include "eav_common.h"
#include "job_table.h"
#include "../../include/eav_hip.h"

namespace {

constexpr int W = EAV_ADAM_JOB_WORDS;
static_assert(W == 10 && (W * 8) % 16 == 0 && EAV_ADAM_SCHED_WORDS == 4 && EAV_ADAM_AVG_WORDS == 4,
              "row layouts of include/eav_hip.h");

__device__ __forceinline__ float word_lo(int64_t w) { return __int_as_float((int)(uint32_t)((uint64_t)w & 0xffffffffull)); }
__device__ __forceinline__ float word_hi(int64_t w) { return __int_as_float((int)(uint32_t)((uint64_t)w >> 32)); }
__device__ __forceinline__ int64_t word_pack(float lo, float hi) {
  return (int64_t)(((uint64_t)__float_as_uint(hi) << 32) | (uint64_t)__float_as_uint(lo));
}

// The lambdas behind transformers.get_scheduler for "constant", "constant_with_warmup", "linear", "cosine", in fp64 and
// in their operation order; t = optimiser steps completed, so the first step of a warmup runs at factor 0.
__device__ double schedule_factor(int kind, int64_t t, int64_t warmup, int64_t total, double cycles) {
#pragma clang fp contract(off)
  if (kind == EAV_SCHED_CONSTANT) return 1.0;
  if (t < warmup) return (double)t / (double)max((int64_t)1, warmup);
  if (kind == EAV_SCHED_CONSTANT_WITH_WARMUP) return 1.0;
  const double span = (double)max((int64_t)1, total - warmup);
  if (kind == EAV_SCHED_LINEAR) return fmax(0.0, (double)(total - t) / span);
  const double progress = (double)(t - warmup) / span;
  return fmax(0.0, 0.5 * (1.0 + cos(3.14159265358979323846 * cycles * 2.0 * progress)));
}

__device__ __forceinline__ void jobs_begin(int64_t* jobs, int njobs, int64_t* counts, int ncounts, int64_t* sched, int kind,
                                           int64_t warmup, int64_t total, double cycles, double report_lr, float b1,
                                           float b2) {
  __shared__ double fac;
  const int t = threadIdx.x;
  for (int i = t; i < ncounts; i += 256) counts[i] += 1;
  if (t == 0) {
    const int64_t s = sched[0];
    const double f = schedule_factor(kind, s, warmup, total, cycles);
    fac = f;
    sched[0] = s + 1;
    sched[1] = __double_as_longlong(f);
    sched[2] = word_pack((float)(report_lr * f), 0.f);
  }
  __syncthreads();          // the counts above are visible to the rows' readers below (one workgroup)
  const double f = fac;
  for (int j = t; j < njobs; j += 256) {
    int64_t* row = jobs + (int64_t)W * j;
    const double base_lr = __longlong_as_double(row[5]);
    const double st = (double)*reinterpret_cast<const int64_t*>(row[6]);
    float bc1, bc2s;
    adam_bias_corrections(b1, b2, st, bc1, bc2s);
    const float lr = (float)(base_lr * f);
    row[8] = word_pack(lr, bc1);
    row[9] = word_pack(bc2s, 0.f);
  }
}

__global__ __launch_bounds__(256) void adam_jobs_begin_kernel(int64_t* jobs, int njobs, int64_t* counts, int ncounts,
                                                              int64_t* sched, int kind, int64_t warmup, int64_t total,
                                                              double cycles, double report_lr, float b1, float b2) {
  jobs_begin(jobs, njobs, counts, ncounts, sched, kind, warmup, total, cycles, report_lr, b1, b2);
}

// The averaging record of this step: s counts from 1; an averaging step is s >= start with (s - start) % every == 0.  The
// first one copies (torch.optim.swa_utils.AveragedModel's first update), later ones lerp with c = 1 - d (EMA; with warmup
// d = min(decay, (1 + n) / (10 + n))) or 1 / (n + 1) (SWA), in fp64 and rounded once.  c reads 1 on a copy and 0 on a skip.
__device__ void avg_advance(int64_t* rec, int kind, double decay, int warm, int64_t start, int64_t every) {
#pragma clang fp contract(off)
  const int64_t s = rec[0] + 1, n = rec[1];
  int mode = EAV_AVG_SKIP;
  float c = 0.f;
  if (s >= start && (s - start) % every == 0) {
    if (n == 0) {
      mode = EAV_AVG_COPY;
      c = 1.f;
    } else {
      mode = EAV_AVG_LERP;
      if (kind == EAV_AVG_EMA) {
        double d = decay;
        if (warm) d = fmin(decay, (1.0 + (double)n) / (10.0 + (double)n));
        c = (float)(1.0 - d);
      } else {
        c = (float)(1.0 / ((double)n + 1.0));
      }
    }
    rec[1] = n + 1;
  }
  rec[0] = s;
  rec[2] = (int64_t)(((uint64_t)(uint32_t)mode << 32) | (uint64_t)__float_as_uint(c));
}

__global__ __launch_bounds__(256) void adam_jobs_begin_avg_kernel(int64_t* jobs, int njobs, int64_t* counts, int ncounts,
                                                                  int64_t* sched, int kind, int64_t warmup, int64_t total,
                                                                  double cycles, double report_lr, float b1, float b2,
                                                                  int64_t* rec, int avg_kind, double decay, int avg_warmup,
                                                                  int64_t start, int64_t every) {
  if (threadIdx.x == 255) avg_advance(rec, avg_kind, decay, avg_warmup, start, every);
  jobs_begin(jobs, njobs, counts, ncounts, sched, kind, warmup, total, cycles, report_lr, b1, b2);
}

__device__ __forceinline__ bool aligned16(const float* p) { return (((uintptr_t)p) & 15) == 0; }

template <bool SCALED>
__device__ __forceinline__ void update4(float4& p, const float4& g, float4& m, float4& v, float gs, float lr, float b1,
                                        float b2, float eps, float wd, float bc1, float bc2s, int decoupled) {
  adam_update<SCALED>(p.x, g.x, m.x, v.x, gs, lr, b1, b2, eps, wd, bc1, bc2s, decoupled);
  adam_update<SCALED>(p.y, g.y, m.y, v.y, gs, lr, b1, b2, eps, wd, bc1, bc2s, decoupled);
  adam_update<SCALED>(p.z, g.z, m.z, v.z, gs, lr, b1, b2, eps, wd, bc1, bc2s, decoupled);
  adam_update<SCALED>(p.w, g.w, m.w, v.w, gs, lr, b1, b2, eps, wd, bc1, bc2s, decoupled);
}

__device__ __forceinline__ float4 lerp4(float c, const float4& p, const float4& a) {
  return make_float4(fmaf(c, p.x - a.x, a.x), fmaf(c, p.y - a.y, a.y), fmaf(c, p.z - a.z, a.z), fmaf(c, p.w - a.w, a.w));
}

// AVG = false is eav_adam_step_jobs' kernel; AVG = true adds the averages (avgs[j]: job j's range, rec: the averaging record).
template <bool SCALED, bool AVG>
__global__ __launch_bounds__(256) void adam_jobs_kernel(const int64_t* __restrict__ jobs, int njobs, int64_t nchunks,
                                                        float b1, float b2, float eps, int decoupled,
                                                        const float* __restrict__ gscale,
                                                        const int64_t* __restrict__ avgs, const int64_t* __restrict__ rec) {
  float gs = 1.f;
  if (SCALED) gs = *gscale;
  float cf = 0.f;
  bool lerp = false, put = false;                       // uniform: put = the average is written (copy or lerp)
  if (AVG) {
    const int64_t w = rec[2];
    const int mode = (int)((uint64_t)w >> 32);
    cf = word_lo(w);
    lerp = mode == EAV_AVG_LERP;
    put = lerp || mode == EAV_AVG_COPY;
  }
  const int t = threadIdx.x;
  int j = 0;
  int64_t base = 0;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    if (!job_locate<W, 4>(jobs, njobs, c, j, base)) return;
    const int64_t* row = jobs + (int64_t)W * j;
    const int64_t off = (c - base) * JOB_CHUNK;
    float* p = reinterpret_cast<float*>(row[0]) + off;
    const float* g = reinterpret_cast<const float*>(row[1]) + off;
    float* m = reinterpret_cast<float*>(row[2]) + off;
    float* v = reinterpret_cast<float*>(row[3]) + off;
    float* a = AVG ? reinterpret_cast<float*>(avgs[j]) + off : nullptr;
    const int len = (int)min((int64_t)JOB_CHUNK, row[4] - off);
    const float wd = word_lo(row[7]), lr = word_lo(row[8]), bc1 = word_hi(row[8]), bc2s = word_lo(row[9]);
    const JobCut k = job_cut_chunk(p, len);
    float4* pb = reinterpret_cast<float4*>(p + k.h);
    const float* gb = g + k.h;
    float* mb = m + k.h;
    float* vb = v + k.h;
    float* ab = AVG ? a + k.h : nullptr;
    const bool gvec = aligned16(gb), mvec = aligned16(mb), vvec = aligned16(vb);      // uniform
    const bool avec = AVG && aligned16(ab);
    const bool head = t < k.h, tail = t < k.r;
    const int et = k.h + 4 * k.nvec + t;
    // every load of the chunk, then the arithmetic and the stores
    float ph = 0.f, gh = 0.f, mh = 0.f, vh = 0.f, pt = 0.f, gt = 0.f, mt = 0.f, vt = 0.f, ah = 0.f, at = 0.f;
    if (head) { ph = p[t]; gh = g[t]; mh = m[t]; vh = v[t]; }
    if (tail) { pt = p[et]; gt = g[et]; mt = m[et]; vt = v[et]; }
    if (AVG && lerp) {
      if (head) ah = a[t];
      if (tail) at = a[et];
    }
    float4 pq[JOB_VPT], gq[JOB_VPT], mq[JOB_VPT], vq[JOB_VPT], aq[AVG ? JOB_VPT : 1];
#pragma unroll
    for (int u = 0; u < JOB_VPT; ++u) {
      const int i = t + 256 * u;
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      pq[u] = gq[u] = mq[u] = vq[u] = z;
      if (AVG) aq[u] = z;
      if (i < k.nvec) {
        pq[u] = pb[i];
        gq[u] = job_ld4(gb + 4 * (int64_t)i, gvec);
        mq[u] = job_ld4(mb + 4 * (int64_t)i, mvec);
        vq[u] = job_ld4(vb + 4 * (int64_t)i, vvec);
        if (AVG && lerp) aq[u] = job_ld4(ab + 4 * (int64_t)i, avec);
      }
    }
    if (head) {
      adam_update<SCALED>(ph, gh, mh, vh, gs, lr, b1, b2, eps, wd, bc1, bc2s, decoupled);
      m[t] = mh; v[t] = vh; p[t] = ph;
      if (AVG && put) a[t] = lerp ? fmaf(cf, ph - ah, ah) : ph;
    }
#pragma unroll
    for (int u = 0; u < JOB_VPT; ++u) {
      const int i = t + 256 * u;
      update4<SCALED>(pq[u], gq[u], mq[u], vq[u], gs, lr, b1, b2, eps, wd, bc1, bc2s, decoupled);
      if (i < k.nvec) {
        job_st4(mb + 4 * (int64_t)i, mvec, mq[u]);
        job_st4(vb + 4 * (int64_t)i, vvec, vq[u]);
        pb[i] = pq[u];
        if (AVG && put) job_st4(ab + 4 * (int64_t)i, avec, lerp ? lerp4(cf, pq[u], aq[u]) : pq[u]);
      }
    }
    if (tail) {
      adam_update<SCALED>(pt, gt, mt, vt, gs, lr, b1, b2, eps, wd, bc1, bc2s, decoupled);
      m[et] = mt; v[et] = vt; p[et] = pt;
      if (AVG && put) a[et] = lerp ? fmaf(cf, pt - at, at) : pt;
    }
  }
}

// p <-> avg over the ranges of a table: cut by p's address like the step, both loads before either store
__global__ __launch_bounds__(256) void swap_jobs_kernel(const int64_t* __restrict__ jobs, const int64_t* __restrict__ avgs,
                                                        int njobs, int64_t nchunks) {
  const int t = threadIdx.x;
  int j = 0;
  int64_t base = 0;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    if (!job_locate<W, 4>(jobs, njobs, c, j, base)) return;
    const int64_t* row = jobs + (int64_t)W * j;
    const int64_t off = (c - base) * JOB_CHUNK;
    float* p = reinterpret_cast<float*>(row[0]) + off;
    float* a = reinterpret_cast<float*>(avgs[j]) + off;
    const int len = (int)min((int64_t)JOB_CHUNK, row[4] - off);
    const JobCut k = job_cut_chunk(p, len);
    float4* pb = reinterpret_cast<float4*>(p + k.h);
    float* ab = a + k.h;
    const bool avec = aligned16(ab);
    const bool head = t < k.h, tail = t < k.r;
    const int et = k.h + 4 * k.nvec + t;
    float ph = 0.f, ah = 0.f, pt = 0.f, at = 0.f;
    if (head) { ph = p[t]; ah = a[t]; }
    if (tail) { pt = p[et]; at = a[et]; }
    float4 pq[JOB_VPT], aq[JOB_VPT];
#pragma unroll
    for (int u = 0; u < JOB_VPT; ++u) {
      const int i = t + 256 * u;
      pq[u] = aq[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (i < k.nvec) {
        pq[u] = pb[i];
        aq[u] = job_ld4(ab + 4 * (int64_t)i, avec);
      }
    }
    if (head) { p[t] = ah; a[t] = ph; }
#pragma unroll
    for (int u = 0; u < JOB_VPT; ++u) {
      const int i = t + 256 * u;
      if (i < k.nvec) {
        pb[i] = aq[u];
        job_st4(ab + 4 * (int64_t)i, avec, pq[u]);
      }
    }
    if (tail) { p[et] = at; a[et] = pt; }
  }
}

}  // namespace

extern "C" int64_t eav_adam_jobs_nchunks(int64_t n) { return n > 0 ? cdiv64(n, JOB_CHUNK) : 0; }

extern "C" int eav_adam_jobs_begin(void* jobs, int njobs, int64_t* counts, int ncounts, void* sched, int kind,
                                   int64_t warmup_steps, int64_t training_steps, double num_cycles, double report_lr,
                                   float beta1, float beta2, void* stream) {
  EAV_REQUIRE(jobs && sched && njobs > 0 && ncounts >= 0 && (counts || ncounts == 0),
              "eav_adam_jobs_begin: bad arguments (table, schedule record, njobs > 0, ncounts >= 0 with their array)");
  EAV_REQUIRE(kind >= EAV_SCHED_CONSTANT && kind <= EAV_SCHED_COSINE,
              "eav_adam_jobs_begin: unknown schedule kind %d (0 constant, 1 constant_with_warmup, 2 linear, 3 cosine)", kind);
  EAV_REQUIRE(warmup_steps >= 0 && training_steps >= 0, "eav_adam_jobs_begin: negative warmup or training steps");
  hipLaunchKernelGGL(adam_jobs_begin_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (int64_t*)jobs, njobs, counts,
                     ncounts, (int64_t*)sched, kind, warmup_steps, training_steps, num_cycles, report_lr, beta1, beta2);
  EAV_CHECK_LAUNCH("eav_adam_jobs_begin");
  return EAV_OK;
}

extern "C" int eav_adam_step_jobs(const void* jobs, int njobs, int64_t nchunks, float beta1, float beta2, float eps,
                                  int decoupled, const float* gscale, void* stream) {
  EAV_REQUIRE(jobs && njobs > 0 && nchunks > 0, "eav_adam_step_jobs: bad arguments (table, njobs > 0, nchunks > 0)");
  if (gscale)
    hipLaunchKernelGGL((adam_jobs_kernel<true, false>), dim3(job_grid_for(nchunks)), dim3(256), 0, (hipStream_t)stream,
                       (const int64_t*)jobs, njobs, nchunks, beta1, beta2, eps, decoupled, gscale, nullptr, nullptr);
  else
    hipLaunchKernelGGL((adam_jobs_kernel<false, false>), dim3(job_grid_for(nchunks)), dim3(256), 0, (hipStream_t)stream,
                       (const int64_t*)jobs, njobs, nchunks, beta1, beta2, eps, decoupled, gscale, nullptr, nullptr);
  EAV_CHECK_LAUNCH("eav_adam_step_jobs");
  return EAV_OK;
}

extern "C" int eav_adam_jobs_begin_avg(void* jobs, int njobs, int64_t* counts, int ncounts, void* sched, int kind,
                                       int64_t warmup_steps, int64_t training_steps, double num_cycles, double report_lr,
                                       float beta1, float beta2, void* avg_record, int avg_kind, double decay,
                                       int avg_warmup, int64_t start_step, int64_t every, void* stream) {
  EAV_REQUIRE(jobs && sched && njobs > 0 && ncounts >= 0 && (counts || ncounts == 0),
              "eav_adam_jobs_begin_avg: bad arguments (table, schedule record, njobs > 0, ncounts >= 0 with their array)");
  EAV_REQUIRE(kind >= EAV_SCHED_CONSTANT && kind <= EAV_SCHED_COSINE,
              "eav_adam_jobs_begin_avg: unknown schedule kind %d (0 constant, 1 constant_with_warmup, 2 linear, 3 cosine)", kind);
  EAV_REQUIRE(warmup_steps >= 0 && training_steps >= 0, "eav_adam_jobs_begin_avg: negative warmup or training steps");
  EAV_REQUIRE(avg_record, "eav_adam_jobs_begin_avg: avg_record is NULL");
  EAV_REQUIRE(avg_kind == EAV_AVG_EMA || avg_kind == EAV_AVG_SWA,
              "eav_adam_jobs_begin_avg: unknown avg_kind %d (0 ema, 1 swa)", avg_kind);
  EAV_REQUIRE(decay >= 0.0 && decay <= 1.0, "eav_adam_jobs_begin_avg: decay %g outside [0, 1]", decay);
  EAV_REQUIRE(every >= 1, "eav_adam_jobs_begin_avg: every %lld < 1", (long long)every);
  EAV_REQUIRE(start_step >= 0, "eav_adam_jobs_begin_avg: negative start_step %lld", (long long)start_step);
  hipLaunchKernelGGL(adam_jobs_begin_avg_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (int64_t*)jobs, njobs, counts,
                     ncounts, (int64_t*)sched, kind, warmup_steps, training_steps, num_cycles, report_lr, beta1, beta2,
                     (int64_t*)avg_record, avg_kind, decay, avg_warmup != 0, start_step, every);
  EAV_CHECK_LAUNCH("eav_adam_jobs_begin_avg");
  return EAV_OK;
}

extern "C" int eav_adam_step_jobs_avg(const void* jobs, const void* avgs, int njobs, int64_t nchunks, float beta1,
                                      float beta2, float eps, int decoupled, const float* gscale, const void* avg_record,
                                      void* stream) {
  EAV_REQUIRE(jobs && njobs > 0 && nchunks > 0, "eav_adam_step_jobs_avg: bad arguments (table, njobs > 0, nchunks > 0)");
  EAV_REQUIRE(avgs && avg_record, "eav_adam_step_jobs_avg: avgs or avg_record is NULL");
  if (gscale)
    hipLaunchKernelGGL((adam_jobs_kernel<true, true>), dim3(job_grid_for(nchunks)), dim3(256), 0, (hipStream_t)stream,
                       (const int64_t*)jobs, njobs, nchunks, beta1, beta2, eps, decoupled, gscale, (const int64_t*)avgs,
                       (const int64_t*)avg_record);
  else
    hipLaunchKernelGGL((adam_jobs_kernel<false, true>), dim3(job_grid_for(nchunks)), dim3(256), 0, (hipStream_t)stream,
                       (const int64_t*)jobs, njobs, nchunks, beta1, beta2, eps, decoupled, gscale, (const int64_t*)avgs,
                       (const int64_t*)avg_record);
  EAV_CHECK_LAUNCH("eav_adam_step_jobs_avg");
  return EAV_OK;
}

extern "C" int eav_swap_jobs(const void* jobs, const void* avgs, int njobs, int64_t nchunks, void* stream) {
  EAV_REQUIRE(jobs && avgs && njobs > 0 && nchunks > 0,
              "eav_swap_jobs: bad arguments (table, avgs, njobs > 0, nchunks > 0)");
  hipLaunchKernelGGL(swap_jobs_kernel, dim3(job_grid_for(nchunks)), dim3(256), 0, (hipStream_t)stream, (const int64_t*)jobs,
                     (const int64_t*)avgs, njobs, nchunks);
  EAV_CHECK_LAUNCH("eav_swap_jobs");
  return EAV_OK;
}
