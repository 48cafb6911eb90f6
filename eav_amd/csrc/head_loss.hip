// The two losses beside cross-entropy that Hugging Face's ForSequenceClassificationLoss picks from config.problem_type:
// nn.BCEWithLogitsLoss ("multi_label_classification") and nn.MSELoss ("regression"), both with torch's default mean over
// all B * NC elements, each with its gradient from the same launch.
//
//   eav_bce_logits_fwd_bwd   term max(x, 0) - x t + log1p(exp(-|x|)) (torch's form: finite at x = +-1e4), gradient
//                            (sigmoid(x) - t) / (B NC), *nhits += #elements with (x > 0) == (t > 0.5)
//   eav_mse_fwd_bwd          term (x - t)^2, gradient 2 (x - t) / (B NC)
//
// Built like eav_ce_wide_fwd_bwd (head_wide.hip): one wave per row, four rows per block, the lanes striding the row so
// that every read and write is coalesced; the per-row sums go to ws and a one-wave kernel adds them in row order.  The
// summation order depends on the shape alone: there are no atomics, and two runs give the same bits.
#include "eav_common.h"
#include "../../include/eav_hip.h"

namespace {

// terms[b] = the row's sum of loss terms; BCE: terms[B + b] = the row's hits (an integer <= NC <= 32768: exact in fp32)
template <bool BCE>
__global__ __launch_bounds__(256) void head_loss_rows_kernel(const float* __restrict__ logits,
                                                             const float* __restrict__ targets,
                                                             float* __restrict__ dlogits, float* __restrict__ terms, int B,
                                                             int NC) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float n = (float)((int64_t)B * NC);
  const float* x = logits + (int64_t)b * NC;
  const float* t = targets + (int64_t)b * NC;
  float* d = dlogits ? dlogits + (int64_t)b * NC : nullptr;
  float s = 0.f;
  int hits = 0;
  for (int j = lane; j < NC; j += 64) {
    const float xv = x[j], tv = t[j];
    if constexpr (BCE) {
      const float e = expf(-fabsf(xv));                       // in (0, 1]: neither side of the sigmoid overflows
      s += (fmaxf(xv, 0.f) - xv * tv) + log1pf(e);
      hits += ((xv > 0.f) == (tv > 0.5f)) ? 1 : 0;
      if (d) d[j] = ((xv >= 0.f ? 1.f : e) / (1.f + e) - tv) / n;
    } else {
      const float df = xv - tv;
      s += df * df;
      if (d) d[j] = 2.f * df / n;
    }
  }
  s = wave_sum(s);
  if constexpr (BCE) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) hits += __shfl_xor(hits, o, 64);
  }
  if (lane == 0) {
    terms[b] = s;
    if constexpr (BCE) terms[B + b] = (float)hits;
  }
}

// The per-row sums added in row order: 64 consecutive rows per trip (a wave sum), the trips one after another.
__global__ __launch_bounds__(64) void head_loss_finish_kernel(const float* __restrict__ terms, float* __restrict__ loss,
                                                              int* __restrict__ nhits, int B, int NC) {
  const int lane = threadIdx.x;
  float tot = 0.f;
  int hits = 0;
  for (int b0 = 0; b0 < B; b0 += 64) {
    const int b = b0 + lane;
    tot += wave_sum(b < B ? terms[b] : 0.f);
    if (nhits && b < B) hits += (int)terms[B + b];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) hits += __shfl_xor(hits, o, 64);
  if (lane == 0 && loss) *loss = tot / (float)((int64_t)B * NC);
  if (lane == 1 && nhits) *nhits += hits;
}

bool loss_shape_ok(int B, int NC) {
  return B > 0 && NC > 0 && NC <= EAV_HEAD_MAX_CLASSES && (int64_t)B * NC < (1ll << 31);
}

template <bool BCE>
int head_loss_launch(const char* name, const float* logits, const float* targets, float* loss, float* dlogits, int* nhits,
                     float* ws, int B, int NC, void* stream) {
  hipLaunchKernelGGL(head_loss_rows_kernel<BCE>, dim3(cdiv(B, 4)), dim3(256), 0, (hipStream_t)stream, logits, targets,
                     dlogits, ws, B, NC);
  EAV_CHECK_LAUNCH(name);
  if (loss || nhits) {
    hipLaunchKernelGGL(head_loss_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, ws, loss, nhits, B, NC);
    EAV_CHECK_LAUNCH(name);
  }
  return EAV_OK;
}

}  // namespace

extern "C" int64_t eav_head_loss_ws_floats(int B) { return B > 0 ? 2 * (int64_t)B : 0; }

extern "C" int eav_bce_logits_fwd_bwd(const float* logits, const float* targets, float* loss, float* dlogits, int* nhits,
                                      float* ws, int B, int NC, void* stream) {
  EAV_REQUIRE(logits && targets && ws && loss_shape_ok(B, NC), "eav_bce_logits_fwd_bwd: bad arguments (classes <= %d)",
              EAV_HEAD_MAX_CLASSES);
  return head_loss_launch<true>("eav_bce_logits_fwd_bwd", logits, targets, loss, dlogits, nhits, ws, B, NC, stream);
}

extern "C" int eav_mse_fwd_bwd(const float* logits, const float* targets, float* loss, float* dlogits, float* ws, int B,
                               int NC, void* stream) {
  EAV_REQUIRE(logits && targets && ws && loss_shape_ok(B, NC), "eav_mse_fwd_bwd: bad arguments (classes <= %d)",
              EAV_HEAD_MAX_CLASSES);
  return head_loss_launch<false>("eav_mse_fwd_bwd", logits, targets, loss, dlogits, nullptr, ws, B, NC, stream);
}
