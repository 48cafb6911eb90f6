// The general cross-entropy: torch.nn.functional.cross_entropy(in, target, weight=weight, label_smoothing=eps) with mean
// reduction, for class-index targets (ignore_index -100) and for class-probability targets (mixup), the loss and its
// gradient from the same launch.  eav_ce_fwd_bwd / eav_ce_wide_fwd_bwd stay what the default criterion launches.
//
// With C classes, w = 1 where there is no weight, W = sum_c w_c and logp = log-softmax(in):
//   index targets   D = sum over the valid rows (0 <= y < C) of w[y_b]
//                   loss = [ (1 - eps) sum_b w[y_b] (-logp[b, y_b]) + (eps / C) sum_b sum_c w_c (-logp[b, c]) ] / D
//                   din[b, j] = [ (1 - eps) w[y_b] (p_j - [j == y_b]) + (eps / C) (p_j W - w_j) ] / D
//                   rows with a label outside [0, C) give nothing and get a zero gradient; D == 0: NaN loss, zero gradient
//   probabilities   t' = (1 - eps) t + eps / C
//                   loss = - sum_b sum_c w_c t'[b, c] logp[b, c] / B
//                   din[b, j] = [ p_j sum_c w_c t'_c - w_j t'_j ] / B
//
// Built like eav_ce_wide_fwd_bwd (head_wide.hip): one wave per row, four rows per block, the lanes striding the row so
// that every read and write is coalesced and a weight is read once per lane stride; the per-row terms go to ws and a
// one-wave kernel adds them in row order.  The summation order depends on the shape alone: there are no atomics, and two
// runs give the same bits.
#include "eav_common.h"
#include "../../include/eav_hip.h"

namespace {

// (value, index) of the larger value, the smaller index on a tie
__device__ __forceinline__ void first_max_merge(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

__device__ __forceinline__ void wave_first_max(float& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    first_max_merge(v, i, ov, oi);
  }
}

// D of the index targets: the weights of the valid labels, lane l adding rows l, l + 64, ... and the lanes added by the
// butterfly.  The row kernel's waves and the finish kernel all form it this way: one value, bit for bit.
__device__ __forceinline__ float label_weight_sum(const int64_t* __restrict__ y, const float* __restrict__ weight, int B,
                                                  int NC, int lane) {
  float d = 0.f;
  for (int i = lane; i < B; i += 64) {
    const int64_t yl = y[i];
    if (yl >= 0 && yl < NC) d += weight ? weight[yl] : 1.f;
  }
  return wave_sum(d);
}

// terms[b] = the row's share of the loss numerator, terms[B + b] = 1 for a hit
template <bool PROB>
__global__ __launch_bounds__(256) void ce_general_rows_kernel(const float* __restrict__ in, const int64_t* __restrict__ y,
                                                              const float* __restrict__ t,
                                                              const float* __restrict__ weight, float eps,
                                                              float* __restrict__ din, int* __restrict__ bad_label,
                                                              float* __restrict__ terms, int B, int NC) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float keep = 1.f - eps, esc = eps / (float)NC;
  const bool smooth = eps > 0.f;
  const float D = PROB ? (float)B : label_weight_sum(y, weight, B, NC, lane);

  const float* r = in + (int64_t)b * NC;
  const float* tr = PROB ? t + (int64_t)b * NC : nullptr;
  // maximum and first arg-maximum of the scores (and of the probability targets); W where the smoothing term needs it
  float mx = -__builtin_inff(), tmx = -__builtin_inff(), W = 0.f;
  int am = 0x7fffffff, tam = 0x7fffffff;
  for (int j = lane; j < NC; j += 64) {
    const float v = r[j];
    if (v > mx) { mx = v; am = j; }
    if constexpr (PROB) {
      const float tv = tr[j];
      if (tv > tmx) { tmx = tv; tam = j; }
    } else if (smooth) {
      W += weight ? weight[j] : 1.f;
    }
  }
  wave_first_max(mx, am);
  if constexpr (PROB) wave_first_max(tmx, tam);
  else if (smooth) W = wave_sum(W);

  float s = 0.f;
  for (int j = lane; j < NC; j += 64) s += expf(r[j] - mx);
  s = wave_sum(s);
  // log-softmax as (r - max) - log(sum), torch's form: mx + log(sum) first would round at the magnitude of the logits
  const float ls = logf(s);

  // index: S = sum_c w_c (-logp_c) (smoothing only); probabilities: S = sum_c w_c t'_c (-logp_c), A = sum_c w_c t'_c
  float S = 0.f, A = 0.f;
  if (PROB || smooth) {
    for (int j = lane; j < NC; j += 64) {
      const float wj = weight ? weight[j] : 1.f;
      const float nlp = ls - (r[j] - mx);
      if constexpr (PROB) {
        const float wt = wj * (keep * tr[j] + esc);
        A += wt;
        S += wt * nlp;
      } else {
        S += wj * nlp;
      }
    }
    S = wave_sum(S);
    if constexpr (PROB) A = wave_sum(A);
  }

  if constexpr (PROB) {
    if (lane == 0) {
      terms[b] = S;
      terms[B + b] = (am == tam) ? 1.f : 0.f;
    }
    if (din) {
      float* d = din + (int64_t)b * NC;
      for (int j = lane; j < NC; j += 64) {
        const float wj = weight ? weight[j] : 1.f;
        d[j] = (expf((r[j] - mx) - ls) * A - wj * (keep * tr[j] + esc)) / D;
      }
    }
  } else {
    const int64_t yl = y[b];
    const bool ok = yl >= 0 && yl < NC;            // never index with a label outside [0, NC)
    const int yy = ok ? (int)yl : -1;
    const float hard = ok ? keep * (weight ? weight[yy] : 1.f) : 0.f;
    if (lane == 0) {
      if (!ok && yl != -100 && bad_label)
        *bad_label = yl >= 0 ? (int)min(yl, (int64_t)0x7ffffffe) + 1 : (int)max(yl, (int64_t)-0x7fffffff);
      terms[b] = ok ? hard * (ls - (r[yy] - mx)) + esc * S : 0.f;
      terms[B + b] = (am == yy) ? 1.f : 0.f;
    }
    if (din) {
      float* d = din + (int64_t)b * NC;
      const bool live = ok && D != 0.f;
      for (int j = lane; j < NC; j += 64) {
        float g = 0.f;
        if (live) {
          const float p = expf((r[j] - mx) - ls);
          g = hard * (p - (j == yy ? 1.f : 0.f));
          if (smooth) g += esc * (p * W - (weight ? weight[j] : 1.f));
          g /= D;
        }
        d[j] = g;
      }
    }
  }
}

// The per-row terms added in row order: 64 consecutive rows per trip (a wave sum), the trips one after another.
template <bool PROB>
__global__ __launch_bounds__(64) void ce_general_finish_kernel(const float* __restrict__ terms,
                                                               const int64_t* __restrict__ y,
                                                               const float* __restrict__ weight, float* __restrict__ loss,
                                                               int* __restrict__ ncorrect, int B, int NC) {
  const int lane = threadIdx.x;
  float tot = 0.f;
  int hits = 0;
  for (int b0 = 0; b0 < B; b0 += 64) {
    const int b = b0 + lane;
    tot += wave_sum(b < B ? terms[b] : 0.f);
    hits += (b < B && terms[B + b] != 0.f) ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) hits += __shfl_xor(hits, o, 64);
  const float D = PROB ? (float)B : label_weight_sum(y, weight, B, NC, lane);
  // no valid label, or labels whose weights add up to nothing: torch's 0 / 0
  if (lane == 0 && loss) *loss = D != 0.f ? tot / D : __builtin_nanf("");
  if (lane == 1 && ncorrect) *ncorrect += hits;
}

template <bool PROB>
int ce_general_launch(const float* in, const int64_t* y, const float* t, const float* weight, float eps, float* loss,
                      float* din, int* ncorrect, int* bad_label, float* ws, int B, int NC, hipStream_t st) {
  hipLaunchKernelGGL(ce_general_rows_kernel<PROB>, dim3(cdiv(B, 4)), dim3(256), 0, st, in, y, t, weight, eps, din,
                     bad_label, ws, B, NC);
  EAV_CHECK_LAUNCH("eav_ce_general_fwd_bwd");
  if (loss || ncorrect) {
    hipLaunchKernelGGL(ce_general_finish_kernel<PROB>, dim3(1), dim3(64), 0, st, ws, y, weight, loss, ncorrect, B, NC);
    EAV_CHECK_LAUNCH("eav_ce_general_fwd_bwd");
  }
  return EAV_OK;
}

}  // namespace

extern "C" int64_t eav_ce_general_ws_floats(int B) { return B > 0 ? 2 * (int64_t)B : 0; }

extern "C" int eav_ce_general_fwd_bwd(const float* in, const int64_t* y, const float* t, const float* weight,
                                      float label_smoothing, float* loss, float* din, int* ncorrect, int* bad_label,
                                      float* ws, int B, int NC, void* stream) {
  EAV_REQUIRE(in && ws && B > 0 && NC > 0 && NC <= EAV_HEAD_MAX_CLASSES && (int64_t)B * NC < (1ll << 31),
              "eav_ce_general_fwd_bwd: bad arguments (classes <= %d)", EAV_HEAD_MAX_CLASSES);
  EAV_REQUIRE((y != nullptr) != (t != nullptr),
              "eav_ce_general_fwd_bwd: exactly one of class indices and class probabilities must be given");
  EAV_REQUIRE(label_smoothing >= 0.f && label_smoothing <= 1.f, "eav_ce_general_fwd_bwd: label_smoothing %g outside [0, 1]",
              (double)label_smoothing);
  if (t) return ce_general_launch<true>(in, y, t, weight, label_smoothing, loss, din, ncorrect, bad_label, ws, B, NC,
                                        (hipStream_t)stream);
  return ce_general_launch<false>(in, y, t, weight, label_smoothing, loss, din, ncorrect, bad_label, ws, B, NC,
                                  (hipStream_t)stream);
}
