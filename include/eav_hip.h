/* libeav_hip.so - C ABI of the MI355X (gfx950) kernels behind the EAV trainer API.
 *
 * The reference (nubcico/EAV) has no native/FFI layer: its hot path is Python calling torch ops.
 * Each entry point below therefore names the *reference op call site* it replaces
 * (file:line under /root/reference).  The Python mirror of the reference's trainer classes
 * (eav_amd/eegnet.py, audio.py, vision.py) binds these with ctypes - see INTEGRATION.md.
 *
 * Conventions: every function returns 0 on success or a negative EAV_E* code (message from
 * eav_last_error(), thread-local).  All pointers are caller-owned DEVICE pointers unless said
 * otherwise; nothing is allocated inside; `stream` is a hipStream_t (NULL = default stream);
 * launches are asynchronous.  Tensors are dense, row-major, fp32 unless noted.
 * The only process-wide state are the eav_*_set_* tuning hooks of include/eav_hip_tuning.h (tile shape, resident-block caps;
 * test / benchmark use only, declared apart from this product ABI): plain globals read at
 * launch time, meant to be set once before work is issued (benchmarks / experiments), not synchronised across threads.
 */
#ifndef EAV_HIP_H
#define EAV_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EAV_ABI_VERSION 3

const char* eav_last_error(void);
int eav_abi_version(void);

/* ---- generic ------------------------------------------------------------------------------ */
/* out[i] = scale * sum_p part[p*stride + i], fp64 accumulation in fixed order (deterministic). */
int eav_reduce_partials(const float* part, int nparts, int64_t stride, int n, float scale, float* out, void* stream);

/* nn.BatchNorm2d forward statistics (EEGNet_tor.py:25,29,38).  part[p][0..nch) = sum x,
 * part[p][nch..2nch) = sum x^2.  Writes bn[0..nch)=mean, invstd, scale=gamma*invstd,
 * shift=beta-mean*scale as four separate arrays; training!=0 also updates the running stats
 * (momentum, unbiased variance); training==0 uses the running stats. */
int eav_bn_finalize(const float* part, int nparts, int nch, double count, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, int training, float momentum, float eps, float* mean,
                    float* invstd, float* scale, float* shift, void* stream);
/* BatchNorm backward sums -> dgamma, dbeta and the two means of the input-gradient formula. */
int eav_bn_bwd_finalize(const float* part, int nparts, int nch, double count, int training, float* dgamma,
                        float* dbeta, float* m1, float* m2, void* stream);
/* eav_reduce_partials(part, nparts, stride, n, 1, out) and one or two eav_bn_bwd_finalize jobs (part_b = NULL: one) in ONE
 * launch - the same arithmetic on disjoint block ranges, the same bits (autograd of EEGNet_tor.py:52-54: depthwiseConv.weight
 * and firstBN - and, in the eval-mode step, depthwiseBN - behind eav_eegnet_dw_bwd_fused). */
int eav_reduce_and_bn_bwd_finalize(const float* part, int nparts, int64_t stride, int n, float* out,
                                   const float* part_a, int nparts_a, int nch_a, double count_a, int training_a,
                                   float* dgamma_a, float* dbeta_a, float* m1_a, float* m2_a,
                                   const float* part_b, int nparts_b, int nch_b, double count_b, int training_b,
                                   float* dgamma_b, float* dbeta_b, float* m1_b, float* m2_b, void* stream);
/* weight.data.renorm_(p=2, dim=0, maxnorm) - the max-norm hooks, EEGNet_tor.py:33-34,47-48. */
int eav_renorm_rows(float* w, int rows, int cols, float maxnorm, void* stream);
/* both hooks of EEGNet_tor.forward (depthwiseConv.weight, dense.weight) in one launch */
int eav_renorm_rows2(float* w_a, int rows_a, int cols_a, float* w_b, int rows_b, int cols_b, float maxnorm,
                     void* stream);

/* ---- EEGNet block 1 ----------------------------------------------------------------------- */
/* firstConv forward: nn.Conv2d(1,8,(1,K<=300),padding='same',bias=False), EEGNet_tor.py:24,51.
 * x [B,C,S] -> y1 [B,8,C,S]; stat_part [eav_eegnet_fir_fwd_nparts()][16] = per-filter sum / sum sq. */
int eav_eegnet_fir_fwd_nparts(int B, int C, int S);
int eav_eegnet_fir_fwd(const float* x, const float* w1, float* y1, float* stat_part, int B, int C, int S, int klen,
                       void* stream);
/* No-grad evaluation of block 1 (Trainer_uni.validate, EEGNet_tor.py:118-135; model.eval(): BatchNorm on running
 * statistics, no dropout): x [B,C,S] (or rows xidx of a resident [*,C,S] array; xidx may be NULL) -> p2 [B,64,S/4] =
 * AvgPool(1,4)(ELU(depthwiseBN(depthwiseConv(ELU(firstBN(firstConv(x))))))) in one pass - the FIR output, its ELU and the
 * depthwise output never exist in memory.  bn1 / bn2: mean, invstd, scale, shift (8 / 64 floats each) as eav_bn_finalize
 * writes them in eval mode; w2 = depthwiseConv.weight [64,C].  C <= 32, S % 4 == 0, klen <= 300. */
int eav_eegnet_block1_infer(const float* x, const int64_t* xidx, const float* w1, const float* bn1, const float* w2,
                            const float* bn2, float* p2, int B, int C, int S, int klen, void* stream);
/* firstConv weight gradient fused with firstBN backward (autograd of EEGNet_tor.py:51-52):
 * bn_params = mean, invstd, scale, shift, m1, m2 (8 floats each); part [nparts][8][klen].
 * y1 == NULL: BatchNorm in eval mode (m1 = m2 = 0, the gradient through firstBN is scale * g1; y1 is not read). */
int eav_eegnet_fir_wgrad_nparts(int B, int C, int S);
int eav_eegnet_fir_wgrad(const float* x, const float* y1, const float* g1, const float* bn_params, float* part,
                         int B, int C, int S, int klen, void* stream);
/* The same two kernels with the batch addressed in place: sample b of the batch = row xidx[b] of x [*,C,S] (the
 * trainer's HBM-resident data set) - the per-step batch copy (EEGNet_tor.py:100-101: a host->device copy in the
 * reference, a device gather otherwise) disappears.  xidx: device int64 [B]; NULL = x is the batch. */
/* firstConv and its weight gradient by overlap-save FFT (csrc/eegnet_fir_fft.hip): the same exact-fp32 linear maps as
 * eav_eegnet_fir_fwd / eav_eegnet_fir_wgrad (nn.Conv2d(1, 8, (1, kernLength), padding='same', bias=False) and autograd's
 * weight gradient of it, CNN_torch/EEGNet_tor.py:24,51,109) in ~13 x fewer flops - HBM-bound instead of MFMA-bound; up to
 * eav_eegnet_fir_fft_max_taps() = 321 taps, any C / S.  xidx (optional): the batch is x[xidx[0..B)].
 * fwd: stat_part [eav_eegnet_fir_fwd_fft_nparts(B,C,S)][16] (8 sums, 8 sums of squares per row) for eav_bn_finalize; NULL:
 * no statistics are collected (firstBN in eval mode uses its running statistics).  Both sizes hold for every klen (short
 * row tails share a transform where klen lets them, which changes the grids); EVERY stat_part row is written.
 * wgrad: dW [8, klen] is WRITTEN (no partials to reduce); ws: eav_eegnet_fir_wgrad_fft_ws_floats(B,C,S) floats;
 * y1 = NULL selects BatchNorm in eval mode (dy = scale g).  Bit-reproducible run to run. */
int eav_eegnet_fir_fft_max_taps(void);
int eav_eegnet_fir_fwd_fft_nparts(int B, int C, int S);
int eav_eegnet_fir_fwd_fft(const float* x, const int64_t* xidx, const float* w1, float* y1, float* stat_part, int B, int C,
                           int S, int klen, void* stream);
int64_t eav_eegnet_fir_wgrad_fft_ws_floats(int B, int C, int S);
int eav_eegnet_fir_wgrad_fft(const float* x, const int64_t* xidx, const float* y1, const float* g1, const float* bn_params,
                             float* ws, float* dW, int B, int C, int S, int klen, void* stream);
/* The unit list and the grids of the two launchers above for a shape, from the functions they call themselves (host only):
 * out[EAV_FIR_FFT_PLAN_FIELDS] = npair (electrode pairs), nmb (whole-segment blocks per row), nmain (= B npair nmb units),
 * ntail (row tails that share transforms, 0: none), npk (= ceil(ntail / 2) packed units), t0t (first output of a packed
 * tail), the forward's workgroups (12 waves each), the weight gradient's groups of 8 units and its workgroups. */
#define EAV_FIR_FFT_PLAN_FIELDS 9
int eav_eegnet_fir_fft_plan(int B, int C, int S, int klen, int* out);
/* The train-mode weight gradient without its y1 read, for a data set that stays in HBM.  y1 = firstConv(x; w1), so its share
 * of dW is a function of x and w1:  dW[f,k] = scale_f (G[f,k] - (m1_f - mean_f invstd_f m2_f) X1[k] - invstd_f m2_f
 * sum_j w1[f,j] A[j,k]),  G = the eval-mode walk on the raw g1,  A = sum_b A_b,  X1 = sum_b X1_b,
 * A_b[j,k] = sum_c sum_{t<S} xp[t+j] xp[t+k],  X1_b[k] = sum_c sum_{t<S} xp[t+k]  (xp: the row padded as the convolution pads it).
 * xtab_build writes the tables of the N trials of x once per data set (tab: eav_eegnet_fir_xtab_floats(N, klen) floats; per
 * trial A_b [klen][klen], then X1_b [klen]; float64 sums rounded once, deterministic; about 361 KB per trial at 300 taps).
 * wgrad_fft_xtab: tab belongs to the array x points to - row xidx[b] (xidx NULL: b) is the table of sample b, repeated indices
 * count as often as they occur; ws: eav_eegnet_fir_wgrad_fft_xtab_ws_floats floats, 8-byte aligned.  Same number of launches
 * as eav_eegnet_fir_wgrad_fft; agrees with it to rounding (not bit for bit); bit-reproducible run to run. */
int64_t eav_eegnet_fir_xtab_floats(int N, int klen);
int eav_eegnet_fir_xtab_build(const float* x, int N, int C, int S, int klen, float* tab, void* stream);
int64_t eav_eegnet_fir_wgrad_fft_xtab_ws_floats(int B, int C, int S, int klen);
int eav_eegnet_fir_wgrad_fft_xtab(const float* x, const int64_t* xidx, const float* tab, const float* w1, const float* g1,
                                  const float* bn_params, float* ws, float* dW, int B, int C, int S, int klen, void* stream);
int eav_eegnet_fir_fwd_indexed(const float* x, const int64_t* xidx, const float* w1, float* y1, float* stat_part, int B,
                               int C, int S, int klen, void* stream);
int eav_eegnet_fir_wgrad_indexed(const float* x, const int64_t* xidx, const float* y1, const float* g1,
                                 const float* bn_params, float* part, int B, int C, int S, int klen, void* stream);
/* What eav_eegnet_fir_fwd / _wgrad / eav_eegnet_block1_infer (and their indexed forms) launch for rows of S samples and a
 * klen-tap kernel - the single statement of each selection rule, shared with the launchers (0 for arguments they reject):
 * FWD_NSTEP the MFMA K-steps of the forward / inference instantiation (34 / 66 / 152), FWD_NSEG the forward's work items per
 * (sample, electrode) row, WGRAD_NCHUNK / WGRAD_CH the weight gradient's items per row and their length, WGRAD_NT its
 * column tiles (2 / 4 / 10), INFER_NSEG the inference kernel's items per sample.  eav_eegnet_block1_infer_nblocks = its grid. */
enum { EAV_FIR_PLAN_FWD_NSTEP = 0, EAV_FIR_PLAN_FWD_NSEG = 1, EAV_FIR_PLAN_WGRAD_NCHUNK = 2, EAV_FIR_PLAN_WGRAD_CH = 3,
       EAV_FIR_PLAN_WGRAD_NT = 4, EAV_FIR_PLAN_INFER_NSEG = 5 };
int eav_eegnet_fir_plan(int S, int klen, int what);
int eav_eegnet_block1_infer_nblocks(int B, int S);
/* Thread geometry of eav_eegnet_dw_fwd(_pool_eval) and eav_eegnet_dw_bwd_fused(_eval) for rows of S samples, as CG * 1000 + NT
 * (channel groups x threads per block: 4256, 4512 or 1256; eav_eegnet_dw_bwd always runs 1256). */
int eav_eegnet_dw_plan(int S);
/* firstBN -> ELU -> depthwiseConv (EEGNet_tor.py:52-54): y1 -> z [B,64,S];
 * stat_part [B*ceil(S/1024)][128]. */
int eav_eegnet_dw_fwd(const float* y1, const float* bn1, const float* w2, float* z, float* stat_part, int B, int C,
                      int S, void* stream);
/* eav_eegnet_dw_fwd that also leaves p2 [B,64,S/4] = AvgPool(1,4)(ELU(depthwiseBN(z))) (EEGNet_tor.py:55-57) when
 * depthwiseBN is in EVAL mode: bn2 = its parameter block as eav_bn_finalize(training = 0) leaves it (scale / shift from the
 * running statistics, known before the launch); no dropout (identity in eval mode).  Saves eav_bn_elu_pool_fwd's pass over
 * z in the eval-mode training steps the reference runs from its second epoch on.  S % 4 == 0. */
int eav_eegnet_dw_fwd_pool_eval(const float* y1, const float* bn1, const float* w2, float* z, float* stat_part,
                                const float* bn2, float* p2, int B, int C, int S, void* stream);
/* backward of the above: g1 [B,8,C,S] = dL/d(firstBN out); stat_part [B*ceil(S/1024)][16];
 * w_part [B*ceil(S/1024)][64*C]. */
int eav_eegnet_dw_bwd(const float* y1, const float* dz, const float* bn1, const float* w2, float* g1,
                      float* stat_part, float* w_part, int B, int C, int S, void* stream);

/* the same with the backward of depthwiseBN -> ELU -> AvgPool(1,4) -> Dropout (EEGNet_tor.py:55-58) folded in: dz is
 * formed from z [B,64,S] and dp2 [B,64,S/4] on the fly (no eav_bn_elu_pool_bwd_apply launch, no dz tensor).
 * bn2 = mean, invstd, scale, shift, m1, m2 of depthwiseBN (64 floats each). */
int eav_eegnet_dw_bwd_fused(const float* y1, const float* z, const float* dp2, const float* bn2, const float* bn1,
                            const float* w2, float* g1, float* stat_part, float* w_part, int B, int C, int S,
                            float drop_p, uint64_t seed, const uint8_t* mask, const uint64_t* seed_dev, void* stream);

/* the same for an eval-mode step (depthwiseBN on its running statistics, what the reference's loop runs from its second
 * epoch on: model.eval() in validate(), EEGNet_tor.py:118, is never undone): dz = scale2 g needs no batch sums first, so the
 * sums themselves (the depthwiseBN weight / bias gradients) leave from this pass - bn2_part [B*ceil(S/1024)][2*64], finished
 * by eav_bn_bwd_finalize(training = 0) AFTER this launch; no eav_bn_elu_pool_bwd_reduce pass; bn2's m1 / m2 are not read. */
int eav_eegnet_dw_bwd_fused_eval(const float* y1, const float* z, const float* dp2, const float* bn2, const float* bn1,
                                 const float* w2, float* g1, float* stat_part, float* w_part, float* bn2_part, int B, int C,
                                 int S, float drop_p, uint64_t seed, const uint8_t* mask, const uint64_t* seed_dev,
                                 void* stream);

/* ---- BN -> ELU -> AvgPool(1,P) -> Dropout (EEGNet_tor.py:55-58, 60-63), P in {4,8} -------- */
/* bn = mean, invstd, scale, shift (CH each).  mask: optional uint8 keep-mask [B,CH,T/P]
 * (NULL = counter-based generator keyed by seed); drop_p = 0 disables dropout; drop_p < 0 = nn.Dropout2d with
 * probability -drop_p: one keep decision per (sample, channel) row (the reference's dropoutType != 'Dropout',
 * EEGNet_tor.py:21) - eav_bn_elu_pool_* and eav_eegnet_dw_bwd_fused. */
/* seed_dev (optional, device uint64): effective seed = seed + 2 * (*seed_dev) - a device-resident step counter,
 * so that a captured hipGraph draws a fresh mask on every replay. */
int eav_bn_elu_pool_fwd(const float* in, const float* bn, float* out, int B, int CH, int T, int P, float drop_p,
                        uint64_t seed, const uint8_t* mask, const uint64_t* seed_dev, void* stream);
int eav_bn_elu_pool_bwd_reduce(const float* dp, const float* u, const float* bn, float* part /*[B][2*CH]*/, int B,
                               int CH, int T, int P, float drop_p, uint64_t seed, const uint8_t* mask,
                               const uint64_t* seed_dev, void* stream);
int eav_bn_elu_pool_bwd_apply(const float* dp, const float* u, const float* bn, const float* m12 /*m1[CH],m2[CH]*/,
                              float* du, int B, int CH, int T, int P, float drop_p, uint64_t seed,
                              const uint8_t* mask, const uint64_t* seed_dev, void* stream);
/* BatchNorm on its running statistics (eval-mode step): du = scale g and the sums of eav_bn_elu_pool_bwd_reduce (part
 * [B][2*CH], to be finished by eav_bn_bwd_finalize(training = 0)) in ONE pass over u and dp. */
int eav_bn_elu_pool_bwd_eval(const float* dp, const float* u, const float* bn, float* du, float* part /*[B][2*CH]*/, int B,
                             int CH, int T, int P, float drop_p, uint64_t seed, const uint8_t* mask,
                             const uint64_t* seed_dev, void* stream);

/* ---- separableConv: dense 64->64, 16 taps, 'same' (EEGNet_tor.py:37,59) ------------------- */
int eav_conv64_prep_weights(const float* w /*[64,64,16]*/, float* wT_fwd /*[1024,64]*/, float* wT_bwd, void* stream);
/* eav_conv64_prep_weights and eav_counter_inc4 (the dropout / num_batches_tracked step counters; NULL = skip) in one
 * launch: the per-step prologue of EEGNet_tor.forward when the direct separableConv kernels run */
int eav_eegnet_step_prologue(const float* w, float* wT_fwd, float* wT_bwd, int64_t* c0, int64_t* c1, int64_t* c2,
                             int64_t* c3, void* stream);
int eav_conv64_ntiles(int T);
/* out[b,o,t] = sum wT[(i*16+k)][o]*in[b,i,t+k-padl]; stat_part (may be NULL) [eav_conv64_fwd_nparts()][128]. */
int eav_conv64_fwd_nparts(int B, int T);
/* output samples per work item of eav_conv64_fwd for this shape (32 or 128): the instantiation the launcher takes */
int eav_conv64_plan(int B, int T);
int eav_conv64_fwd(const float* in, const float* wT, float* out, float* stat_part, int B, int T, int padl,
                   void* stream);
/* separableConv and its data gradient in the frequency domain (csrc/eegnet_conv64_fft.hip): the same exact-fp32 linear maps
 * as eav_conv64_fwd with wT_fwd / wT_bwd (nn.Conv2d(64, 64, (1,16), padding='same', bias=False), CNN_torch/EEGNet_tor.py:37,59
 * and autograd's input gradient of it) by overlap-save blocks of 64 samples: per frequency bin the channel mixing is one
 * [128 x 128] real matrix - 6 x fewer multiply-adds than the 1024-deep direct contraction.  w = separableConv.weight
 * [64,64,16] (no prepared copy needed); bwd = 0 forward (stat_part [eav_conv64_fft_nparts(B,T)][128] or NULL), bwd = 1 data
 * gradient, bwd = 2 data gradient re-using the filter spectra the forward call of the same step prepared in ws; ws: eav_conv64_fft_ws_floats(B,T) floats, 16-byte aligned (it keeps the input spectra of both calls for the
 * weight gradient). */
int64_t eav_conv64_fft_ws_floats(int B, int T);
int eav_conv64_fft_nparts(int B, int T);
int eav_conv64_fft_fwd(const float* in, const float* w, float* out, float* stat_part, float* ws, int B, int T, int bwd,
                       void* stream);
/* dW [64,64,16] = d loss / d separableConv.weight, WRITTEN (replaces eav_conv64_wgrad + eav_reduce_partials); needs the
 * forward input's spectra of the same step in ws (eav_conv64_fft_fwd with bwd = 0 was called on it). */
int eav_conv64_fft_wgrad(const float* du, float* dW, float* ws, int B, int T, void* stream);
/* The separableConv backward of a step from ONE pack launch that writes both du spectra: dx = what eav_conv64_fft_fwd(bwd = 2)
 * gives and dW = what eav_conv64_fft_wgrad gives, bit for bit; ws as for those two (the forward call of the step was made on
 * it).  du != NULL: du [B,64,T] is read.  du == NULL: du is formed while loading - the backward of separableBN -> ELU ->
 * AvgPool(1,8) -> Dropout, i.e. eav_bn_elu_pool_bwd_apply(dp, u, bn, m12, ..., P = 8, drop_p, seed, mask, seed_dev) without
 * that launch and without the du tensor (dp [B,64,T/8], u [B,64,T], bn = mean, invstd, scale, shift, m12 = m1, m2). */
int eav_conv64_fft_bwd(const float* du, const float* dp, const float* u, const float* bn, const float* m12, float drop_p,
                       uint64_t seed, const uint8_t* mask, const uint64_t* seed_dev, float* dx, float* dW, float* ws, int B,
                       int T, void* stream);
int eav_conv64_wgrad_nparts(int B, int T);
/* part [nparts][64*64*16]; sum over parts = dL/dW[o,i,k]. */
int eav_conv64_wgrad(const float* du, const float* in, float* part, int B, int T, int padl, void* stream);

/* ---- canonical EEGNet (CNN_torch/CNN_EEG.py:7-67): run-time F1<=16, D<=8, F2<=64, K1<=1024, K2<=32, Chans<=256 -- */
/* block1[0] nn.Conv2d(1,F1,(1,K),padding='same',bias=False) (CNN_EEG.py:22): x [B,C,S] -> y1 [B,F1,C,S];
 * stat_part [eav_tconv_fwd_nparts()][2*F1] = per-filter sum / sum of squares (input of eav_bn_finalize).
 * F1 == 8 with K <= 300 runs the fp32-MFMA Toeplitz kernels of eav_eegnet_fir_* (nparts = eav_eegnet_fir_fwd_nparts);
 * other shapes a direct kernel with one row per (sample, electrode, 1024-sample tile): nparts = B*C*ceil(S/1024). */
int eav_tconv_fwd_nparts(int B, int C, int S, int F1, int K);
int eav_tconv_fwd(const float* x, const float* w, float* y1, float* stat_part, int B, int C, int S, int F1, int K,
                  void* stream);
/* its weight gradient with the block1[1] BatchNorm backward folded in; bn_params = mean, invstd, scale, shift,
 * m1, m2 (F1 each); part [eav_tconv_wgrad_nparts()][F1*K], nparts = min(B*C*ceil(S/512), 1024) for the direct kernel
 * (eav_eegnet_fir_wgrad_nparts for F1 == 8, K <= 300). */
int eav_tconv_wgrad_nparts(int B, int C, int S, int F1, int K);
int eav_tconv_wgrad(const float* x, const float* y1, const float* g1, const float* bn_params, float* part, int B,
                    int C, int S, int F1, int K, void* stream);
/* block1[1..2]: BatchNorm affine -> depthwise nn.Conv2d(F1,D*F1,(Chans,1),groups=F1) (CNN_EEG.py:23-25):
 * y1 -> z [B,D*F1,S]; stat_part [eav_spatial_nparts() = B*ceil(S/1024)][2*D*F1], row (b, tile).  elu != 0 puts an ELU
 * between the BatchNorm and the conv: firstBN -> ELU -> depthwiseConv of EEGNet_tor (EEGNet_tor.py:52-54) for widths the specialised
 * eav_eegnet_dw_* kernels do not cover. */
int eav_spatial_nparts(int B, int S);
int eav_spatial_fwd(const float* y1, const float* bn1, const float* wd, float* z, float* stat_part, int B, int C,
                    int S, int F1, int D, int elu, void* stream);
/* backward: g1 [B,F1,C,S] = dL/d(BN output); stat_part [nparts][2*F1]; w_part [nparts][D*F1*C]. */
int eav_spatial_bwd(const float* y1, const float* dz, const float* bn1, const float* wd, float* g1, float* stat_part,
                    float* w_part, int B, int C, int S, int F1, int D, int elu, void* stream);
/* Dense temporal conv nn.Conv2d(Cin,Cout,(1,K),padding='same',bias=False), K <= 16, channels <= 64: the
 * "separableConv" of EEGNet_tor (EEGNet_tor.py:37,59) at widths other than 64 -> 64 (those run eav_conv64_*).
 * in [B,Cin,T], w [Cout,Cin,K] -> out [B,Cout,T]; stat_part (or NULL) [eav_dconv_fwd_nparts() = B*ceil(T/64)][2*Cout],
 * row (b, tile) = per-channel sum / sum of squares.
 * transposed != 0: the data gradient - in = dL/dout [B,Cin,T] (Cin = the conv's OUTPUT
 * channels), out = dL/din [B,Cout,T], w = the forward weight [Cin,Cout,K]. */
int eav_dconv_fwd_nparts(int B, int T);
int eav_dconv_fwd(const float* in, const float* w, float* out, float* stat_part, int B, int Cin, int Cout, int T,
                  int K, int transposed, void* stream);
/* its weight gradient: part [B][Cout*Cin*K] (finish with eav_reduce_partials over the B rows). */
int eav_dconv_wgrad(const float* dy, const float* x, float* part, int B, int Cin, int Cout, int T, int K, void* stream);
/* block2[0..1]: depthwise (1,K2) 'same' conv then pointwise 1x1 conv (CNN_EEG.py:35-37): a [B,C2,T] ->
 * d3 [B,C2,T] (kept for the backward) and z [B,F2,T]; stat_part [eav_sepconv_fwd_nparts() = B*ceil(T/128)][2*F2],
 * row (b, tile).  C2 = D*F1 <= 64. */
int eav_sepconv_fwd_nparts(int B, int T);
int eav_sepconv_fwd(const float* a, const float* wdw, const float* wp, float* d3, float* z, float* stat_part, int B,
                    int C2, int F2, int T, int K2, void* stream);
/* pointwise backward: dd3 [B,C2,T] and w_part [eav_pointwise_bwd_nparts() = min(B*ceil(T/64), 512)][F2*C2]. */
int eav_pointwise_bwd_nparts(int B, int T);
int eav_pointwise_bwd(const float* du, const float* d3, const float* wp, float* dd3, float* w_part, int B, int C2,
                      int F2, int T, void* stream);
/* depthwise temporal conv backward: da [B,C2,T] and w_part [B][C2*K2]. */
int eav_dwt_bwd(const float* dd3, const float* a, const float* wdw, float* da, float* w_part, int B, int C2, int T,
                int K2, void* stream);

/* ---- head, loss, optimiser ---------------------------------------------------------------- */
/* nn.Linear + nn.Softmax(dim=1) (EEGNet_tor.py:65-66); logits or probs may be NULL. */
int eav_dense_softmax_fwd(const float* in, const float* w, const float* bias, float* logits, float* probs, int B,
                          int NF, int NC, void* stream);
/* probs != NULL: dout is dL/dprobs (softmax backward applied first); NULL: dout is dL/dlogits. */
int eav_dense_softmax_bwd(const float* dout, const float* probs, const float* in, const float* w, float* dw,
                          float* dbias, float* din, int B, int NF, int NC, void* stream);
/* nn.CrossEntropyLoss (mean) on [B,NC] rows + gradient (din may be NULL); *ncorrect += #argmax hits (may be NULL).
 * A class index outside [0,NC) never indexes anything: it is reported through *bad_label (device int, may be NULL;
 * label+1 for label >= 0, the label itself if negative) - torch raises at this point, the Python wrapper does too. */
int eav_ce_fwd_bwd(const float* in, const int64_t* y, float* loss, float* din, int* ncorrect, int* bad_label, int B,
                   int NC, void* stream);
/* The wide head (csrc/head_wide.hip): the same Linear and loss for more than 16 classes, exact fp32, no atomics - the
 * summation order is fixed by the shape, two runs give the same bits.  NF a multiple of 4 up to 1024, 1 <= NC <=
 * EAV_HEAD_MAX_CLASSES.  logits = in . w^T + bias. */
#define EAV_HEAD_MAX_CLASSES 32768
int eav_dense_wide_fwd(const float* in, const float* w, const float* bias, float* logits, int B, int NF, int NC,
                       void* stream);
/* dw = dlogits^T . in, dbias = column sums of dlogits, din = dlogits . w (din may be NULL: not computed).  ws: device
 * scratch of eav_dense_wide_bwd_ws_floats(B, NF, NC) floats (the class slices of din; may be NULL when that is 0). */
int64_t eav_dense_wide_bwd_ws_floats(int B, int NF, int NC);
int eav_dense_wide_bwd(const float* dlogits, const float* in, const float* w, float* dw, float* dbias, float* din,
                       float* ws, int B, int NF, int NC, void* stream);
/* eav_ce_fwd_bwd's contract (ignore_index -100, bad_label encoding, *ncorrect += hits with the first maximum winning a
 * tie, NaN when every row is ignored) with one wave per row; ws: eav_ce_wide_ws_floats(B) floats of device scratch. */
int64_t eav_ce_wide_ws_floats(int B);
int eav_ce_wide_fwd_bwd(const float* in, const int64_t* y, float* loss, float* din, int* ncorrect, int* bad_label,
                        float* ws, int B, int NC, void* stream);
/* The other two losses of HF's ForSequenceClassificationLoss (csrc/head_loss.hip), mean over all B * NC elements like torch's
 * defaults, laid out like eav_ce_wide_fwd_bwd (one wave per row, row sums in ws, added in row order: no atomics, two runs
 * give the same bits).  logits, targets fp32 [B,NC], 1 <= NC <= EAV_HEAD_MAX_CLASSES, B * NC < 2^31; targets are not
 * validated (torch accepts any float); loss, dlogits and nhits may each be NULL; ws: eav_head_loss_ws_floats(B) floats.
 * nn.BCEWithLogitsLoss: term max(x,0) - x t + log1p(exp(-|x|)), dlogits = (sigmoid(x) - t) / (B NC), *nhits += the number
 * of elements with (x > 0) == (t > 0.5).  nn.MSELoss: term (x - t)^2, dlogits = 2 (x - t) / (B NC). */
int64_t eav_head_loss_ws_floats(int B);
int eav_bce_logits_fwd_bwd(const float* logits, const float* targets, float* loss, float* dlogits, int* nhits, float* ws,
                           int B, int NC, void* stream);
int eav_mse_fwd_bwd(const float* logits, const float* targets, float* loss, float* dlogits, float* ws, int B, int NC,
                    void* stream);
/* torch.nn.functional.cross_entropy(in, target, weight=weight, label_smoothing=eps), mean reduction (csrc/head_ce_soft.hip),
 * laid out like eav_ce_wide_fwd_bwd: one wave per row, row terms in ws (eav_ce_general_ws_floats(B) floats) added in row order,
 * no atomics, two runs give the same bits.  Exactly one of y (class indices [B]) and t (fp32 class probabilities [B,NC], not
 * validated) is non-NULL; weight [NC] may be NULL (all 1); 0 <= label_smoothing <= 1; loss, din, ncorrect and bad_label may
 * each be NULL; 1 <= NC <= EAV_HEAD_MAX_CLASSES, B * NC < 2^31.  With W = sum_c w_c and logp = log-softmax(in):
 *   y:  D = sum over the valid rows (0 <= y < NC) of w[y_b];
 *       loss = [(1 - eps) sum_b w[y_b] (-logp[b,y_b]) + (eps / NC) sum_b sum_c w_c (-logp[b,c])] / D over the valid rows,
 *       din[b,j] = [(1 - eps) w[y_b] (p_j - [j == y_b]) + (eps / NC) (p_j W - w_j)] / D; -100 is ignored, any other label
 *       outside [0,NC) is treated the same way and reported through *bad_label (eav_ce_fwd_bwd's encoding); D == 0 (every row
 *       ignored, or labels whose weights add up to 0): NaN loss, zero din.
 *   t:  t' = (1 - eps) t + eps / NC;  loss = -sum_b sum_c w_c t'[b,c] logp[b,c] / B;
 *       din[b,j] = [p_j sum_c w_c t'_c - w_j t'_j] / B.
 * *ncorrect += the rows whose first arg-maximum of `in` is the label (y) / the first arg-maximum of the row of t. */
int64_t eav_ce_general_ws_floats(int B);
int eav_ce_general_fwd_bwd(const float* in, const int64_t* y, const float* t, const float* weight, float label_smoothing,
                           float* loss, float* din, int* ncorrect, int* bad_label, float* ws, int B, int NC, void* stream);
/* v[i] *= *scalar (device scalar): the upstream gradient applied to the stored d loss / d scores. */
int eav_scale_by_scalar(float* v, const float* scalar, int64_t n, void* stream);
/* torch.optim.Adam (decoupled=0) / AdamW (decoupled=1) update of one flat tensor; step >= 1.
 * step_dev (optional, device int64): take the step count from device memory instead (graph-capturable). */
int eav_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                  float eps, float weight_decay, int64_t step, int decoupled, const int64_t* step_dev, void* stream);
/* eav_adam_step on the gradient g * *gscale (device scalar, e.g. out2 + 1 of eav_grad_clip_finish): the product is rounded to
 * fp32 first, so p, m, v get the bits eav_adam_step gives a gradient tensor scaled beforehand; g itself is not written. */
int eav_adam_step_scaled(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                         float eps, float weight_decay, int64_t step, int decoupled, const int64_t* step_dev,
                         const float* gscale, void* stream);
/* ---- Global-norm gradient clipping and gradient accumulation (csrc/grad_clip.hip) ----
 * A job table is a device array of njobs rows of 2 int64 {pointer, element count}: fp32 ranges, 4-byte aligned at least.
 * Every job is cut into chunks of eav_grad_chunk_elems() elements from its own start; the chunks of job 0, job 1, ... are
 * numbered 0 .. nchunks - 1 with nchunks = the sum over the jobs of eav_grad_nchunks(element count), a host helper like the
 * other *_nparts (integer arithmetic, no pointer).  Chunk c is handled by one workgroup
 * and its fp64 sum of squares goes to partials[c] (nchunks doubles): no atomics, results independent of the grid, two runs
 * give the same bits.  All scalars that change from step to step (weight, scalar, out2) are device memory. */
int64_t eav_grad_chunk_elems(void);
int64_t eav_grad_nchunks(int64_t n);
/* partials[c] = sum over chunk c of (double)g * (double)g */
int eav_grad_sumsq(const void* jobs, int njobs, int64_t nchunks, double* partials, void* stream);
/* acc = first ? w g : fma(w, g, acc) with w = *weight, element by element over two tables of equal counts (jobs_g's are
 * used; first: the old contents of acc are not read).  partials (may be NULL): eav_grad_sumsq of the values just stored,
 * bit for bit what eav_grad_sumsq over jobs_acc gives afterwards. */
int eav_grad_fold(const void* jobs_g, const void* jobs_acc, int njobs, int64_t nchunks, const float* weight, int first,
                  double* partials, void* stream);
/* out2[0] = (float)sqrt(sum of the partials, fp64, fixed order); out2[1] = min(1, max_norm / (out2[0] + 1e-6f)), formed as
 * torch.nn.utils.clip_grad_norm_ forms it (NaN norm: NaN; infinite norm: 0).  max_norm > 0 (infinity allowed). */
int eav_grad_clip_finish(const double* partials, int64_t nchunks, float max_norm, float* out2, void* stream);
/* g *= *scalar in place over a job table; nothing is written when the scalar is exactly 1. */
int eav_scale_ranges(const void* jobs, int njobs, int64_t nchunks, const float* scalar, void* stream);
/* ---- Multi-tensor Adam / AdamW over a job table, learning-rate schedule on the device (csrc/adam_jobs.hip) ----
 * One optimiser step = eav_adam_jobs_begin + eav_adam_step_jobs however many tensors, learning rates, weight decays and
 * step counts there are; nothing is read back, every per-step scalar is device memory, so the pair can be captured.
 * A job row is EAV_ADAM_JOB_WORDS int64 words (80 bytes):
 *   0 p  1 g  2 m  3 v   fp32 ranges of `numel` elements, 4-byte aligned at least
 *   4 numel              > 0
 *   5 base_lr            the bits of a double
 *   6 step               pointer to the device int64 step count the job reads (its own entry of `counts`, or a count the
 *                        caller advances itself, e.g. the one a capturable optimiser shares with eav_adam_step)
 *   7 weight_decay       fp32 bits in the low half, high half 0
 *   8 lr | bc1 << 32     fp32 bits, written by eav_adam_jobs_begin
 *   9 bc2s               fp32 bits in the low half, written by eav_adam_jobs_begin
 * The schedule record is EAV_ADAM_SCHED_WORDS int64 words: 0 t = optimiser steps completed since the schedule was attached
 * (the caller zeroes it), 1 the factor of the last step (double), 2 (float)(report_lr * factor) of the last step (fp32, low
 * half: the rate a caller wants to show, e.g. its first group's), 3 unused.
 * The jobs are cut into chunks like a table of eav_grad_sumsq: eav_adam_jobs_nchunks(numel) chunks per job (the same
 * number as eav_grad_nchunks), nchunks = their sum. */
#define EAV_ADAM_JOB_WORDS 10
#define EAV_ADAM_SCHED_WORDS 4
#define EAV_SCHED_CONSTANT 0
#define EAV_SCHED_CONSTANT_WITH_WARMUP 1
#define EAV_SCHED_LINEAR 2
#define EAV_SCHED_COSINE 3
int64_t eav_adam_jobs_nchunks(int64_t n);
/* One workgroup.  counts[i] += 1 for i < ncounts (ncounts may be 0, counts then NULL); factor = the multiplier of
 * transformers.get_scheduler's lambda for `kind` at t = sched[0], in fp64 (W = warmup_steps, T = training_steps):
 *   t < W (every kind but constant): t / max(1, W);  constant, constant_with_warmup: 1;
 *   linear: max(0, (T - t) / max(1, T - W));  cosine: max(0, 0.5 (1 + cos(pi * num_cycles * 2 * (t - W) / max(1, T - W))));
 * then sched[0] += 1, and every row gets lr = (float)(base_lr * factor), bc1 = (float)(1 - beta1^step),
 * bc2s = (float)sqrt(1 - beta2^step) with the powers in fp64 - the expressions of eav_adam_step's step_dev branch - from the
 * step counts as they stand after the increments.  An unknown kind is refused before anything is launched. */
int eav_adam_jobs_begin(void* jobs, int njobs, int64_t* counts, int ncounts, void* sched, int kind, int64_t warmup_steps,
                        int64_t training_steps, double num_cycles, double report_lr, float beta1, float beta2, void* stream);
/* The update of every job, element by element what eav_adam_step (gscale NULL) / eav_adam_step_scaled (the gradient is
 * g * *gscale, rounded to fp32 first; g is not written) computes with the row's lr, weight_decay, bc1 and bc2s: the same
 * bits, whichever way a range is cut into jobs.  No atomics; results do not depend on the grid. */
int eav_adam_step_jobs(const void* jobs, int njobs, int64_t nchunks, float beta1, float beta2, float eps, int decoupled,
                       const float* gscale, void* stream);
/* ---- Weight averaging (EMA / SWA) inside the multi-tensor step (csrc/adam_jobs.hip) ----
 * The averaging record is EAV_ADAM_AVG_WORDS int64 words of device memory (an enumerator, not a macro):
 *   0 s   optimiser steps seen since averaging was attached (the caller zeroes it); the first step is s = 1
 *   1 n   n_averaged: how many steps have entered the average
 *   2 c | mode << 32     the fp32 coefficient of the current step (low half) and its EAV_AVG_* mode
 *   3 unused
 * eav_adam_jobs_begin_avg does everything eav_adam_jobs_begin does (same outputs, same bits) and, in the same workgroup,
 * s += 1 and the mode of this step: an averaging step is s >= start_step with (s - start_step) % every == 0;
 *   not an averaging step: EAV_AVG_SKIP, c = 0 - the averages are neither read nor written;
 *   averaging step, n == 0: EAV_AVG_COPY, c = 1 - avg = p bit for bit (AveragedModel.update_parameters' first call);
 *   else EAV_AVG_LERP with c = (float)(1 - d), d = decay or, avg_warmup != 0, min(decay, (1 + n) / (10 + n))  (EAV_AVG_EMA)
 *                       or c = (float)(1 / (n + 1))                                                            (EAV_AVG_SWA)
 * in fp64, rounded once; after a copy or lerp step n += 1. */
enum { EAV_ADAM_AVG_WORDS = 4 };
#define EAV_AVG_EMA 0
#define EAV_AVG_SWA 1
#define EAV_AVG_SKIP 0
#define EAV_AVG_COPY 1
#define EAV_AVG_LERP 2
int eav_adam_jobs_begin_avg(void* jobs, int njobs, int64_t* counts, int ncounts, void* sched, int kind, int64_t warmup_steps,
                            int64_t training_steps, double num_cycles, double report_lr, float beta1, float beta2,
                            void* avg_record, int avg_kind, double decay, int avg_warmup, int64_t start_step, int64_t every,
                            void* stream);
/* eav_adam_step_jobs over the same table - p, m and v come out with its bits - plus avgs[j], the device address (int64) of
 * job j's average range (fp32, `numel` elements, 4-byte aligned at least, 16-byte accesses where its own address allows).
 * Mode of avg_record word 2: skip touches no average; copy stores the new p; lerp stores fmaf(c, p_new - avg, avg). */
int eav_adam_step_jobs_avg(const void* jobs, const void* avgs, int njobs, int64_t nchunks, float beta1, float beta2, float eps,
                           int decoupled, const float* gscale, const void* avg_record, void* stream);
/* Exchanges the contents of the p and avgs[j] ranges of a table (words 0 and 4 of a row are read): a pure swap. */
int eav_swap_jobs(const void* jobs, const void* avgs, int njobs, int64_t nchunks, void* stream);
/* Batch assembly in HBM: out[i,:] = src[idx[i],:] (rows of row_elems floats) / out[i] = src[idx[i]] (labels).
 * Replaces the per-batch host->device copies of the reference loops (EEGNet_tor.py:100-101). */
int eav_gather_rows(const float* src, const int64_t* idx, float* out, int nrows, int64_t row_elems, void* stream);
int eav_gather_i64(const int64_t* src, const int64_t* idx, int64_t* out, int n, void* stream);
/* Batch assembly with augmentation (csrc/augment.hip): x is the split [N,R,C] (C contiguous; an AST clip is [time, mel], a
 * ViT frame [3,H,W] is [3 H, W]); record b of `table` (EAV_AUGMENT_RECORD_INTS int32 words: source i, partner j, the bits of
 * the fp32 lambda, flip flag, two row bands [r0,r1), two column bands [c0,c1)) describes out[b]:
 *   out[b,r,c] = fill inside any band, else lambda x[i,r,c'] + (1 - lambda) x[j,r,c'], c' = flip ? C - 1 - c : c.
 * lambda == 1 never reads the partner and hands the source's bits through (a record (i, *, 1.0, 0, empty bands) is
 * eav_gather_rows); empty, full-range and overlapping bands are legal; i and j are trusted like eav_gather_rows' indices.
 * tout [B,NC] (may be NULL; needs y, the split's int64 labels) = lambda onehot(y[i]) + (1 - lambda) onehot(y[j]), 1 where the
 * labels coincide.  16-byte accesses when C % 4 == 0, the grid sized by the batch's elements, no atomics. */
#define EAV_AUGMENT_RECORD_INTS 12
int eav_augment_gather(const float* x, const int64_t* y, const int32_t* table, float fill, float* out, float* tout, int B,
                       int R, int C, int NC, void* stream);
/* *counter += 1 on the stream (device-resident step counters for hipGraph replay). */
int eav_counter_inc(int64_t* counter, void* stream);
int eav_counter_inc4(int64_t* c0, int64_t* c1, int64_t* c2, int64_t* c3, void* stream);   /* distinct counters; NULL = skip */
/* The start of a captured training step in one launch (EEGNet_tor.py:100-104): up to five DISTINCT step counters + 1 (NULL =
 * skip: dropout stream, the three BatchNorm num_batches_tracked, the optimiser's step count) and out[i] = labels[idx[i]] for
 * i < n (n = 0: counters only). */
int eav_step_begin(int64_t* c0, int64_t* c1, int64_t* c2, int64_t* c3, int64_t* c4, const int64_t* labels,
                   const int64_t* idx, int64_t* out, int n, void* stream);

/* ---- AST / ViT encoders (HF ASTForAudioClassification / ViTForImageClassification as called at
 *      Transformer_Audio.py:22,72 and Transformer_Vision.py:29,92) ------------------------------ */
/* Batched fp32 GEMM on the fp32 matrix cores: C[z] = epilogue(alpha * opA(A[z]) . opB(B[z])).
 * transA=0: A is [M,K]; 1: A is [K,M].  transB=0: B is [N,K] (nn.Linear weight layout); 1: B is [K,N].
 * z = zb*heads + zh, operand z at base + zb*s?b + zh*s?h (element strides, multiples of 4).
 * Epilogue: +bias[n]; pre (optional) receives the value before GELU; gelu=1 applies erf-GELU; +resid;
 * accumulate=1 adds into C.  Replaces nn.Linear fwd/bwd, the patch-embedding conv (with eav_im2col),
 * Q.K^T, P.V and the attention backward products. */
int eav_gemm_f32(const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc,
                 int transA, int transB, int batch, int heads, int64_t sAb, int64_t sAh, int64_t sBb, int64_t sBh,
                 int64_t sCb, int64_t sCh, float alpha, const float* bias, int gelu, float* pre, const float* resid,
                 int ldr, int accumulate, void* stream);
/* The tile form eav_gemm_f32 launches for an [M,N] output over `batch` slabs, as BM * 1000 + BN (BM, BN in {64, 128}):
 * the single statement of the heuristic, shared with the launcher (0 for non-positive arguments). */
int eav_gemm_f32_plan(int M, int N, int batch);
/* Split-K form for weight gradients: C[M,N] = opA(A).opB(B) with the contraction cut into
 * eav_gemm_f32_splitk_plan(M,N,K) slices; ws holds [nsplit][M][N] partials, summed in fixed order.
 * eav_gemm_f32_splitk_nz = the slices that actually run (<= nsplit; the tile form is eav_gemm_f32_plan(M, N, nz));
 * eav_gemm_f32_splitk_reduce = the pass that sums them: 0 none (one slice, written to C), 1 plain, 2 wide (8 lanes per
 * float4 of a small output with many slices). */
int eav_gemm_f32_splitk_plan(int M, int N, int K);
int eav_gemm_f32_splitk_nz(int M, int N, int K);
int eav_gemm_f32_splitk_reduce(int M, int N, int K);
int eav_gemm_f32_splitk(const float* A, const float* B, float* C, float* ws, int M, int N, int K, int lda, int ldb,
                        int transA, int transB, void* stream);
/* fp32-grade GEMM on the fp16 matrix cores with split operands (csrc/gemm_sp.hip) - the same call sites as eav_gemm_f32
 * (nn.Linear forward / data gradient / weight gradient inside HF's ASTLayer / ViTLayer, Transformer_Audio.py:72,
 * Transformer_Vision.py:92).  Operands are "sp16 planes": X[R,K] with the contraction index along K stored as
 * uint16 [R][Kp/8][2][8] (8 hi halves, then 8 lo halves; Kp = eav_sp_kpad(K), zero beyond K) of sigma*X, hi =
 * fp16(sigma x), lo = fp16(sigma x - hi).  A device slot of EAV_SP_SLOT floats per tensor holds 64 shards of the bits of
 * max|x| (one per 128-byte line), sigma and 1/sigma: zero it, let producers atomicMax the shards
 * (eav_sp_absmax or a GEMM's amax_slot), then eav_sp_convert writes the planes of X (dst: contraction over columns)
 * and / or of X^T (dstT: contraction over rows) and fills sigma. */
#define EAV_SP_SLOT 4128   /* shard i at word 32*i (one 128-byte line each), sigma at word 2048, 1/sigma at 2049; words
                            * 2080.. : max|x| bits per 32-row block, 3104.. : boost exponent per 32-row block (1024 each; blocks alias beyond 32768 rows) */
int eav_sp_kpad(int K);
int eav_sp_absmax(const float* src, int R, int C, int64_t ld, float* slot, void* stream);
int eav_sp_convert(const float* src, int R, int C, int64_t ld, float* slot, void* dst, void* dstT, void* stream);
/* planes of GELU(src): src = pre-activations written by eav_gemm_sp with gelu = 3, slot = max |GELU(src)| */
int eav_sp_convert_gelu(const float* src, int R, int C, int64_t ld, float* slot, void* dst, void* dstT, void* stream);
/* the same pass also emitting bias-gradient partials: colsum_part [eav_sp_convert_colsum_nparts(R)][C] (column sums of
 * 64-row tiles; finish with eav_reduce_partials) */
int eav_sp_convert_colsum_nparts(int R);
int eav_sp_convert_colsum(const float* src, int R, int C, int64_t ld, float* slot, void* dst, void* dstT,
                          float* colsum_part, void* stream);
/* eav_sp_absmax + eav_sp_convert for a whole table of dense matrices in two launches (the weight refresh of an encoder
 * after an optimiser step: 49 matrices).  jobs: n entries in DEVICE memory; slots zeroed by the caller; every C % 4 == 0,
 * sources 16-byte aligned; maxR / maxC = the largest R and C in the table. */
typedef struct EavPlaneJob {
  const float* src;   /* [R, C] dense fp32 */
  void* dst;          /* planes [R][Cp/8][2][8] or NULL */
  void* dstT;         /* planes of the transpose [C][Rp/8][2][8] or NULL */
  float* slot;        /* EAV_SP_SLOT floats */
  int R, C;
} EavPlaneJob;
int eav_sp_refresh_planes(const void* jobs, int n, int maxR, int maxC, void* stream);
/* producers that also accumulate max|output| into an operand-scale slot (zeroed by the caller).  Both LayerNorm forward forms
 * that take a slot (amax_slot here, scale_slot of eav_layernorm_fwd_planes) ALSO WRITE max(rstd) into word 1 of the slot's 64
 * shard lines (atomicMax of the float bits): the slot is an output of the forward in that respect even where it is declared
 * const, and eav_layernorm_bwd_planes / _bound read it through slot_rstd (a slot whose word 1 is still zero is not trusted:
 * the backward then walks rstd[M]). */
int eav_layernorm_fwd_amax(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                           int M, int D, float eps, float* amax_slot, void* stream);
int eav_layernorm_bwd_amax(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                           float* dx, int accumulate, float* part, int M, int D, float* amax_slot, void* stream);
/* eav_layernorm_bwd_amax whose stored value (dx after the accumulation) also leaves as the row planes [M][Dp/8][2][8] of the
 * gradient products that consume it - no conversion pass over the residual-stream gradient (modeling_vit.py /
 * modeling_audio_spectrogram_transformer.py layernorm_before / layernorm_after backward through HF autograd) - scaled by
 * slot's sigma = the rigorous bound of eav_layernorm_bwd_bound, which the kernel forms itself when slot_dy is given (every
 * workgroup from the same slot words, published in slot by the first; a separate one-block launch queued 15-40 us behind the
 * persistent GEMMs) or which a call of eav_layernorm_bwd_bound put there before (slot_dy NULL):
 * max|dx_old| + (2 + sqrt(D)) max|gamma| max(rstd) max|dy| (slot_old: shards of the measured max|dx_old| or NULL; slot_dy:
 * shards of max|dy|; max(rstd) from slot_rstd - the scale slot the forward LayerNorm launch had, whose shard lines carry it in
 * word 1 - or, slot_rstd NULL, from a walk over rstd[M]).  part is [nparts][3 D]: dgamma | dbeta | column sums of the stored value (a bias gradient).  slot's
 * shards receive the measured maximum of the stored value. */
int eav_layernorm_bwd_planes(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                             float* dx, int accumulate, float* part, int M, int D, float* slot, void* planes,
                             const float* slot_old, const float* slot_dy, const float* slot_rstd, void* stream);
int eav_layernorm_bwd_bound(float* slot_out, const float* slot_old, const float* slot_dy, const float* gamma,
                            const float* rstd, int M, int D, const float* slot_rstd, void* stream);
int eav_gelu_bwd_amax(float* dact, const float* pre, int64_t n, float* amax_slot, void* stream);
/* C[z][m,n] = epilogue(alpha * sum_k A[z][m,k] B[n,k]) from planes A [M,Kp], B [N,Kp]; epilogue as eav_gemm_f32
 * (bias, erf-GELU with pre-activation store, residual, accumulate); amax_slot (optional) receives max |C| bits.
 * gelu = 2: backward through GELU - the product is multiplied by gelu'(pre[m,n]), `pre` (ldc) is READ (the forward's
 * stored pre-activation): fc2's data gradient and eav_gelu_bwd in one pass.
 * gelu = 3: C receives the pre-activation itself and amax_slot max |GELU(C)| - the activation is formed by
 * eav_sp_convert_gelu while it splits (no fp32 activation tensor); pre / resid / accumulate must be unset. */
int eav_gemm_sp(const void* A, const void* B, float* C, const float* slotA, const float* slotB, int M, int N, int K,
                int ldc, int batch, int64_t sA_bytes, int64_t sC, float alpha, const float* bias, int gelu, float* pre,
                const float* resid, int ldr, int accumulate, float* amax_slot, void* stream);
/* eav_gemm_sp that also - or only (C = NULL) - writes the stored value (after the activation) as the row planes
 * [M][Np/8][2][8] of the NEXT product, scaled by planes_slot[EAV_SLOT sigma]: no fp32 activation tensor, no conversion
 * pass.  The scale must be known before the launch: eav_tf_forward_scales derives it from a rigorous bound of |output|.
 * N % 8 == 0, batch 1.  (fc1 of HF's ASTMLP / ViTMLP: bias + erf-GELU, pre-activation kept in `pre` for the backward.) */
int eav_gemm_sp_planes(const void* A, const void* B, float* C, const float* slotA, const float* slotB, int M, int N, int K,
                       int ldc, int batch, int64_t sA_bytes, int64_t sC, float alpha, const float* bias, int gelu,
                       float* pre, const float* resid, int ldr, int accumulate, float* amax_slot, void* planes_out,
                       const float* planes_slot, void* stream);
/* nn.LayerNorm whose output leaves as the row planes of the product that consumes it (y optional, may be NULL);
 * scale_slot as above; D % 8 == 0. */
int eav_layernorm_fwd_planes(const float* x, const float* gamma, const float* beta, float* y, void* planes,
                             const float* scale_slot, float* mean, float* rstd, int M, int D, float eps, void* stream);
/* max over the rows of ||w_r||_2 into *out (float bits combined with atomicMax: zero it first) */
int eav_rownorm_max(const float* w, int R, int C, int64_t ld, float* out, void* stream);
/* the same over the COLUMNS of w [R, C] (C, ld multiples of 4) */
int eav_colnorm_max(const float* w, int R, int C, int64_t ld, float* out, void* stream);
/* A table of eav_rownorm_max / eav_colnorm_max jobs in one launch: jobs = device array of njobs rows of 5 int64
 * {w, ld, out, R | C << 32, cols} (cols 0: max row norm, 1: max column norm; outputs zeroed by the caller), max_blocks >=
 * the largest job's block count (rows: min(ceil(R / 4), 128); columns: ceil(C / 64)).  The weight refresh after an optimiser
 * step forms all the norms behind the a-priori operand scales with it. */
int eav_norm_max_multi(const void* jobs, int njobs, int max_blocks, void* stream);
/* sigma, 1/sigma of slot_out from the bound  factor * max|x| * *norm  (max|x| = the maximum held by amax_slot's shards, norm a
 * device scalar): the operand scale of a tensor BEFORE it is produced, so that its producer can write planes directly.
 * Used for the MLP hidden-state gradient dact = (dh W2) o gelu'(pre): |dact| <= 1.13 sqrt(D) max|dh| max_j ||W2[:,j]||_2. */
int eav_sp_bound_scale(float* slot_out, const float* amax_slot, const float* norm, float factor, void* stream);
/* sigma, 1/sigma of the operand slots of LayerNorm-before output (k_y1), LayerNorm-after output (k_y2) and the MLP's GELU
 * output (k_act) of `layers` encoder layers from rigorous bounds: |LN out| <= sqrt(D) max|gamma| + max|beta|,
 * |GELU(y2 W1^T + b1)| <= (sqrt(D) max|gamma2| + ||beta2||_2) max_n ||W1_n||_2 + max|b1|.  params: first float of layer 0
 * in the flat parameter buffer, layer_stride floats per layer, off_*: offsets of layernorm_before.{weight,bias},
 * layernorm_after.{weight,bias}, mlp.fc1.bias within a layer; wnorm_fc1 [layers]: eav_rownorm_max of mlp.fc1.weight;
 * slots: layer 0's first forward slot, slot_stride floats per layer. */
int eav_tf_forward_scales(const float* params, int64_t layer_stride, int layers, int off_g1, int off_b1, int off_g2,
                          int off_b2, int off_bfc1, int D, int FF, const float* wnorm_fc1, float* slots,
                          int64_t slot_stride, int k_y1, int k_y2, int k_act, void* stream);
int eav_tf_forward_scales_qkv(const float* params, int64_t layer_stride, int layers, int off_g1, int off_b1, int off_g2,
                              int off_b2, int off_bfc1, int off_bqkv, int D, int FF, const float* wnorm_fc1,
                              const float* wnorm_qkv, float* slots, int64_t slot_stride, int k_y1, int k_y2, int k_act,
                              int k_qkv, void* stream);
/* long-contraction form (weight gradients): C[M,N] = sum_t A[t,m] B[t,n] over ROW planes A [Tp][Mp/8][2][8], B
 * [Tp][Np/8][2][8] - the contraction runs over the rows (tokens), read with transposing LDS loads; Tp = T rounded up to
 * 32 and the rows >= T must be ZERO.  eav_gemm_sp_splitk_plan(M,N,T) token slices, ws [nsplit][M][N] partials summed in
 * fixed order (deterministic); C[M,N] dense (ldc = N). */
int eav_gemm_sp_splitk_plan(int M, int N, int K);
int eav_gemm_sp_splitk(const void* A, const void* B, float* C, float* ws, const float* slotA, const float* slotB, int M,
                       int N, int T, int accumulate, void* stream);
/* One-term forms: the hi.hi product alone - the operands rounded to fp16 under the planes' scales (11-bit mantissas, fp32
 * accumulation), a third of the matrix work on the SAME planes, same epilogues.  The opt-in precision of the backward
 * products (Encoder.grad_terms = 1): gradients then carry ~2^-11 relative rounding per operand, the forward (logits)
 * stays on the three-term product unless Encoder.fwd_terms = 1 asks for the plain fp16 forward as well (comparison leg of
 * bench.py: 16-bit matrix operands everywhere, as BASELINE.json's configs name them). */
int eav_gemm_sp_x1(const void* A, const void* B, float* C, const float* slotA, const float* slotB, int M, int N, int K,
                   int ldc, int batch, int64_t sA_bytes, int64_t sC, float alpha, const float* bias, int gelu, float* pre,
                   const float* resid, int ldr, int accumulate, float* amax_slot, void* stream);
/* eav_gemm_sp_planes with option flags */
#define EAV_GEMM_ONE_TERM 1    /* the hi.hi term alone */
#define EAV_GEMM_PLANES_NOLIFT 4 /* planes_out with lo = fp16(sigma x - hi), no 2^11 lift: the row planes the fused attention
                                  * reads (the fused q/k/v projection writes them directly, scale from eav_tf_forward_scales_qkv) */
#define EAV_GEMM_NO_BLOCKMAX 8  /* amax_slot receives the tensor-wide maximum only, no 32-row block entries: for outputs whose
                                 * consumer takes one scale per tensor (the attention operand preparation of dO) */
#define EAV_GEMM_SHARED_GPU 2  /* a second persistent GEMM runs beside this one (the backward's data gradients next to the
                                * side stream's weight gradients): prefer the 256 x 128 one-workgroup-per-CU form */
/* colsum_part (optional): [ceil(M / 64)][N], row p = column sums of the stored value over rows [64 p, 64 p + 64) - bias-gradient
 * partials for eav_reduce_partials; batch 1. */
int eav_gemm_sp_ex(const void* A, const void* B, float* C, const float* slotA, const float* slotB, int M, int N, int K,
                   int ldc, int batch, int64_t sA_bytes, int64_t sC, float alpha, const float* bias, int gelu, float* pre,
                   const float* resid, int ldr, int accumulate, float* amax_slot, void* planes_out,
                   const float* planes_slot, float* colsum_part, int flags, void* stream);
int eav_gemm_sp_splitk_x1(const void* A, const void* B, float* C, float* ws, const float* slotA, const float* slotB, int M,
                          int N, int T, int accumulate, void* stream);
/* eav_gemm_sp_splitk on TWO terms, hi_A.hi_B + lo_A.hi_B: operand B rounded to fp16 (its lo pieces are not read), operand A
 * at full split precision.  For weight gradients with A = the gradient tensor and B = the activation (autograd of
 * Transformer_Audio.py:74-79 / Transformer_Vision.py:94-99 through the HF nn.Linear layers): two thirds of the matrix work. */
int eav_gemm_sp_splitk_x2(const void* A, const void* B, float* C, float* ws, const float* slotA, const float* slotB, int M,
                          int N, int T, int accumulate, void* stream);
/* (the process-global tile / slice-count overrides the kernel benchmarks use are NOT part of this header: eav_hip_tuning.h) */
/* The same fused attention on the fp16 matrix cores with split operands (csrc/attention_sp.hip; fp32-grade, 3 MFMAs per
 * product).  eav_attn_sp_prep converts an fp32 activation src [B*N, ncols] (qkv or dO; slot holds its max|x| shards, see
 * EAV_SP_SLOT) into row planes [B*N][ncols/8][2][8] f16 and, for the column sections (of secw columns) selected by
 * tmask, per-head transposed planes [B][ncols/64][64][Npad/8][2][8] (Npad = eav_attn_sp_npad(N), zero beyond N); here
 * lo = fp16(sigma x - hi) without the 2^11 lift of the GEMM planes.  amax_slot (optional) receives max|output| shards. */
int eav_attn_sp_npad(int N);
int eav_attn_sp_prep(const float* src, float* slot, void* rowp, void* tp, int B, int N, int ncols, int secw,
                     unsigned tmask, void* stream);
/* Since round 3 the three attention kernels take their token-contracting operands (V in the forward, K in the dQ kernel,
 * Q and dO in the dK,dV kernel) from the ROW tiles with transposing LDS reads (ds_read_b64_tr_b16): the transposed planes
 * `tp` / `dotp` are not read any more and may be NULL (the parameters stay for binary compatibility; eav_attn_sp_prep
 * still writes them on request). */
int eav_attn_fwd_sp(const void* rowp, const void* tp, const float* slot, float* ao, float* lse, float* amax_slot, int B,
                    int H, int N, int head_dim, float scale, void* stream);
/* the same, the output also - or only (ao = NULL: forward-only passes) - as the GEMM operand planes [B*N][D/8][2][8] of the
 * o-proj products (lo lifted by 2^11 like eav_sp_convert's), scaled with qkv's own sigma (O is a convex combination of V
 * rows: |O| <= max|V| <= max|qkv|), which the kernel copies into ao_slot: no conversion pass for the attention output. */
int eav_attn_fwd_sp_planes(const void* rowp, const void* tp, const float* slot, float* ao, float* lse, float* amax_slot,
                           void* ao_planes, float* ao_slot, int B, int H, int N, int head_dim, float scale, void* stream);
/* dorow / dotp: planes of dO [B*N, H*64]; slot_ds: zeroed scratch slot (max|dS| travels from the dQ to the dK,dV kernel);
 * ao, dout: fp32 O and dO for delta = rowsum(dO o O); delta: scratch [B*H, N]; dqkv [B*N, 3*H*64] fp32. */
int eav_attn_bwd_sp(const void* rowp, const void* tp, const void* dorow, const void* dotp, const float* slot,
                    const float* slot_do, float* slot_ds, const float* ao, const float* dout, const float* lse,
                    float* delta, float* dqkv, float* amax_slot, int B, int H, int N, int head_dim, float scale,
                    void* stream);
/* eav_attn_bwd_sp that also (or only: dqkv = NULL) writes dqkv as the operand planes [B*N][3D/8][2][8] of the q/k/v
 * projection's gradient products - no fp32 dqkv, no conversion pass - scaled by a sigma the kernels form themselves and
 * publish in planes_slot (eav_attn_dqkv_bound computes the same number stand-alone) from a rigorous bound |dqkv| <= N max|dO| max(1, 128 scale max|qkv|^2) (slot_do: the
 * shards of max|dO|; slot_qkv: the forward's qkv slot); colsum_part (optional) [B * ceil(N/32)][3D] receives the column sums
 * of every 32-row tile (bias-gradient partials: finish with eav_reduce_partials).  ao_planes + ao_slot (optional): the attention
 * output as the planes eav_attn_fwd_sp_planes wrote - delta = dO . O then comes from planes and ao / dout may be NULL (the
 * training step keeps no fp32 attention output).  Replaces, in the split step, the
 * eav_sp_convert_colsum pass over dqkv (Transformer_Audio.py:72 / Transformer_Vision.py:92 through HF's backward). */
int eav_attn_dqkv_bound(float* slot_out, const float* slot_do, const float* slot_qkv, int N, float scale, void* stream);
int eav_attn_bwd_sp_planes(const void* rowp, const void* tp, const void* dorow, const void* dotp, const float* slot,
                           const float* slot_do, float* slot_ds, const float* ao, const float* dout, const float* lse,
                           float* delta, float* dqkv, float* amax_slot, void* planes, float* planes_slot,
                           float* colsum_part, const void* ao_planes, const float* ao_slot, int B, int H, int N,
                           int head_dim, float scale, void* stream);
/* Fused multi-head self-attention (head_dim 64), exact fp32 MFMA, flash-style: softmax(Q K^T scale) V per
 * (image, head) of qkv [B*N, 3*H*64] (HF eager_attention_forward).  ao [B*N, H*64]; lse [B*H, N] saved for
 * the backward. */
int eav_attn_fwd(const float* qkv, float* ao, float* lse, int B, int H, int N, int head_dim, float scale,
                 void* stream);
/* Backward of eav_attn_fwd: dqkv [B*N, 3*H*64] <- (dQ | dK | dV) from dout [B*N, H*64]; ao / lse as produced by
 * the forward; delta: scratch [B*H, N]. */
int eav_attn_bwd(const float* qkv, const float* ao, const float* dout, const float* lse, float* delta, float* dqkv,
                 int B, int H, int N, int head_dim, float scale, void* stream);
/* The attention probabilities of the fused kernels after the fact (csrc/attn_probs.hip; HF output_attentions=True):
 * P[b, h, q, k] = exp(scale q.k - lse[b, h, q]) from the operands the layer's attention kernel consumed - qkv [B*N, 3*H*64]
 * fp32 (eav_attn_fwd), or the row planes and scale slot of eav_attn_sp_prep / the plane-writing q/k/v projection
 * (eav_attn_fwd_sp) - and the lse [B*H, N] it wrote; the scores are formed as that precision's kernels form them.
 * probs [B, H, N, N] and probs_mean [B, N, N] (the mean over heads, summed in head order inside one workgroup) are fp32;
 * either may be NULL, not both.  head_dim must be 64.  Deterministic: the same bits on every run. */
int eav_attn_probs(const float* qkv, const float* lse, float* probs, float* probs_mean, int B, int H, int N, int head_dim,
                   float scale, void* stream);
int eav_attn_probs_sp(const void* rowp, const float* slot, const float* lse, float* probs, float* probs_mean, int B, int H,
                      int N, int head_dim, float scale, void* stream);
/* One step of attention rollout (Abnar & Zuidema 2020) for R readout rows: r_out[b, r, k] = 0.5 sum_q r_in[b, r, q]
 * abar[b, q, k] + 0.5 r_in[b, r, k]; r [B, R, N], abar [B, N, N] (a layer's head mean), fp32, q summed in ascending order.
 * r_out must not alias r_in. */
int eav_rollout_step(const float* r_in, const float* abar, float* r_out, int B, int R, int N, void* stream);
/* The same with attention-probability dropout 0 < drop_p < 1 (HF attention_probs_dropout_prob, training mode): the keep
 * decision of element (b, h, q, key) is a pure function of (seed + 2 * *seed_dev, ((b H + h) N + q) N + key) - or the
 * byte of an explicit uint8 keep-mask [B, H, N, N] - so no mask is stored: the backward kernels regenerate it and must
 * be given the forward's (drop_p, seed, mask, *seed_dev).  ao receives the dropped output (M o P / (1 - p)) V; lse holds
 * the statistics of the undropped scores. */
int eav_attn_fwd_dropout(const float* qkv, float* ao, float* lse, int B, int H, int N, int head_dim, float scale,
                         float drop_p, uint64_t seed, const uint8_t* mask, const uint64_t* seed_dev, void* stream);
int eav_attn_bwd_dropout(const float* qkv, const float* ao, const float* dout, const float* lse, float* delta,
                         float* dqkv, int B, int H, int N, int head_dim, float scale, float drop_p, uint64_t seed,
                         const uint8_t* mask, const uint64_t* seed_dev, void* stream);
/* Split-operand fused attention with attention-probability dropout (csrc/attention_sp.hip): same mask addressing; fp32
 * outputs only (ao with max|O| into amax_slot, dqkv with its maximum into amax_slot) - the fused-plane forms, whose
 * a-priori bounds assume rows of P sum to 1, are not offered with dropout.  rowp / dorow: row planes of qkv / dO
 * (eav_attn_sp_prep), slot / slot_do their scale slots, slot_ds a zeroed scratch slot. */
int eav_attn_fwd_sp_dropout(const void* rowp, const float* slot, float* ao, float* lse, float* amax_slot, int B, int H,
                            int N, int head_dim, float scale, float drop_p, uint64_t seed, const uint8_t* mask,
                            const uint64_t* seed_dev, void* stream);
int eav_attn_bwd_sp_dropout(const void* rowp, const void* dorow, const float* slot, const float* slot_do, float* slot_ds,
                            const float* ao, const float* dout, const float* lse, float* delta, float* dqkv,
                            float* amax_slot, int B, int H, int N, int head_dim, float scale, float drop_p, uint64_t seed,
                            const uint8_t* mask, const uint64_t* seed_dev, void* stream);
/* Encoder dropout sites (emb, attn_out, mlp_out) and the materialised-score attention path (csrc/tf_dropout.hip).
 * eav_tf_dropout_mask writes the uint8 keep-mask the generator produces for (drop_p, seed, *seed_dev) over n elements.
 * eav_tf_dropout_add: out = resid + Dropout(y) over n floats (n % 4 == 0; resid NULL: out = Dropout(y), the gate of the
 * backward; out may be y).  eav_softmax_dropout_fwd: softmax in place over s (kept undropped for the Jacobian) and
 * pd = M o P / (1 - p) for the P.V product; element (row, c) draws with index row * N + c.  eav_softmax_dropout_bwd:
 * dS = P o (M o dP / (1 - p) - rowsum) in place over dP, and (pd not NULL) the forward's pd again for dV = pd^T dO. */
int eav_tf_dropout_mask(uint8_t* mask, int64_t n, float drop_p, uint64_t seed, const uint64_t* seed_dev, void* stream);
int eav_tf_dropout_add(const float* y, const float* resid, float* out, int64_t n, float drop_p, uint64_t seed,
                       const uint8_t* mask, const uint64_t* seed_dev, void* stream);
int eav_softmax_dropout_fwd(float* s, float* pd, int64_t rows, int N, int ld, float drop_p, uint64_t seed,
                            const uint8_t* mask, const uint64_t* seed_dev, void* stream);
int eav_softmax_dropout_bwd(const float* P, float* dP, float* pd, int64_t rows, int N, int ld, float drop_p,
                            uint64_t seed, const uint8_t* mask, const uint64_t* seed_dev, void* stream);
/* nn.LayerNorm(D, eps) forward over M rows; mean/rstd [M] saved for the backward (may be NULL). */
int eav_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                      int M, int D, float eps, void* stream);
int eav_layernorm_bwd_nparts(int M);
/* dx (accumulate=1: dx += ...) and per-block partials part[nparts][2*D] = (dgamma, dbeta); part may be NULL. */
int eav_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                      float* dx, int accumulate, float* part, int M, int D, void* stream);
/* softmax over rows of length N (leading dimension ld), in place; backward dS = P o (dP - sum dP*P) in place on dP. */
int eav_softmax_fwd(float* s, int64_t rows, int N, int ld, void* stream);
int eav_softmax_bwd(const float* P, float* dP, int64_t rows, int N, int ld, void* stream);
/* dact *= GELU'(pre) (exact erf form, HF GELUActivation), in place. */
int eav_gelu_bwd(float* dact, const float* pre, int64_t n, void* stream);
/* bias gradient: part[eav_colsum_nparts(M)][N] partial column sums of dy [M,N]. */
int eav_colsum_nparts(int M);
int eav_colsum(const float* dy, float* part, int M, int N, int ld, void* stream);
/* patch extraction for the Conv2d patch embedding (HF AST :53-61 with transposed=1, HF ViT :60-69). */
int eav_im2col(const float* x, float* col, int B, int C, int H, int W, int P, int sy, int sx, int transposed,
               void* stream);
/* h[b,t] = (t<nextra ? token_t : h[b,t]) + pos[t]  (HF AST :93-97, ViT :146-157) and its backward. */
int eav_embed_finish(float* h, const float* cls, const float* dist, const float* pos, int B, int ntok, int D,
                     int nextra, void* stream);
int eav_embed_bwd(const float* dh, float* dpos, float* demb, int B, int ntok, int D, int nextra, void* stream);
/* Patch dropout (timm.layers.PatchDropout; csrc/patch_keep.hip): a training forward keeps K of the P patches of every sample
 * and the readout tokens.  All five kernels are in gather form - no atomics, the same bits on every run - and read nothing
 * back, so a captured step may hold them.  keep is int32 [B, K], the kept patch indices of every sample ascending; inv is
 * int32 [B, P], the slot of patch p in keep[b] or -1.  1 <= K <= P <= EAV_MAX_TOKENS - nextra.
 * eav_patch_keep_plan draws the tables, one workgroup per sample: the key of patch p of sample b is
 * eav_hash32(seed + 2 * *counter, b*P + p) (counter NULL: seed itself; the rule of the dropout kernels), the kept set the K
 * smallest of the total order (key, p) - the 24-bit keys do tie, the patch index decides.  keys (optional, uint32 [B, P])
 * replaces the hash, as the explicit masks replace it for the dropout kernels.
 * eav_patch_keep_invert builds inv from a given keep (rows ascending and unique).
 * eav_im2col_keep: col [B*K, C*P*P], row b*K + s the row eav_im2col forms for patch keep[b][s] (arguments as eav_im2col;
 * an index outside the grid gives a row of zeros).
 * eav_embed_finish_keep: h [B, nextra + K, D]; eav_embed_finish with the position row of patch slot s taken from
 * pos[nextra + keep[b][s]], pos the full [nextra + P, D] table.
 * eav_embed_bwd_keep: demb[b*K + s] = dh[b, nextra + s]; dpos [nextra + P, D]: rows r < nextra the sum over b of dh[b, r],
 * row nextra + p the sum in ascending b of dh[b, nextra + inv[b][p]] over the samples that kept p, +0.0 where none did. */
#define EAV_MAX_TOKENS 2048
int eav_patch_keep_plan(int* keep, int* inv, int B, int P, int K, uint64_t seed, const uint64_t* counter,
                        const uint32_t* keys, void* stream);
int eav_patch_keep_invert(const int* keep, int* inv, int B, int P, int K, void* stream);
int eav_im2col_keep(const float* x, float* col, const int* keep, int B, int C, int H, int W, int P, int sy, int sx,
                    int transposed, int K, void* stream);
int eav_embed_finish_keep(float* h, const float* cls, const float* dist, const float* pos, const int* keep, int B, int K,
                          int D, int nextra, void* stream);
int eav_embed_bwd_keep(const float* dh, float* dpos, float* demb, const int* inv, int B, int P, int K, int D, int nextra,
                       void* stream);
/* Stochastic depth (timm.layers.DropPath, scale_by_keep; csrc/drop_path.hip): in training mode sample b drops the whole
 * residual branch of layer i with probability p_i = rate * i / (L - 1) (formed in double, rounded once to float; 0 for
 * L = 1), kept branches are scaled by 1 / (1 - p_i).  Both kernels are in gather form - no atomics, the same bits on every
 * run - and read nothing back, so a captured step may hold them.
 * eav_drop_path_plan fills scale, float [L, 2, B]: row 2 i the attention branch of layer i, row 2 i + 1 its MLP branch.  Rows
 * with p_i == 0 hold 1.0.  Elsewhere scale[r][b] is 1 / (1 - p_i) where sample b is kept and 0 where it is dropped: kept means
 * eav_hash32(seed + (r << 40) + 2 * *counter, b) * 2^-24 >= p_i (counter NULL: no counter term; seed is the site seed of row
 * 0, consecutive rows have consecutive site ids), or keep[r][b] != 0 where keep (optional, uint8 [L, 2, B]) is given.
 * eav_drop_path_add: out[b, :] = resid[b, :] + y[b, :] * scale_row[b] over B samples of per_sample floats (per_sample % 4 == 0,
 * 16-byte aligned pointers; resid NULL: out = y * s, the gate of the backward; out may be y, not resid).  The product is
 * rounded, then added - float32 resid + y * s bit for bit, signed zeros included; NaN / Inf in a dropped y give NaN. */
int eav_drop_path_plan(float* scale, int L, int B, double rate, uint64_t seed, const uint64_t* counter, const uint8_t* keep,
                       void* stream);
int eav_drop_path_add(const float* y, const float* resid, float* out, const float* scale_row, int B, int64_t per_sample,
                      void* stream);
/* ViT position table at another patch grid (HF ViTEmbeddings.interpolate_pos_encoding: F.interpolate(mode="bicubic",
 * align_corners=False), no antialiasing): pos [nextra + g*g, D] -> out [nextra + ny*nx, D], the first nextra rows copied,
 * the patch rows out = (Wy (x) Wx) pos.  iy / ix [n_out][4] are the source indices of the four taps of every output index
 * along its axis (each within [0, g)), wy / wx [n_out][4] their weights; a tap of weight 0 is skipped, so an identity
 * resampling copies bit for bit.  The tables are device arrays (eav_amd/pos_interp.py builds them in float64).
 * eav_pos_bicubic_bwd is the exact adjoint in gather form: dpos [nextra + g*g, D] from dout [nextra + ny*nx, D], one
 * workgroup per source row walking the transposed per-axis lists - ypt / xpt [g + 1] CSR row pointers, yidx / xidx the
 * output indices, yw / xw the weights, nnzy / nnzx their lengths (<= 4 n_out) - in stored order: no atomics, the same bits
 * on every run, every element of dpos written.  D % 4 == 0; pos / out / dout / dpos 16-byte aligned; g, ny, nx <= 2048. */
int eav_pos_bicubic_fwd(const float* pos, float* out, int g, int ny, int nx, int D, int nextra, const int* iy,
                        const float* wy, const int* ix, const float* wx, void* stream);
int eav_pos_bicubic_bwd(const float* dout, float* dpos, int g, int ny, int nx, int D, int nextra, const int* ypt,
                        const int* yidx, const float* yw, int nnzy, const int* xpt, const int* xidx, const float* xw,
                        int nnzx, void* stream);
/* AST position table at another number of time patches: pos [nextra + ny*nx0, D] -> out [nextra + ny*nx, D], rows
 * frequency-major (nextra + f*nx + t), the first nextra rows copied, out[f, t] = sum_a w[t][a] pos[f, idx[t][a]] with
 * idx / w [nx][2] device arrays (eav_amd/pos_time.py: one tap of weight 1 for a centre cut, nx < nx0; the two taps of a
 * linear interpolation, align_corners=False, for nx > nx0); the frequency axis is untouched.  A tap of weight 0 is skipped
 * and the first term is a plain product, so a cut copies bit for bit.  eav_pos_time_bwd is the exact adjoint in gather
 * form: dpos [nextra + ny*nx0, D] from dout [nextra + ny*nx, D], one workgroup per source row walking the transposed list -
 * ptr [nx0 + 1] CSR row pointers, oidx the output time indices, w the weights, nnz their length (<= 2 nx) - in stored
 * order: no atomics, the same bits on every run, every element of dpos written (zeros where no output reads the row).
 * D % 4 == 0; pos / out / dout / dpos 16-byte aligned and distinct; ny, nx0, nx in 1 .. 2048; nextra <= 2. */
int eav_pos_time_fwd(const float* pos, float* out, int ny, int nx0, int nx, int D, int nextra, const int* idx,
                     const float* w, void* stream);
int eav_pos_time_bwd(const float* dout, float* dpos, int ny, int nx0, int nx, int D, int nextra, const int* ptr,
                     const int* oidx, const float* w, int nnz, void* stream);
/* gather (scatter=0) / scatter (1) the first nextra token rows of every image: rows[b*nextra+e] <-> h[b,e]. */
int eav_token_rows(float* h, float* rows, int B, int ntok, int D, int nextra, int scatter, void* stream);
/* AST pooled = (cls + dist)/2 (HF AST :304); backward=1 writes dseq from dpooled. */
int eav_pair_mean(float* seq, float* pooled, int B, int D, int backward, void* stream);

/* ---- ShallowConvNet + single-head transformer (Transformer_torch/Transformer_EEG.py:14-148) ------------------- */
/* conv(1->NF,(1,KC),valid) fused with PatchEmbedding's per-filter Linear(Chans->1) (:117,:28-35):
 * x [B,C,S] -> u [B,NF,S] (channel-projected input, kept for the backward) and v [B,S-KC+1,NF] tokens.
 * Chans <= 32, NF <= 48, KC <= 16, S >= KC; the columns of wv beyond Chans are not read.
 * eav_shallow_embed_nparts(B, S) = B*ceil(S/64). */
int eav_shallow_embed_nparts(int B, int S);
int eav_shallow_embed_fwd(const float* x, const float* wc, const float* wv /*[NF] rows, stride ldv*/, int ldv, float* u,
                          float* v, int B, int C, int S, int NF, int KC, void* stream);
/* weight gradients: part_c [nparts][NF*KC] (conv taps), part_v [nparts][NF*C] (channel projections). */
int eav_shallow_embed_bwd(const float* dv, const float* x, const float* u, const float* wc, float* part_c,
                          float* part_v, int B, int C, int S, int NF, int KC, void* stream);
/* nn.ReLU -> nn.Dropout in place (:84-85) and its backward (act = the forward's output).  A NaN propagates, as in
 * nn.ReLU: the forward leaves it a NaN whatever its keep decision; the backward passes the gradient (times the dropout
 * scale) where act is NaN, as torch's ReLU backward does - act does not record whether a NaN was kept. */
int eav_relu_dropout(float* h, int64_t n, float drop_p, uint64_t seed, const uint8_t* mask, const uint64_t* seed_dev,
                     void* stream);
int eav_relu_dropout_bwd(float* dact, const float* act, int64_t n, float drop_p, void* stream);
/* out = resid + Dropout(y) (:103-104); resid NULL: out = Dropout(y) (also the backward of the dropout branch). */
int eav_dropout_add(const float* y, const float* resid, float* out, int64_t n, float drop_p, uint64_t seed,
                    const uint8_t* mask, const uint64_t* seed_dev, void* stream);
/* out[m,0:n) = a[m,0:n) (+ b[m,0:n)) with leading dimensions - the "+ V" residual of MultiHeadAttention (:74-76). */
int eav_add_strided(const float* a, int lda, const float* b, int ldb, float* out, int ldo, int64_t M, int n,
                    void* stream);
/* per-column sum / sum of squares of x [M,N<=256]: part [eav_colstats_nparts(M) = ceil(M/256)][2N], row p = rows
 * [256 p, 256 p + 256) (BatchNorm over tokens, :136). */
int eav_colstats_nparts(int64_t M);
int eav_colstats(const float* x, float* part, int64_t M, int N, int ld, void* stream);
/* head (:136-144): BatchNorm affine -> square -> AvgPool(1,win)/stride -> log(clamp(lo,hi)) -> Dropout.
 * v [B,T,NF] tokens -> pooled [B,NF,NP] (pre-log means, kept for the backward) and out [B,NF*NP].  A NaN mean propagates
 * (torch.clamp), it is not clamped to lo.  NF <= 256, (NP-1)*stride + win <= T, NF*NP + 512 floats within 64 KB. */
int eav_sqpool_log_fwd(const float* v, const float* bn, float* pooled, float* out, int B, int T, int NF, int NP,
                       int win, int stride, float lo, float hi, float drop_p, uint64_t seed, const uint8_t* mask,
                       const uint64_t* seed_dev, void* stream);
/* g [B,T,NF] = dL/d(BatchNorm output) (zero for tokens no window covers); part [B][2*NF] = sums for
 * eav_bn_bwd_finalize.  The gradient passes where lo <= pooled <= hi, bounds included (torch.clamp's backward), and is zero
 * at a NaN mean. */
int eav_sqpool_log_bwd(const float* dy, const float* pooled, const float* v, const float* bn, float* g, float* part,
                       int B, int T, int NF, int NP, int win, int stride, float lo, float hi, float drop_p,
                       uint64_t seed, const uint8_t* mask, const uint64_t* seed_dev, void* stream);
/* BatchNorm input gradient on token-major rows; bn = mean, invstd, scale, shift, m1, m2 (NF each). */
int eav_bn_rows_bwd(const float* g, const float* v, const float* bn, float* dx, int64_t M, int NF, void* stream);

/* ---- pre-processing (SURVEY section 8f "next" rows) ------------------------------------------------ */
/* HF image processor on a batch of uint8 HWC frames (Transformer_Vision.py:52-59): Pillow-exact 8-bit
 * bilinear resize (coefficient tables kx/ky [out][ksize] int32 and bounds [out][2] = (first, count), built
 * on the host like Pillow's precompute_coeffs), * rescale (float64), (x - mean) / std -> out [n,C,OH,OW] fp32.
 * mean3 / std3 are HOST pointers. */
int eav_resize_normalize_u8(const uint8_t* frames, const int* kx, const int* boundsx, const int* ky,
                            const int* boundsy, float* out, int n, int H, int W, int C, int OH, int OW, int ksize_x,
                            int ksize_y, double rescale, const float* mean3, const float* std3, void* stream);

/* AST log-mel front-end, HF ASTFeatureExtractor numpy path (Transformer_Audio.py:38-42): wav [n,L] fp32 (16 kHz)
 * -> out [n,max_len,nmel] fp32 = (log-mel - mean) / std2 with frames beyond the clip zero-padded before the
 * normalisation.  window400 (Hann, symmetric), twiddle256 ([k] = cos, -sin of 2 pi k/512) and melT [nmel][257]
 * are float64 DEVICE tables built by the host (eav_amd/preprocess.py). */
int eav_ast_fbank(const float* wav, const double* window400, const double* twiddle256, const double* melT, float* out,
                  int n, int L, int max_len, int nmel, double preemph, double mel_floor, float mean, float std2,
                  void* stream);

/* EEG pre-processing, float64 like scipy (Dataload_eeg.py:85-121).
 * scipy.signal.resample_poly(x, 1, down): y[c][m] = sum_j h[j] x[c][m*down + center - j], x [nch][n_in]. */
int eav_decimate_fir_f64(const double* x, const double* h, double* y, int nch, int64_t n_in, int64_t n_out, int down,
                         int ntaps, int center, void* stream);
/* scipy.signal.resample_poly(x, up, down, axis=1) for any reduced up / down, centred form:
 * y[c][m] = sum_i h[m*down + center - i*up] x[c][i] over 0 <= i < n_in with the tap index in [0, ntaps);
 * n_out = ceil(n_in * up / down).  h [ntaps] float64 is the DEVICE table of eav_amd.eeg_data.resample_poly_design
 * (already times up; center = half_len, ntaps = 2 half_len + 1).  LDS: one budget of 64 KiB = 8192 doubles per workgroup
 * for taps and input tile TOGETHER - the taps are staged when ntaps <= 8192, the tile ((255 down + ntaps - 1) / up + 2
 * samples) when it fits what the taps leave; whichever does not fit is read from global memory by the same loop (no ratio
 * is refused).  One fma chain per output in ascending i (no atomics). */
int eav_resample_poly_f64(const double* x, const double* h, double* y, int nch, int64_t n_in, int64_t n_out, int up,
                          int down, int ntaps, int center, void* stream);
/* scipy.signal.sosfilt(sos, x) along the last axis of x [nch][n] (zero initial state), exact chunk-parallel form:
 * sos [nsec][6]; H [Lc][2 nsec] = cascade output at step k from unit initial state j; AL [2 nsec][2 nsec] = state
 * after Lc zero-input steps; zend / zstart: scratch [nch][ceil(n/Lc)][2 nsec]. */
int eav_sosfilt_f64(const double* x, double* y, const double* sos, const double* H, const double* AL, double* zend,
                    double* zstart, int nch, int64_t n, int nsec, int Lc, void* stream);

/* Audio resampling, torchaudio.transforms.Resample (sinc_interp_hann; Dataload_audio.py:40-45): x [rows][n_in] fp32 ->
 * y [rows][n_out], n_out = ceil(nw * n_in / orig), y[f*nw + p] = sum_j taps[p][j] xp[f*orig + j] with xp = x padded by
 * `width` zeros in front and width + orig behind (the padding is implicit).  taps [nw][ntaps = 2 width + orig] fp32 is
 * the DEVICE table of eav_amd.preprocess.sinc_resample_design; taps the design clamps to the window's edge (~1e-33)
 * are skipped.  Rows of different lengths: zero-pad to the longest and drop each row's outputs beyond its own
 * ceil(nw * L / orig).  Fixed accumulation order (no atomics). */
int eav_resample_sinc_f32(const float* x, const float* taps, float* y, int rows, int64_t n_in, int64_t n_out, int orig,
                          int nw, int width, int ntaps, void* stream);

/* ---- audio CNN (CNN_torch/CNN_audio.py AudioModel; csrc/audio_cnn.hip) -------------------------------------------
 * Every conv of the model is Conv1d(kernel 5, padding 2) with a bias; tensors are [B][channels][length] fp32.
 * Forward: out = ReLU(conv(in) + bias), then (drop_p > 0) dropout - mask (uint8 [B][N][Lin], may be NULL) or the
 * counter-based generator (seed + 2 * *seed_dev when seed_dev is set) - and with pool = 1 MaxPool1d(8): out is
 * [B][N][Lout/8] and idx receives the argmax within each window (first index on ties, NaN propagates).  pool = 0 needs
 * Lout == Lin; pool = 1 needs Lin / 8 == Lout / 8 (the classifier's fixed width: T in Lout...Lout+7) and C % 16 == 0;
 * C is 1 or a multiple of 16. */
int eav_audio_conv5_fwd(const float* in, const float* w, const float* bias, float* out, uint8_t* idx, int B, int C,
                        int N, int Lin, int Lout, int pool, float drop_p, uint64_t seed, const uint8_t* mask,
                        const uint64_t* seed_dev, void* stream);
/* Data gradient of a conv whose weight is w [C][N][5] (C = the layer's output channels, N = its input channels):
 * din[b][n][t] = sum_{c,tap} w[c][n][tap] g[b][c][t - tap + 2] for t < Lout, g = dout [B][C][Lin] times
 * (gate_in > 0 ? gscale_in : 0) when gate_in is set.  mode 0: din [B][N][Lout], zero where aux [B][N][Lout] <= 0 (ReLU
 * backward; aux may be NULL).  mode 1 (MaxPool1d(8) + dropout + ReLU backward): din is the dense [B][N][8 Lout] gradient
 * of the pre-pool activation: at 8 t + idx[b][n][t] it holds the product times gscale_out where the pooled value aux
 * [B][N][Lout] is > 0, zero elsewhere.  C % 16 == 0. */
int eav_audio_conv5_dgrad(const float* dout, const float* gate_in, float gscale_in, const float* w, float* din,
                          const float* aux, const uint8_t* idx, float gscale_out, int B, int C, int N, int Lin, int Lout,
                          int mode, void* stream);
/* Weight + bias gradient partials: part[p][m * Cact * 5 + c * 5 + tap] = sum dout[b][m][t] act[b][c][t + tap - 2],
 * part[p][M * Cact * 5 + m] = sum dout[b][m][t], over the (sample, 32-position) chunks p, p + nparts, ... (dout [B][M][Lout]
 * times (gate > 0 ? gscale : 0) when gate is set; act [B][Cact][Lact], zero outside).  eav_reduce_partials sums them in
 * fixed order into the adjacent weight and bias gradients.  nparts must be eav_audio_wgrad_nparts(B, Cact, M, Lout). */
int eav_audio_wgrad_nparts(int B, int Cact, int M, int Lout);
int eav_audio_conv5_wgrad(const float* dout, const float* gate, float gscale, const float* act, float* part, int B,
                          int Cact, int M, int Lact, int Lout, int nparts, void* stream);

/* ---- video CNN (CNN_torch/CNN_Vision.py VideoModel: torchvision ResNet-50 trunk + channel-attention head;
 *      csrc/video_cnn.hip) ------------------------------------------------------------------------------------------
 * Activations are NHWC fp32 (rows [B*H*W][C]); weights keep torchvision's layout w [Cout][Cin][kh][kw] and are re-laid for
 * the implicit GEMMs by eav_video_conv_relayout: wf [Cout][kh][kw][Cin] (forward), wd [Cin][kh][kw][Cout] (data gradient).
 * A conv geometry is (B, C = input channels, H, W, N = output channels, KH, KW, S = stride, P = pad, OH, OW), with
 * OH = (H + 2P - KH) / S + 1 (floor) and OW likewise; channels <= 4096, kernel <= 15, stride <= 4, P < kernel.
 * nchw = 1 reads the input image as [B][C][H][W] (the pre-processed frames of the stem conv).  Operands need 16-byte
 * alignment only where they are read as float4: an NHWC image with C % 8 == 0, an output gradient with N % 8 == 0, a
 * re-laid weight whose rows are a multiple of 8 floats. */
int eav_video_conv_relayout(const float* w, float* wf, float* wd, int Co, int Ci, int KK, void* stream);
/* out [B*OH*OW][N] = sum_{kh,kw,c} in[b][oh*S-P+kh][ow*S-P+kw][c] w[n][c][kh][kw] (zero outside the image). */
int eav_video_conv_fwd(const float* x, const float* wf, float* out, int B, int C, int H, int W, int N, int KH, int KW,
                       int S, int P, int OH, int OW, int nchw, void* stream);
/* din [B*H*W][C] = (add, may be NULL) + sum over (kh, kw, n) with (ih + P - kh) and (iw + P - kw) non-negative multiples
 * of S inside the output map of dout[b][oh][ow][n] w[n][c][kh][kw]. */
int eav_video_conv_dgrad(const float* dout, const float* wd, const float* add, float* din, int B, int C, int H, int W,
                         int N, int KH, int KW, int S, int P, int OH, int OW, void* stream);
/* Weight-gradient partials part[p][n][c][kh][kw] = sum over the 32-pixel chunks q = p, p + nparts, ... of the B*OH*OW
 * output pixels of dout[pixel][n] in[window][c]; eav_reduce_partials sums them in fixed order.  nparts must be
 * eav_video_wgrad_nparts(N, C, KH*KW, B*OH*OW). */
int eav_video_wgrad_nparts(int N, int C, int KK, int64_t M);
int eav_video_conv_wgrad(const float* dout, const float* x, float* part, int B, int C, int H, int W, int N, int KH, int KW,
                         int S, int P, int OH, int OW, int nchw, int nparts, void* stream);
/* BatchNorm over rows [M][C] (C <= 4096): part [eav_video_bn_nparts(M)][2C] = per-channel sum x, sum x^2 of 256-row
 * chunks (input of eav_bn_finalize), two rows per chunk: the fp32 rounding of the chunk's fp64 sum and its remainder. */
int eav_video_bn_nparts(int64_t M);
int eav_video_bn_stats(const float* x, float* part, int64_t M, int C, void* stream);
/* out = ReLU?(x * scale[c] + shift[c] + r), r = res * rscale[c] + rshift[c] (rscale / rshift set), res (only res set) or
 * 0 (res NULL).  out may alias x or res. */
int eav_video_bn_apply(const float* x, const float* scale, const float* shift, const float* res, const float* rscale,
                       const float* rshift, float* out, int64_t M, int C, int relu, void* stream);
/* Backward sums: g = dy, zero where y <= 0 when y (the stored ReLU output) is set; g is written to `g` when set (needed
 * with y); part [eav_video_bn_nparts(M)][2C] = sum g, sum g * (x - mean) * invstd for eav_bn_bwd_finalize; bn = mean,
 * invstd, ... as eav_bn_finalize writes them.  The input gradient is eav_bn_rows_bwd on the same rows. */
int eav_video_bn_bwd(const float* dy, const float* y, const float* x, const float* bn, float* g, float* part, int64_t M,
                     int C, void* stream);
/* nn.MaxPool2d(K, S, P) on NHWC: idx = kh * K + kw of the window maximum (scan order, first index on ties, a NaN
 * propagates - torch's CPU max_pool2d); the backward gathers dx from the windows whose argmax is the position. */
int eav_video_maxpool_fwd(const float* x, float* out, uint8_t* idx, int B, int H, int W, int C, int OH, int OW, int K,
                          int S, int P, void* stream);
int eav_video_maxpool_bwd(const float* dout, const uint8_t* idx, float* dx, int B, int H, int W, int C, int OH, int OW,
                          int K, int S, int P, void* stream);
/* Channel-attention head on the trunk output y [B][HW][C] (HW <= 256):
 * head_pool: pooled [2B][C] = AdaptiveAvgPool (rows 0..B-1) and AdaptiveMaxPool (rows B..2B-1, argmax idx [B][C]);
 * head_scale_pool: attn = A[b] + A[B+b] (the fc2 outputs of both rows), z [B][C] = mean_hw(y * attn);
 * head_attn_bwd: dA [2B][C] = d attn = sum_hw (dz / HW) y, in both halves;
 * head_feat_bwd: dy = (dz / HW) attn + dP[b] / HW + (hw == argmax ? dP[B+b] : 0), dP = d pooled. */
int eav_video_head_pool(const float* y, float* pooled, uint8_t* idx, int B, int HW, int C, void* stream);
int eav_video_head_scale_pool(const float* y, const float* A, float* attn, float* z, int B, int HW, int C, void* stream);
int eav_video_head_attn_bwd(const float* y, const float* dz, float* dA, int B, int HW, int C, void* stream);
int eav_video_head_feat_bwd(const float* dz, const float* attn, const float* dP, const uint8_t* idx, float* dy, int B,
                            int HW, int C, void* stream);
/* c[i] += 1 for i < n (the BatchNorm num_batches_tracked counters, one device array) */
int eav_video_counters_inc(int64_t* c, int n, void* stream);

/* ---- measured peaks (bench.py): register-only fp32 MFMA loop (FLOP = blocks*4 waves*iters*4*4096) and a float4
 *      streaming copy, to quote roofline fractions against what this chip sustains. */
int eav_peak_mfma_f32(float* sink, int blocks, int iters, void* stream);
int eav_peak_mfma_f16(float* sink, int blocks, int iters, void* stream);
/* L2 -> CU read ceiling probe (bench.py measured_peaks / tuning): mode 0 = 16-byte loads into registers, 1 = LDS-DMA;
 * every wave reads 1-KB chunks of the first footprint_kb KB of src, 8 in flight; bytes = blocks * 4 * iters * 8192. */
int eav_peak_l2_read(const void* src, int footprint_kb, int mode, int iters, int blocks, float* sink, void* stream);
int eav_peak_copy_variant(const float* src, float* dst, int64_t n, int variant, int blocks, void* stream);
int eav_peak_copy(const float* src, float* dst, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EAV_HIP_H */
