// EEGNet temporal FIR (firstConv, up to 321 taps, 1 -> 8 filters) and its weight gradient by FFT, exact fp32 arithmetic.
//
// Reference op: nn.Conv2d(1, F1=8, (1, kernLength=300), padding='same', bias=False) (CNN_torch/EEGNet_tor.py:24,51) and
// the weight gradient autograd derives for it (:109).  The direct form costs 2 x 300 flops per output and filter - 92 GFLOP
// per pass at [64,1,30,10000], 0.59 ms at the fp32 matrix peak (eegnet_fir.hip reaches 0.73 / 0.83 ms).  A convolution
// with a 300-tap filter is the same linear map evaluated by overlap-save blocks of 1024-point FFTs in ~350 flops per
// output sample for all 8 filters together: 13 x fewer flops, so the two kernels here are bound by the HBM traffic of
// y1 / g1 (614 MB each) instead of by arithmetic.
//
// Forward (per block of LB = 704 outputs of a pair of electrodes c, c+1):
//   s[n] = x[c][t0 - padl + n] + i x[c+1][t0 - padl + n], n = 0 .. 1023 (zero outside the recording)
//   y_f[j] = sum_k w_f[k] s[j + k]  (j < 704, k < klen: j + k <= 1023, no wrap)  = IFFT(FFT(s) . conj(FFT(w_f)))[j]
//   Re y_f = the output of electrode c, Im y_f = that of electrode c+1 (a real filter maps real to real, imaginary to
//   imaginary): one complex transform serves two electrodes with no unpacking.
// Weight gradient (dy formed from g1, y1 and the BatchNorm-backward coefficients while loading, as in eegnet_fir.hip):
//   dW_f[k] = sum_{b,c,t} dy[b,f,c,t] x[b,c,t + k - padl] = Re IFFT( sum_{b, pairs, blocks} conj(FFT(D_f)) . FFT(s) )[k]
//   with D_f = dy_c + i dy_{c+1} of a block (704 samples, zero-padded): Re(conj(D) s') = d_c s'_c + d_{c+1} s'_{c+1}.
//   The spectra are accumulated per workgroup in registers (wave f owns filter f), written once, summed over the
//   workgroups in a fixed order and transformed back by a finishing kernel - bit-reproducible run to run.
// The last block of a row is usually short (144 of 704 outputs at 10000 samples); where two such tails fit into the two
// halves of one segment they share its transforms (`Units` below).
//
// The 1024-point complex FFT runs inside ONE wave, 16 points per lane (element j of lane l = index l + 64 j on input and
// output), as radix 16 x 16 x 4 with one exchange through a wave-private LDS buffer and one between lanes:
//   n = 64 n1 + 4 n2 + n3,  k = k1 + 16 k2 + 256 k3
//   (1) radix-16 DFT over n1 in registers (lane = 4 n2 + n3), twiddle W^(lane k1)
//   (2) exchange through LDS: slot 66 k1 + lane  ->  lane' = k1 + 16 n3 reads slots 66 k1 + n3 + 4 n2 (n2 < 16)
//   (3) radix-16 DFT over n2, twiddle W64^(n3 k2): lane' holds k2 = 4 m + r in register 4 m + r
//   (4) exchange in registers: per m < 4 a 4 x 4 transpose between the lane bits 4-5 (n3) and the register bits 0-1 (r)
//       by v_permlane32_swap / v_permlane16_swap  ->  lane'' = k1 + 16 r holds n3 in register 4 m + n3
//   (5) radix-4 DFT over n3: X[lane'' + 64 (m + 4 k3)] in register m + 4 k3
// Every ds_write_b64 / ds_read_b64 of the LDS exchange is bank-conflict free (pitch 66 slots; checked in
// tests/test_fir_fft_layout_cpu.py against the lane groups of MI355X_MICROARCH.md section LDS).  No workgroup barrier
// inside the transform.
#include <algorithm>
#include <type_traits>

#include "eav_common.h"
#include "../../include/eav_hip.h"
#include "../../include/eav_hip_tuning.h"

namespace {

constexpr int F1 = 8;
constexpr int NF = 1024;        // transform length
constexpr int LB = 704;         // outputs per block: 11 rows of 64 (2816 B = 22 cache lines, so every block is line aligned)
constexpr int NROW = LB / 64;   // 11
constexpr int XP = 66;          // pitch of the exchange rows: reads 66 k1 + n3 (+ 4 n2) cover 32 distinct 8-byte banks
constexpr int WBUF = 1056;      // float2 slots of a wave's exchange buffer: 66 x 15 + 64, rounded to 128 bytes
constexpr int MAXK = NF - LB + 1;   // 321 taps

typedef float v2f __attribute__((ext_vector_type(2)));

// y1 / g1 are streamed exactly once by these kernels (614 MB each): non-temporal accesses keep them from evicting the
// input segments that ARE re-used out of the L2 (plain accesses measured 2-4 % slower).
// Timing-only ablations (measured once, since removed): the arithmetic side alone (no loads or stores) / the memory side
// alone (no transforms) - forward 0.26 / 0.15 ms of 0.28, weight gradient 0.31 / 0.25 ms of 0.39: the transforms, not HBM,
// are the longer leg.
#define EAV_LDG(p) __builtin_nontemporal_load(p)
#define EAV_STG(p, v) __builtin_nontemporal_store((v), (p))

__device__ __forceinline__ v2f swp(v2f a) { return __builtin_shufflevector(a, a, 1, 0); }      // (y, x): an op_sel, no move
__device__ __forceinline__ v2f fma2(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }
// Two complex products a0 b0, a1 b1 (CONJ: a conj(b)) in FOUR packed instructions: what hipcc cannot select is one
// v_pk_fma_f32 with a swapped AND half-negated operand (it builds the pair with a third instruction).  The two products are
// interleaved so that no packed result is consumed by the next instruction (gfx950 needs one wait state there); the
// leading s_nop covers a packed producer of an input directly in front of the block, the trailing `s_nop 1` a consumer
// hipcc schedules directly behind it (the hazard recogniser does not see into inline asm: a v_permlane*_swap of the last
// result needs two wait states after the VALU write, a packed consumer one).
template <bool CONJ>
__device__ __forceinline__ void cmul2(v2f a0, v2f b0, v2f a1, v2f b1, v2f& r0, v2f& r1) {
  if (CONJ)
    asm("s_nop 0\n\t"
        "v_pk_mul_f32 %0, %2, %3 op_sel_hi:[0,1] neg_hi:[0,1]\n\t"
        "v_pk_mul_f32 %1, %4, %5 op_sel_hi:[0,1] neg_hi:[0,1]\n\t"
        "v_pk_fma_f32 %0, %2, %3, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1]\n\t"
        "v_pk_fma_f32 %1, %4, %5, %1 op_sel:[1,1,0] op_sel_hi:[1,0,1]\n\t"
        "s_nop 1"
        : "=&v"(r0), "=&v"(r1) : "v"(a0), "v"(b0), "v"(a1), "v"(b1));
  else
    asm("s_nop 0\n\t"
        "v_pk_mul_f32 %0, %2, %3 op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %1, %4, %5 op_sel_hi:[0,1]\n\t"
        "v_pk_fma_f32 %0, %2, %3, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0]\n\t"
        "v_pk_fma_f32 %1, %4, %5, %1 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0]\n\t"
        "s_nop 1"
        : "=&v"(r0), "=&v"(r1) : "v"(a0), "v"(b0), "v"(a1), "v"(b1));
}
// acc0 += a0 conj(b0), acc1 += a1 conj(b1): four packed fmas, the accumulators interleaved for the same reason
__device__ __forceinline__ void cmacc2_conj(v2f a0, v2f b0, v2f a1, v2f b1, v2f& acc0, v2f& acc1) {
  asm("s_nop 0\n\t"
      "v_pk_fma_f32 %0, %2, %3, %0 op_sel_hi:[0,1,1] neg_hi:[0,1,0]\n\t"
      "v_pk_fma_f32 %1, %4, %5, %1 op_sel_hi:[0,1,1] neg_hi:[0,1,0]\n\t"
      "v_pk_fma_f32 %0, %2, %3, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1]\n\t"
      "v_pk_fma_f32 %1, %4, %5, %1 op_sel:[1,1,0] op_sel_hi:[1,0,1]\n\t"
      "s_nop 1"
      : "+v"(acc0), "+v"(acc1) : "v"(a0), "v"(b0), "v"(a1), "v"(b1));
}

// a w (forward) / a conj(w) (inverse) for a twiddle w, in a form hipcc maps to v_pk_mul_f32 / v_pk_fma_f32 with op_sel
// operands only (written as a.xx * w + a.yy * (-w.y, w.x) it builds the swapped / negated pair with a v_xor + v_mov per
// product): the w-only factors are loop invariants the compiler keeps in registers, which leaves two instructions per product
template <bool INV>
__device__ __forceinline__ v2f twmul(v2f a, v2f w) {
  return fma2(w.yy * (INV ? (v2f){1.f, -1.f} : (v2f){-1.f, 1.f}), swp(a), w.xx * a);
}
// multiply by -i (forward) / +i (inverse)
template <bool INV>
__device__ __forceinline__ v2f rot(v2f a) {
  return swp(a) * (INV ? (v2f){-1.f, 1.f} : (v2f){1.f, -1.f});
}

template <bool INV>
__device__ __forceinline__ void dft4(v2f& a0, v2f& a1, v2f& a2, v2f& a3) {
  // t1 +- rot(d) = fma(swap(d), (1, -1), t1): the rotation rides on the add (exact: the factors are +-1)
  const v2f t0 = a0 + a2, t1 = a0 - a2, t2 = a1 + a3, d = swp(a1 - a3);
  const v2f c = INV ? (v2f){-1.f, 1.f} : (v2f){1.f, -1.f};
  a0 = t0 + t2;
  a1 = fma2(d, c, t1);
  a2 = t0 - t2;
  a3 = fma2(d, -c, t1);
}

// 16-point DFT in registers: n = 4 a + b, k = c + 4 d; X[c + 4 d] = sum_b W16^(b c) W4^(b d) sum_a v[4 a + b] W4^(a c)
template <bool INV>
__device__ __forceinline__ void dft16(v2f (&v)[16]) {
  constexpr float C1 = 0.92387953251128674f, S1 = 0.38268343236508977f, R2 = 0.70710678118654752f;
#pragma unroll
  for (int b = 0; b < 4; ++b) dft4<INV>(v[b], v[4 + b], v[8 + b], v[12 + b]);      // v[4 c + b] = y[b][c]
  // y[b][c] *= W16^(b c), W16^m = (cos, -sin)(2 pi m / 16)
  v[4 * 1 + 1] = twmul<INV>(v[4 * 1 + 1], (v2f){C1, -S1});      // b c = 1
  v[4 * 2 + 1] = twmul<INV>(v[4 * 2 + 1], (v2f){R2, -R2});      // 2
  v[4 * 3 + 1] = twmul<INV>(v[4 * 3 + 1], (v2f){S1, -C1});      // 3
  v[4 * 1 + 2] = twmul<INV>(v[4 * 1 + 2], (v2f){R2, -R2});      // 2
  v[4 * 2 + 2] = rot<INV>(v[4 * 2 + 2]);                        // 4: -i
  v[4 * 3 + 2] = twmul<INV>(v[4 * 3 + 2], (v2f){-R2, -R2});     // 6
  v[4 * 1 + 3] = twmul<INV>(v[4 * 1 + 3], (v2f){S1, -C1});      // 3
  v[4 * 2 + 3] = twmul<INV>(v[4 * 2 + 3], (v2f){-R2, -R2});     // 6
  v[4 * 3 + 3] = twmul<INV>(v[4 * 3 + 3], (v2f){-C1, S1});      // 9
  // for each c: DFT over b of y[b][c] = v[4 c + b] -> X[c + 4 d]
  v2f o[16];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    v2f y0 = v[4 * c], y1 = v[4 * c + 1], y2 = v[4 * c + 2], y3 = v[4 * c + 3];
    dft4<INV>(y0, y1, y2, y3);
    o[c] = y0; o[c + 4] = y1; o[c + 8] = y2; o[c + 12] = y3;
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) v[k] = o[k];
}

// Twiddle tables of a workgroup in LDS (8.5 KB): t1[k][lane] = W1024^(lane k), t2[k][n3] = W64^(n3 k) - one
// conflict-free ds_read_b64 per use instead of 64 resident VGPRs (with them the forward kernel spilled 68 registers).
constexpr int TWSZ = 16 * 64 + 16 * 4;

__device__ __forceinline__ void make_twiddles(v2f* __restrict__ twl) {      // 512 threads: one entry each, twice
  for (int i = threadIdx.x; i < TWSZ; i += blockDim.x) {
    float s, c;
    // 2 pi m / 1024 = pi (m / 512), 2 pi m / 64 = pi (m / 32): m exact
    if (i < 1024) sincospif((float)((i & 63) * (i >> 6)) * (1.0f / 512.0f), &s, &c);      // t1[k][lane] = W1024^(lane k)
    else sincospif((float)(((i - 1024) & 3) * ((i - 1024) >> 2)) * (1.0f / 32.0f), &s, &c);      // t2[k][n3] = W64^(n3 k)
    twl[i] = (v2f){c, -s};
  }
  __syncthreads();
}

// LDS reads as single ds_read_b64 (2 LDS cycles per wave-instruction): left alone, hipcc pairs them into ds_read2_b64 /
// ds_read2st64_b64, which the LDS serves as two 4 x 16-lane accesses = 8 cycles for the same 16 bytes per lane
// (MI355X_MICROARCH.md, LDS table).  A volatile access is the one form its load-store optimiser leaves alone.
typedef const volatile __attribute__((address_space(3))) v2f* lds_cvp;
__device__ __forceinline__ v2f lds_ld(const v2f* p) { return *(lds_cvp)p; }

// The exchange needs no hardware wait between a wave's writes and its own reads: the LDS executes one wave's DS
// instructions in issue order, and the transform is private to the wave.  What is needed is that the COMPILER keeps the
// order (a "memory" clobber); it then places counted lgkmcnt waits in front of the first use of each read by itself, so the
// butterflies start on the first rows while the last ones are still in flight.
#define FFT_ORDER() asm volatile("" ::: "memory")

// exchange a[lanes 32-63] with b[lanes 0-31] / a[lanes 16-31, 48-63] with b[lanes 0-15, 32-47]: one step of a transpose
// between a lane bit and a register-index bit, both directions in ONE instruction, no LDS
__device__ __forceinline__ void swap32(v2f& a, v2f& b) {
  const auto rx = __builtin_amdgcn_permlane32_swap(__float_as_uint(a.x), __float_as_uint(b.x), false, false);
  const auto ry = __builtin_amdgcn_permlane32_swap(__float_as_uint(a.y), __float_as_uint(b.y), false, false);
  a = (v2f){__uint_as_float(rx[0]), __uint_as_float(ry[0])};
  b = (v2f){__uint_as_float(rx[1]), __uint_as_float(ry[1])};
}
__device__ __forceinline__ void swap16(v2f& a, v2f& b) {
  const auto rx = __builtin_amdgcn_permlane16_swap(__float_as_uint(a.x), __float_as_uint(b.x), false, false);
  const auto ry = __builtin_amdgcn_permlane16_swap(__float_as_uint(a.y), __float_as_uint(b.y), false, false);
  a = (v2f){__uint_as_float(rx[0]), __uint_as_float(ry[0])};
  b = (v2f){__uint_as_float(rx[1]), __uint_as_float(ry[1])};
}

// In-wave 1024-point FFT: v[j] = x[lane + 64 j] -> v[j] = X[lane + 64 j].  INV: conjugate twiddles, no 1/N.
template <bool INV>
__device__ __forceinline__ void fft1024(v2f (&v)[16], v2f* __restrict__ xb, int lane, const v2f* __restrict__ twl) {
  const v2f* t1 = twl + lane;
  const v2f* t2 = twl + 1024 + (lane >> 4);
  dft16<INV>(v);
  v[1] = twmul<INV>(v[1], lds_ld(t1 + 64));
#pragma unroll
  for (int k = 2; k < 16; k += 2) cmul2<INV>(v[k], lds_ld(t1 + 64 * k), v[k + 1], lds_ld(t1 + 64 * k + 64), v[k], v[k + 1]);
#pragma unroll
  for (int k = 0; k < 16; ++k) xb[XP * k + lane] = v[k];
  FFT_ORDER();
  {
    const v2f* rp = xb + XP * (lane & 15) + (lane >> 4);
#pragma unroll
    for (int n2 = 0; n2 < 16; ++n2) v[n2] = lds_ld(rp + 4 * n2);
  }
  FFT_ORDER();
  dft16<INV>(v);
  v[1] = twmul<INV>(v[1], lds_ld(t2 + 4));
#pragma unroll
  for (int k = 2; k < 16; k += 2) cmul2<INV>(v[k], lds_ld(t2 + 4 * k), v[k + 1], lds_ld(t2 + 4 * k + 4), v[k], v[k + 1]);
  // lane 16 n3 + k1 holds k2 = 4 m + r in register 4 m + r; the 4 x 4 transposes put n3 into the register index:
  // lane 16 r + k1, register 4 m + n3
  v2f o[16];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    swap32(v[4 * m], v[4 * m + 2]);
    swap32(v[4 * m + 1], v[4 * m + 3]);
    swap16(v[4 * m], v[4 * m + 1]);
    swap16(v[4 * m + 2], v[4 * m + 3]);
    dft4<INV>(v[4 * m], v[4 * m + 1], v[4 * m + 2], v[4 * m + 3]);
    o[m] = v[4 * m]; o[m + 4] = v[4 * m + 1]; o[m + 8] = v[4 * m + 2]; o[m + 12] = v[4 * m + 3];
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) v[k] = o[k];
}

// segment of one electrode pair: v[j] = x[c0][t0 - padl + lane + 64 j] + i x[c0 + 1][...].  Interior segments of a full
// pair (12 of the 15 blocks of a 10000-sample row) take 32 unpredicated loads; the others one exec-masked load per element.
__device__ __forceinline__ void load_segment(v2f (&v)[16], const float* __restrict__ xrow, bool has1, int S, int tbase,
                                             int lane) {
  if (has1 && tbase >= 0 && tbase + NF <= S) {
    const float* p = xrow + tbase + lane;
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = (v2f){p[64 * j], p[S + 64 * j]};
    return;
  }
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int t = tbase + lane + 64 * j;
    const bool ok = t >= 0 && t < S;
    v[j].x = ok ? xrow[t] : 0.f;
    v[j].y = (ok && has1) ? xrow[S + t] : 0.f;
  }
}

// Unit list of both kernels.  A row of S samples is nblk = ceil(S / 704) blocks, the last one with Lt = S - 704 (nblk - 1)
// outputs.  A tail block needs Lt + klen - 1 input samples; where that is at most 512, TWO tails share one transform: tail
// A in slots 0 .. 511 (register rows 0 .. 7 of every lane), tail B in slots 512 .. 1023 (rows 8 .. 15).  A's outputs
// j < Lt read slots j .. j + klen - 1 <= 511 and B's 512 + j .. <= 1023: no wrap and no cross-talk, and in the weight
// gradient the lags k < klen of IFFT(Z conj(D)) hold A A and B B terms only.  Then the list is
//   main units   u < nmain = B npair nmb: (sample, pair, block) with block < nmb = nblk - 1, all of them whole blocks
//   packed units nmain + p, p < npk = ceil(B npair / 2): the tails 2 p and 2 p + 1 of the flattened (sample npair + pair)
//                index - possibly of two samples; with an odd count the last one stands alone, its upper half empty.
// Otherwise (10000 samples pack: Lt = 144; 500 or 918 samples at 300 taps do not) nmb = nblk, npk = 0 and the tail is an
// ordinary ragged unit.
struct Units {
  int npair, nmb, nmain, ntail, npk, t0t;      // t0t: first output of a packed tail
  __host__ __device__ int total() const { return nmain + npk; }
};
__host__ __device__ inline Units fft_units(int B, int C, int S, int klen) {
  Units q;
  q.npair = (C + 1) / 2;
  const int nblk = (S + LB - 1) / LB, lt = S - (nblk - 1) * LB;
  const bool pack = lt + klen - 1 <= NF / 2;
  q.nmb = pack ? nblk - 1 : nblk;
  q.nmain = B * q.npair * q.nmb;
  q.ntail = pack ? B * q.npair : 0;
  q.npk = (q.ntail + 1) / 2;
  q.t0t = q.nmb * LB;
  return q;
}
// the two tails of packed unit p: (sample, first electrode) of each; the second may be missing
struct Tails {
  int b0, c0, b1, c1;
  bool ex1;
};
__device__ __forceinline__ Tails decode_tails(const Units& q, int p) {
  Tails t;
  const int pr0 = (2 * p) % q.npair;
  t.b0 = (2 * p) / q.npair;
  t.c0 = 2 * pr0;
  t.ex1 = 2 * p + 1 < q.ntail;
  const bool wrap = pr0 + 1 == q.npair;
  t.b1 = wrap ? t.b0 + 1 : t.b0;
  t.c1 = wrap ? 0 : 2 * (pr0 + 1);
  return t;
}
// one half of a packed segment: rows j0 .. j0 + 7 = 512 slots of one tail's electrode pair, zero outside [0, S)
__device__ __forceinline__ void load_half(v2f (&v)[16], int j0, const float* __restrict__ xrow, bool ex, bool has1, int S,
                                          int tbase, int lane) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int t = tbase + lane + 64 * j;
    const bool ok = ex && t >= 0 && t < S;
    v[j0 + j].x = ok ? xrow[t] : 0.f;
    v[j0 + j].y = (ok && has1) ? xrow[S + t] : 0.f;
  }
}

// rows J0 .. J0 + NR - 1 of a ragged block or of one half of a packed unit: the outputs tl + 64 j < S of electrode c0 (and
// of c0 + 1 where the pair has one) are stored, and only they enter the BatchNorm sums
template <bool STATS, int J0, int NR>
__device__ __forceinline__ void store_rows(const v2f (&v)[16], float* __restrict__ dst, int tl, int S, bool has1, float& a1,
                                           float& a2) {
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    if (tl + 64 * j < S) {
      EAV_STG(dst + 64 * j, v[J0 + j].x);
      if (STATS) a1 += v[J0 + j].x, a2 += v[J0 + j].x * v[J0 + j].x;
      if (has1) {
        EAV_STG(dst + S + 64 * j, v[J0 + j].y);
        if (STATS) a1 += v[J0 + j].y, a2 += v[J0 + j].y * v[J0 + j].y;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------ fwd
// Work unit = (sample b, electrode pair, block of 704 outputs), one wave each; the NWF = 12 waves of a workgroup (3 per
// SIMD) share the 8 filter spectra H_f = conj(FFT(w_f)) / 1024, computed by the workgroup itself (wave f < 8 transforms
// filter f).  The filters are real, so H_f[1024 - k] = conj(H_f[k]): only bins 0 .. 512 are kept (33 KB instead of 64 KB -
// what makes room for the exchange buffers of 12 waves), rows j >= 8 of a lane read the mirrored bin and conjugate.
constexpr int NWF = 12;
constexpr int HB = 520;         // float2 slots per filter: bins 0 .. 512, padded to a multiple of 64 bytes

template <bool STATS>
__global__ __launch_bounds__(64 * NWF, 1) void fir_fft_fwd_kernel(const float* __restrict__ x, const int64_t* __restrict__ xidx,
                                                                  const float* __restrict__ w1, float* __restrict__ y1,
                                                                  float* __restrict__ part, int C, int S, int klen, int padl,
                                                                  Units q, int nrows) {
  __shared__ v2f smem[F1 * HB + NWF * WBUF + TWSZ];
  v2f* Hs = smem;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // wave id as a scalar
  v2f* xb = smem + F1 * HB + wave * WBUF;
  const v2f* tw = smem + F1 * HB + NWF * WBUF;
  make_twiddles(smem + F1 * HB + NWF * WBUF);
  v2f v[16];
  if (wave < F1) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int n = lane + 64 * j;
      v[j] = (v2f){n < klen ? w1[wave * klen + n] : 0.f, 0.f};
    }
    fft1024<false>(v, xb, lane, tw);
#pragma unroll
    for (int j = 0; j < 8; ++j) Hs[wave * HB + j * 64 + lane] = (v2f){v[j].x, -v[j].y} * (1.0f / NF);
    if (lane == 0) Hs[wave * HB + 512] = (v2f){v[8].x, -v[8].y} * (1.0f / NF);
  }
  __syncthreads();
  float sacc = 0.f;      // lane f: sum of filter f's outputs, lane 8 + f: sum of their squares (this wave's share)
  const int wgid = blockIdx.x * NWF + wave, nwaves = gridDim.x * NWF, nunits = q.total();
  // The deal: nunits / nwaves full rounds (round r: unit r nwaves + wgid), then the remainder slot by slot - extra e goes
  // to workgroup e % gridDim.x, wave slot e / gridDim.x.  Consecutive wave slots of a workgroup sit on consecutive SIMDs,
  // so the extras of a CU spread over its four SIMDs: 13920 units on 256 x 12 waves are 4 rounds + 1632 extras = 12 + at
  // most 2 per SIMD (dealt wave after wave, the extras would fill three waves of ONE SIMD first).
  const int rounds = nunits / nwaves, xunit = rounds * nwaves + wave * (int)gridDim.x + (int)blockIdx.x;
  const int cnt = rounds + (xunit < nunits ? 1 : 0);
  auto unit_of = [&](int i) { return i < rounds ? i * nwaves + wgid : xunit; };
  // Units ascend along a wave's list and the packed tails end the unit list, so a wave runs its main units, then its packed
  // ones, in a loop of their own: the loop of whole and ragged blocks stays what it was, and the registers are the larger
  // of the two loops, not their sum (one loop with both kinds of unit took 166 VGPRs and spilled).
  int nmine = 0;
  while (nmine < cnt && unit_of(nmine) < q.nmain) ++nmine;
  auto run = [&](auto pk, int i0, int i1) {
    constexpr bool PK = decltype(pk)::value;
    const int tbt = q.t0t - padl;      // packed tails: slot 0 of each half
    // the NEXT main unit's input segment is fetched into registers before the eight inverse transforms of the current one
    v2f nx[16];
    auto fetch = [&](int u, v2f (&dst)[16]) {
      if (!PK) {
        const int blk = u % q.nmb, pr = (u / q.nmb) % q.npair, b = u / (q.nmb * q.npair);
        const int c0 = 2 * pr;
        const float* xrow = x + ((xidx ? xidx[b] : (int64_t)b) * C + c0) * S;
        load_segment(dst, xrow, c0 + 1 < C, S, blk * LB - padl, lane);
      } else {
        const Tails tl = decode_tails(q, u - q.nmain);
        const int b1 = tl.ex1 ? tl.b1 : tl.b0;      // (a missing tail reads nothing: any valid row will do)
        load_half(dst, 0, x + ((xidx ? xidx[tl.b0] : (int64_t)tl.b0) * C + tl.c0) * S, true, tl.c0 + 1 < C, S, tbt, lane);
        load_half(dst, 8, x + ((xidx ? xidx[b1] : (int64_t)b1) * C + tl.c1) * S, tl.ex1, tl.c1 + 1 < C, S, tbt, lane);
      }
    };
    if (!PK && i0 < i1) fetch(unit_of(i0), nx);
    for (int i = i0; i < i1; ++i) {
      const int u = unit_of(i);
      int b, c0, t0;
      Tails tl = {0, 0, 0, 0, false};
      if (!PK) {
        const int blk = u % q.nmb, pr = (u / q.nmb) % q.npair;
        b = u / (q.nmb * q.npair), c0 = 2 * pr, t0 = blk * LB;
      } else {
        tl = decode_tails(q, u - q.nmain);
        b = tl.b0, c0 = tl.c0, t0 = q.t0t;
      }
      const bool has1 = c0 + 1 < C;
      if (PK) {      // (a wave has one packed unit, seldom two: loaded where it is needed, no registers held for the next)
        fetch(u, v);
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = nx[j];
        if (i + 1 < i1) fetch(unit_of(i + 1), nx);
      }
      fft1024<false>(v, xb, lane, tw);
      v2f z[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) z[j] = v[j];
#pragma unroll 1
      for (int f = 0; f < F1; ++f) {
        const v2f* hp = Hs + f * HB + lane;       // bins lane + 64 j, j < 8
        const v2f* hm = Hs + f * HB - lane;       // bins 1024 - (lane + 64 j), j >= 8: the conjugates
#pragma unroll
        for (int j = 0; j < 8; j += 2)
          cmul2<false>(z[j], lds_ld(hp + 64 * j), z[j + 1], lds_ld(hp + 64 * j + 64), v[j], v[j + 1]);
#pragma unroll
        for (int j = 8; j < 16; j += 2)
          cmul2<true>(z[j], lds_ld(hm + (NF - 64 * j)), z[j + 1], lds_ld(hm + (NF - 64 * j - 64)), v[j], v[j + 1]);
        fft1024<true>(v, xb, lane, tw);
        float* dst = y1 + (((int64_t)b * F1 + f) * C + c0) * S + t0 + lane;
        float a1 = 0.f, a2 = 0.f;
        if (PK) {      // two tails: rows 0 .. 7 are A's outputs, rows 8 .. 15 B's (those at or past S are not outputs)
          store_rows<STATS, 0, 8>(v, dst, t0 + lane, S, has1, a1, a2);
          if (tl.ex1)
            store_rows<STATS, 8, 8>(v, y1 + (((int64_t)tl.b1 * F1 + f) * C + tl.c1) * S + t0 + lane, t0 + lane, S,
                                    tl.c1 + 1 < C, a1, a2);
        } else if (has1 && t0 + LB <= S) {      // a whole block of a full pair (14 of 15, or every main unit): no predicates
          v2f s1 = (v2f){0.f, 0.f}, s2 = (v2f){0.f, 0.f};
#pragma unroll
          for (int j = 0; j < NROW; ++j) {
            EAV_STG(dst + 64 * j, v[j].x);
            EAV_STG(dst + S + 64 * j, v[j].y);
            if (STATS) {
              s1 += v[j];
              s2 = fma2(v[j], v[j], s2);
            }
          }
          a1 = s1.x + s1.y;
          a2 = s2.x + s2.y;
        } else {
          store_rows<STATS, 0, NROW>(v, dst, t0 + lane, S, has1, a1, a2);
        }
        if (!STATS) continue;      // firstBN in eval mode: no batch statistics to collect (stat_part is not written)
        a1 = wave_total_dpp(a1);
        a2 = wave_total_dpp(a2);
        if (lane == f) sacc += a1;
        if (lane == 8 + f) sacc += a2;
      }
    }
  };
  run(std::false_type{}, 0, nmine);
  run(std::true_type{}, nmine, cnt);
  // (a wave without units writes its zeros; so do the rows behind the grid's own, which the sizing export counts because it
  // does not know klen and hence not whether the tails pack)
  if (STATS && lane < 16) {
    part[wgid * 16 + lane] = sacc;
    for (int r = wgid + nwaves; r < nrows; r += nwaves) part[r * 16 + lane] = 0.f;
  }
}

// ---------------------------------------------------------------------------------------------------------------- wgrad
// Workgroup = 8 waves, wave f owns filter f's spectrum accumulator.  Per group of 8 units: wave w transforms the input
// segment of unit w into LDS (register layout), then every wave walks the 8 units, forms its filter's dy block, transforms
// it and accumulates Z conj(D).  PLAIN: BatchNorm in eval mode (dy = scale g, y1 is not read).
// UNIT (with PLAIN): dy = g, no scale and no BatchNorm parameters read (bnp and y1 NULL) - the G term of the table form
// further down.
template <bool PLAIN, bool UNIT = false>
__global__ __launch_bounds__(512, 1) void fir_fft_wgrad_kernel(const float* __restrict__ x, const int64_t* __restrict__ xidx,
                                                               const float* __restrict__ y1, const float* __restrict__ g1,
                                                               const float* __restrict__ bnp, float* __restrict__ spec,
                                                               int C, int S, int padl, Units q) {
  __shared__ v2f smem[8 * NF + 8 * WBUF + TWSZ];
  v2f* zb = smem;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), f = wave;
  v2f* xb = smem + 8 * NF + wave * WBUF;
  const v2f* tw = smem + 8 * NF + 8 * WBUF;
  make_twiddles(smem + 8 * NF + 8 * WBUF);
  const float mean = UNIT ? 0.f : bnp[f], invstd = UNIT ? 0.f : bnp[8 + f], sc = UNIT ? 1.f : bnp[16 + f],
              m1 = UNIT ? 0.f : bnp[32 + f], m2 = UNIT ? 0.f : bnp[40 + f];
  v2f acc[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = (v2f){0.f, 0.f};
  v2f v[16];
  // main units first, in groups of 8; the packed tails follow in groups of their own (no mixed group: the unit body is a
  // compile-time variant).  A workgroup walks the groups blockIdx.x, + gridDim.x, ... of the joint list.
  const int nunits = q.nmain, nblk = q.nmb, npair = q.npair;
  const int ngroups = (nunits + 7) >> 3, ngpk = (q.npk + 7) >> 3;
  // raw g1 (and y1) rows of a unit for this wave's filter: .x = electrode c0, .y = electrode c0 + 1 (0 outside)
  v2f cg[NROW], cy[NROW];
  // (block, pair, sample) of a unit: one set of integer divisions per GROUP (they compile to ~60 scalar instructions each);
  // inside a group the position is advanced
  struct Pos { int blk, pr, b; };
  auto decode = [&](int u) { return Pos{u % nblk, (u / nblk) % npair, u / (nblk * npair)}; };
  auto advance = [&](Pos& q) {
    if (++q.blk == nblk) {
      q.blk = 0;
      if (++q.pr == npair) q.pr = 0, ++q.b;
    }
  };
  auto fetch_raw = [&](const Pos& q, v2f (&gr)[NROW], v2f (&yr)[NROW]) {
    const int blk = q.blk, pr = q.pr, b = q.b;
    const int c0 = 2 * pr, t0 = blk * LB;
    const bool has1 = c0 + 1 < C;
    const int64_t off = (((int64_t)b * F1 + f) * C + c0) * S + t0 + lane;
    if (has1 && t0 + LB <= S) {      // a whole block of a full pair: no predicates
#pragma unroll
      for (int j = 0; j < NROW; ++j) {
        gr[j] = (v2f){EAV_LDG(g1 + off + 64 * j), EAV_LDG(g1 + off + S + 64 * j)};
        if (!PLAIN) yr[j] = (v2f){EAV_LDG(y1 + off + 64 * j), EAV_LDG(y1 + off + S + 64 * j)};
      }
      return;
    }
#pragma unroll
    for (int j = 0; j < NROW; ++j) {
      const bool ok = t0 + lane + 64 * j < S;
      gr[j].x = ok ? EAV_LDG(g1 + off + 64 * j) : 0.f;
      gr[j].y = (ok && has1) ? EAV_LDG(g1 + off + S + 64 * j) : 0.f;
      if (!PLAIN) {
        yr[j].x = ok ? EAV_LDG(y1 + off + 64 * j) : 0.f;
        yr[j].y = (ok && has1) ? EAV_LDG(y1 + off + S + 64 * j) : 0.f;
      }
    }
  };
  Pos cur = {0, 0, 0};      // the unit whose rows are in cg / cy
  if (blockIdx.x * 8 < nunits) {
    cur = decode(blockIdx.x * 8);
    fetch_raw(cur, cg, cy);
  }
  // input segment of this wave's unit of a group: fetched one group ahead, so that the Z transforms that open a group
  // find their data in registers (the loads travel under the previous group's eight dy transforms)
  v2f nx[16];
  auto fetch_x = [&](int u, v2f (&dst)[16]) {
    const int blk = u % nblk, pr = (u / nblk) % npair, b = u / (nblk * npair);
    const int c0 = 2 * pr;
    const float* xrow = x + ((xidx ? xidx[b] : (int64_t)b) * C + c0) * S;
    load_segment(dst, xrow, c0 + 1 < C, S, blk * LB - padl, lane);
  };
  if (blockIdx.x * 8 + wave < nunits) fetch_x(blockIdx.x * 8 + wave, nx);
  for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
    if (g * 8 + wave < nunits) {
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = nx[j];
      const int un = (g + (int)gridDim.x) * 8 + wave;
      if (un < nunits) fetch_x(un, nx);
      fft1024<false>(v, xb, lane, tw);
#pragma unroll
      for (int j = 0; j < 16; ++j) zb[wave * NF + j * 64 + lane] = v[j];
    }
    __syncthreads();
#pragma unroll 1
    for (int uu = 0; uu < 8; ++uu) {
      const int u = g * 8 + uu;
      if (u >= nunits) break;
      const int t0 = cur.blk * LB;
      const bool has1 = 2 * cur.pr + 1 < C;
      // the next unit's rows (of this group, or the first of this workgroup's next group - they then travel under that
      // group's Z transforms too) are in flight under this unit's transform; they are consumed one iteration later
      v2f ng[NROW], ny[NROW];
      const int nu = (uu + 1 < 8) ? u + 1 : (g + (int)gridDim.x) * 8;
      if (uu + 1 < 8) advance(cur);
      else if (nu < nunits) cur = decode(nu);
      if (nu < nunits) fetch_raw(cur, ng, ny);
#pragma unroll
      for (int j = 0; j < NROW; ++j) {
        if (UNIT) {
          v[j] = cg[j];
        } else if (PLAIN) {
          v[j] = sc * cg[j];
        } else {
          v[j] = sc * (cg[j] - m1 - (cy[j] - mean) * invstd * m2);
        }
      }
      if (!(has1 && t0 + LB <= S)) {      // ragged last block / odd electrode count: zero what lies outside
#pragma unroll
        for (int j = 0; j < NROW; ++j) {
          if (t0 + lane + 64 * j >= S) v[j] = (v2f){0.f, 0.f};
          if (!has1) v[j].y = 0.f;
        }
      }
#pragma unroll
      for (int j = NROW; j < 16; ++j) v[j] = (v2f){0.f, 0.f};
      fft1024<false>(v, xb, lane, tw);
      const v2f* zp = zb + uu * NF + lane;
#pragma unroll
      for (int j = 0; j < 16; j += 2) cmacc2_conj(lds_ld(zp + 64 * j), v[j], lds_ld(zp + 64 * j + 64), v[j + 1], acc[j], acc[j + 1]);
#pragma unroll
      for (int j = 0; j < NROW; ++j) {       // (after the transform: the copy is what waits for the loads)
        cg[j] = ng[j];
        if (!PLAIN) cy[j] = ny[j];
      }
    }
    __syncthreads();
  }
  // Groups of packed tails: the same walk with both halves of a unit - dy rows 0 .. 7 from tail A's g1 / y1, rows 8 .. 15
  // from tail B's, zero at and past S.  All 16 rows can be live (a short filter packs tails of up to 7 rows), so the rows
  // of the next unit go straight into pg / py once the current ones are consumed; cg / cy and their copies are dead here.
  int gp = (int)blockIdx.x - ngroups;
  if (gp < 0) gp += (-gp + (int)gridDim.x - 1) / (int)gridDim.x * (int)gridDim.x;
  if (gp < ngpk) {
    const int tbt = q.t0t - padl;
    v2f pg[16], py[16];
    auto half_raw = [&](int j0, int b, int c0, bool ex, v2f (&gr)[16], v2f (&yr)[16]) {
      const bool has1 = c0 + 1 < C;
      const int64_t off = (((int64_t)b * F1 + f) * C + c0) * S + q.t0t + lane;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool ok = ex && q.t0t + lane + 64 * j < S;
        gr[j0 + j].x = ok ? EAV_LDG(g1 + off + 64 * j) : 0.f;
        gr[j0 + j].y = (ok && has1) ? EAV_LDG(g1 + off + S + 64 * j) : 0.f;
        if (!PLAIN) {
          yr[j0 + j].x = ok ? EAV_LDG(y1 + off + 64 * j) : 0.f;
          yr[j0 + j].y = (ok && has1) ? EAV_LDG(y1 + off + S + 64 * j) : 0.f;
        }
      }
    };
    auto fetch_raw_pk = [&](int p, v2f (&gr)[16], v2f (&yr)[16]) {
      const Tails tl = decode_tails(q, p);
      half_raw(0, tl.b0, tl.c0, true, gr, yr);
      half_raw(8, tl.ex1 ? tl.b1 : tl.b0, tl.c1, tl.ex1, gr, yr);
    };
    auto fetch_x_pk = [&](int p, v2f (&dst)[16]) {
      const Tails tl = decode_tails(q, p);
      const int b1 = tl.ex1 ? tl.b1 : tl.b0;
      load_half(dst, 0, x + ((xidx ? xidx[tl.b0] : (int64_t)tl.b0) * C + tl.c0) * S, true, tl.c0 + 1 < C, S, tbt, lane);
      load_half(dst, 8, x + ((xidx ? xidx[b1] : (int64_t)b1) * C + tl.c1) * S, tl.ex1, tl.c1 + 1 < C, S, tbt, lane);
    };
    fetch_raw_pk(gp * 8, pg, py);
    if (gp * 8 + wave < q.npk) fetch_x_pk(gp * 8 + wave, nx);
    for (; gp < ngpk; gp += gridDim.x) {
      if (gp * 8 + wave < q.npk) {
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = nx[j];
        const int pn = (gp + (int)gridDim.x) * 8 + wave;
        if (pn < q.npk) fetch_x_pk(pn, nx);
        fft1024<false>(v, xb, lane, tw);
#pragma unroll
        for (int j = 0; j < 16; ++j) zb[wave * NF + j * 64 + lane] = v[j];
      }
      __syncthreads();
#pragma unroll 1
      for (int uu = 0; uu < 8; ++uu) {
        const int p = gp * 8 + uu;
        if (p >= q.npk) break;
        const Tails tl = decode_tails(q, p);
        const bool has0 = tl.c0 + 1 < C, has1 = tl.c1 + 1 < C;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          if (UNIT) {
            v[j] = pg[j];
          } else if (PLAIN) {
            v[j] = sc * pg[j];
          } else {
            v[j] = sc * (pg[j] - m1 - (py[j] - mean) * invstd * m2);
          }
          // zero what is no output: past S, the missing electrode of an odd count, the upper half of a tail that stands alone
          const bool ok = q.t0t + lane + 64 * (j & 7) < S && (j < 8 || tl.ex1);
          if (!ok) v[j] = (v2f){0.f, 0.f};
          if (!(j < 8 ? has0 : has1)) v[j].y = 0.f;
        }
        const int np = (uu + 1 < 8) ? p + 1 : (gp + (int)gridDim.x) * 8;
        if (np < q.npk) fetch_raw_pk(np, pg, py);
        fft1024<false>(v, xb, lane, tw);
        const v2f* zp = zb + uu * NF + lane;
#pragma unroll
        for (int j = 0; j < 16; j += 2)
          cmacc2_conj(lds_ld(zp + 64 * j), v[j], lds_ld(zp + 64 * j + 64), v[j + 1], acc[j], acc[j + 1]);
      }
      __syncthreads();
    }
  }
  float* out = spec + ((int64_t)blockIdx.x * F1 + f) * (2 * NF);
#pragma unroll
  for (int j = 0; j < 16; ++j) *reinterpret_cast<v2f*>(out + 2 * (j * 64 + lane)) = acc[j];
}

// Finish in two small launches.  (1) 256 workgroups = (filter, slice of 32 bins): 16 thread groups each sum every sixteenth
// per-workgroup spectrum of their bins in order (at 225 partials: 14 or 15 loads per thread, all in flight together), the
// 16 group sums are added as a fixed tree - bit-reproducible - and the total goes to row `nparts` of the workspace.
// (2) One wave per filter transforms the total back and keeps the real parts of lags 0 .. klen - 1.  (One workgroup per
// filter doing both took 30 us at 225 partials; 64 workgroups of 4 groups 16.6 us: a chain of 56 loads per thread.)
__device__ __forceinline__ void wgrad_spec_sum(float* __restrict__ spec, int nparts, v2f* __restrict__ red) {
  const int f = blockIdx.x >> 5, bin = (blockIdx.x & 31) * 32 + (threadIdx.x & 31), grp = threadIdx.x >> 5;
  const v2f* src = reinterpret_cast<const v2f*>(spec) + (int64_t)f * NF + bin;
  v2f a = (v2f){0.f, 0.f};
#pragma unroll 4
  for (int p = grp; p < nparts; p += 16) a += src[(int64_t)p * F1 * NF];
  red[threadIdx.x] = a;
  __syncthreads();
  if (threadIdx.x < 128) {                 // groups g, g + 4, g + 8, g + 12
    a = (red[threadIdx.x] + red[threadIdx.x + 128]) + (red[threadIdx.x + 256] + red[threadIdx.x + 384]);
    red[threadIdx.x] = a;
  }
  __syncthreads();
  if (threadIdx.x < 32) {
    a = (red[threadIdx.x] + red[threadIdx.x + 32]) + (red[threadIdx.x + 64] + red[threadIdx.x + 96]);
    reinterpret_cast<v2f*>(spec)[((int64_t)nparts * F1 + f) * NF + bin] = a;
  }
}
__global__ __launch_bounds__(512) void fir_fft_wgrad_sum_kernel(float* __restrict__ spec, int nparts) {
  __shared__ v2f red[512];
  wgrad_spec_sum(spec, nparts, red);
}

__global__ __launch_bounds__(64) void fir_fft_wgrad_finish_kernel(const float* __restrict__ spec, int nparts,
                                                                  float* __restrict__ dW, int klen) {
  __shared__ v2f smem[WBUF + TWSZ];
  const int lane = threadIdx.x, f = blockIdx.x;
  make_twiddles(smem + WBUF);
  v2f v[16];
  const v2f* src = reinterpret_cast<const v2f*>(spec) + ((int64_t)nparts * F1 + f) * NF + lane;
#pragma unroll
  for (int j = 0; j < 16; ++j) v[j] = src[64 * j];
  fft1024<true>(v, smem, lane, smem + WBUF);
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int n = lane + 64 * j;
    if (n < klen) dW[f * klen + n] = v[j].x * (1.0f / NF);
  }
}

// ----------------------------------------------------------------------------------------- wgrad from per-trial input tables
// The train-mode weight gradient reads y1 only to form dy = scale (g - m1 - (y1 - mean) invstd m2) while loading.  y1 is
// firstConv(x), so its share of dW is a function of x and w alone.  With xp = the row zero-padded by (left, K - 1 - left):
//   dW[f,k] = scale_f ( G[f,k] - (m1_f - mean_f invstd_f m2_f) X1[k] - invstd_f m2_f Y[f,k] )
//   G[f,k]  = sum_{b,c,t<S} g1[b,f,c,t] xp[b,c,t+k]          the PLAIN walk on the raw g1 (fir_fft_wgrad_kernel<true, true>)
//   X1[k]   = sum_b X1_b[k],  X1_b[k]   = sum_c sum_{t<S} xp[t+k]
//   Y[f,k]  = sum_j w[f,j] A[j,k],  A = sum_b A_b,  A_b[j,k] = sum_c sum_{t<S} xp[t+j] xp[t+k]      (symmetric, K x K)
// A_b and X1_b depend on trial b of the data set alone: a table of K K + K floats per trial (A_b row-major, then X1_b), built
// once per data set by fir_xtab_build_kernel; a step sums the rows of its batch.  Every sum below is formed in float64 in
// a fixed order and rounded once.
__host__ __device__ inline int64_t xtab_stride(int klen) { return (int64_t)klen * klen + klen; }

// xp[u] of a row of S samples
__device__ __forceinline__ double xpad(const float* __restrict__ row, int S, int left, int u) {
  const int t = u - left;
  return (t >= 0 && t < S) ? (double)row[t] : 0.0;
}
// a[tid] = sum of the 256 entries of a, as a fixed tree
__device__ __forceinline__ double block_sum256(double* a, int tid) {
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) a[tid] += a[tid + s];
    __syncthreads();
  }
  return a[0];
}

// Workgroup = (trial b, lag d): the diagonal A_b[j, j + d], j < K - d, of the table, its mirror, and X1_b[d].  With
// R = sum_c sum_{u<S} xp[u] xp[u+d] (one autocorrelation lag per row) the diagonal is R less the products of the first j
// samples plus those of the j samples from S on:
//   A_b[j, j+d] = sum_{u=j}^{S+j-1} xp[u] xp[u+d] = R - sum_{u<j} xp[u] xp[u+d] + sum_{S<=u<S+j} xp[u] xp[u+d]
// (u + d <= S + K - 2 throughout: j + d <= K - 1).
__global__ __launch_bounds__(256) void fir_xtab_build_kernel(const float* __restrict__ x, float* __restrict__ tab, int C, int S,
                                                             int klen) {
  __shared__ double ra[256], rb[256], hs[MAXK];
  const int d = blockIdx.x % klen, b = blockIdx.x / klen, tid = threadIdx.x, left = (klen - 1) / 2;
  const float* xb = x + (int64_t)b * C * S;
  float* A = tab + (int64_t)b * xtab_stride(klen);
  double r = 0.0, s1 = 0.0;
  for (int c = 0; c < C; ++c) {
    const float* row = xb + (int64_t)c * S;
    for (int u = tid; u < S; u += 256) {
      const double q = xpad(row, S, left, u + d);
      r = fma(xpad(row, S, left, u), q, r);
      s1 += q;
    }
  }
  ra[tid] = r;
  rb[tid] = s1;
  const double R = block_sum256(ra, tid), X1 = block_sum256(rb, tid);
  const int nj = klen - d;
  // hs[j] = (products of the j-th sample from S on) - (products of the j-th sample), over the rows
  for (int j = tid; j < nj; j += 256) {
    double h = 0.0, t = 0.0;
    for (int c = 0; c < C; ++c) {
      const float* row = xb + (int64_t)c * S;
      h = fma(xpad(row, S, left, j), xpad(row, S, left, j + d), h);
      t = fma(xpad(row, S, left, S + j), xpad(row, S, left, S + j + d), t);
    }
    hs[j] = t - h;
  }
  __syncthreads();
  if (tid == 0) {      // hs[j] <- A_b[j, j + d]: the running sum, in order
    double a = R;
    for (int j = 0; j < nj; ++j) {
      const double nxt = a + hs[j];
      hs[j] = a;
      a = nxt;
    }
    A[(int64_t)klen * klen + d] = (float)X1;
  }
  __syncthreads();
  for (int j = tid; j < nj; j += 256) {
    const float a = (float)hs[j];
    A[j * klen + j + d] = a;
    A[(j + d) * klen + j] = a;
  }
}

// The first finishing launch with the batch's tables riding in it: acc[0 .. K K) = A = sum_b A_{xidx[b]}, acc[K K .. + K) = X1,
// in float64, b = 0 .. B - 1 in order.  A is symmetric: the upper triangle is read, both halves are written.
__global__ __launch_bounds__(512) void fir_fft_wgrad_sum_tab_kernel(float* __restrict__ spec, int nparts,
                                                                    const float* __restrict__ tab,
                                                                    const int64_t* __restrict__ xidx, int B, int klen,
                                                                    double* __restrict__ acc) {
  __shared__ v2f red[512];
  wgrad_spec_sum(spec, nparts, red);
  const int64_t stride = xtab_stride(klen);
  const int n = (int)stride;
  for (int e = blockIdx.x * 512 + threadIdx.x; e < n; e += gridDim.x * 512) {
    const int j = e / klen, k = e - j * klen;      // j == klen: the X1 row
    if (j < klen && k < j) continue;
    double a = 0.0;
#pragma unroll 16
    for (int b = 0; b < B; ++b) a += (double)tab[(xidx ? xidx[b] : (int64_t)b) * stride + e];
    acc[e] = a;
    if (j < klen && k > j) acc[k * klen + j] = a;
  }
}

// The second: workgroup = (filter f, 64 lags k).  Wave 0 transforms the summed spectrum back (G, as
// fir_fft_wgrad_finish_kernel) while each of the 16 waves forms its slice of Y[f,k] = sum_j w[f,j] A[j,k]; the slices are
// added in order and the combination above is rounded to fp32 once.
__global__ __launch_bounds__(1024) void fir_fft_wgrad_finish_tab_kernel(const float* __restrict__ spec, int nparts,
                                                                        const double* __restrict__ acc,
                                                                        const float* __restrict__ w1,
                                                                        const float* __restrict__ bnp, float* __restrict__ dW,
                                                                        int klen) {
  __shared__ v2f smem[WBUF + TWSZ];
  __shared__ double ys[16][64];
  __shared__ float gs[64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), f = blockIdx.x;
  const int kb = blockIdx.y, k = kb * 64 + lane;
  make_twiddles(smem + WBUF);
  const int jn = (klen + 15) / 16, j0 = wave * jn, j1 = min(klen, j0 + jn);
  double y = 0.0;
  if (k < klen)
    for (int j = j0; j < j1; ++j) y = fma((double)w1[f * klen + j], acc[j * klen + k], y);
  ys[wave][lane] = y;
  if (wave == 0) {
    v2f v[16];
    const v2f* src = reinterpret_cast<const v2f*>(spec) + ((int64_t)nparts * F1 + f) * NF + lane;
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = src[64 * j];
    fft1024<true>(v, smem, lane, smem + WBUF);
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (j == kb) gs[lane] = v[j].x;      // lag lane + 64 j
  }
  __syncthreads();
  if (wave == 0 && k < klen) {
    double Y = 0.0;
#pragma unroll
    for (int w = 0; w < 16; ++w) Y += ys[w][lane];
    const double mean = bnp[f], invstd = bnp[8 + f], sc = bnp[16 + f], m1 = bnp[32 + f], m2 = bnp[40 + f];
    const double G = (double)gs[lane] * (1.0 / NF), X1 = acc[klen * klen + k];
    dW[f * klen + k] = (float)(sc * (G - (m1 - mean * invstd * m2) * X1 - invstd * m2 * Y));
  }
}

// weight gradient: workgroups of 8 waves, at most one per CU, over `items` groups of 8 units: the smallest grid that needs
// no more rounds than 256 workgroups would (13920 units = 1680 + 60 groups: 249 workgroups x 7 rounds; unpacked, 1800
// groups took 8 rounds on 225)
// (the 256 of both grids is one workgroup per CU; eav_eegnet_fir_fft_set_grid_cap - tests and tuning only - lowers it so
// that the multi-round paths of both kernels are reached at small shapes)
int g_grid_cap = 0;
int grid_cap() { return g_grid_cap > 0 ? g_grid_cap : 256; }
int fft_grid(int items) {
  const int cap = grid_cap();
  if (items <= cap) return std::max(1, items);
  const int rounds = cdiv(items, cap);
  return cdiv(items, rounds);
}
int wgrad_groups(const Units& q) { return cdiv(q.nmain, 8) + cdiv(q.npk, 8); }
// forward: one workgroup of NWF waves per CU while the units last (the kernel deals them round by round, then slot by slot)
int fwd_grid(const Units& q) { return std::min(grid_cap(), std::max(1, cdiv(q.total(), NWF))); }
// The sizing exports do not know klen, hence not whether the tails pack: they take the larger of the two lists (klen = 1
// packs whenever any filter does, klen = NF never).
constexpr int K_PACKS = 1, K_NEVER = NF;

}  // namespace

extern "C" int eav_eegnet_fir_fft_max_taps(void) { return MAXK; }

// test / tuning only (include/eav_hip_tuning.h): the most workgroups either kernel launches; n <= 0 restores 256.  The
// sizing exports and the plan below follow it, so buffers sized after the call fit the launches after it.
extern "C" int eav_eegnet_fir_fft_set_grid_cap(int n) {
  g_grid_cap = n > 0 ? n : 0;
  return 0;
}

// The unit list and both grids for a shape, from the very functions the launchers call (host only, no GPU needed):
// out[0..9) = npair, nmb, nmain, ntail, npk, t0t, forward workgroups, weight-gradient groups, weight-gradient workgroups
extern "C" int eav_eegnet_fir_fft_plan(int B, int C, int S, int klen, int* out) {
  EAV_REQUIRE(out && B > 0 && C > 0 && S > 0, "eav_eegnet_fir_fft_plan: bad arguments");
  EAV_REQUIRE(klen >= 1 && klen <= MAXK, "eav_eegnet_fir_fft_plan: kernLength %d outside [1,%d]", klen, MAXK);
  const Units q = fft_units(B, C, S, klen);
  const int groups = wgrad_groups(q);
  const int v[EAV_FIR_FFT_PLAN_FIELDS] = {q.npair, q.nmb, q.nmain, q.ntail, q.npk, q.t0t, fwd_grid(q), groups, fft_grid(groups)};
  std::copy(v, v + EAV_FIR_FFT_PLAN_FIELDS, out);
  return EAV_OK;
}

// stat_part rows (16 floats each: 8 sums, 8 sums of squares) the forward writes - one per wave, and zeros in those a
// shorter unit list leaves without a wave
extern "C" int eav_eegnet_fir_fwd_fft_nparts(int B, int C, int S) {
  return std::max(fwd_grid(fft_units(B, C, S, K_PACKS)), fwd_grid(fft_units(B, C, S, K_NEVER))) * NWF;
}

// y1 [B,8,C,S] = firstConv(x) for the batch x[xidx[0..B)] (xidx NULL: x itself), 'same' padding, klen <= 321 taps;
// stat_part [eav_eegnet_fir_fwd_fft_nparts][16]: per-wave sums / sums of squares per filter (input of eav_bn_finalize); NULL:
// none (firstBN in eval mode takes its running statistics - the sums, their wave totals and the partial rows are skipped).
extern "C" int eav_eegnet_fir_fwd_fft(const float* x, const int64_t* xidx, const float* w1, float* y1, float* stat_part,
                                      int B, int C, int S, int klen, void* stream) {
  EAV_REQUIRE(x && w1 && y1 && B > 0 && C > 0 && S > 0, "eav_eegnet_fir_fwd_fft: bad arguments");
  EAV_REQUIRE(klen >= 1 && klen <= MAXK, "eav_eegnet_fir_fwd_fft: kernLength %d outside [1,%d]", klen, MAXK);
  const Units q = fft_units(B, C, S, klen);
  const int grid = fwd_grid(q), nrows = eav_eegnet_fir_fwd_fft_nparts(B, C, S);
  if (stat_part)
    hipLaunchKernelGGL(fir_fft_fwd_kernel<true>, dim3(grid), dim3(64 * NWF), 0, (hipStream_t)stream, x, xidx, w1, y1,
                       stat_part, C, S, klen, (klen - 1) / 2, q, nrows);
  else      // firstBN in eval mode: running statistics, nothing to collect
    hipLaunchKernelGGL(fir_fft_fwd_kernel<false>, dim3(grid), dim3(64 * NWF), 0, (hipStream_t)stream, x, xidx, w1, y1,
                       stat_part, C, S, klen, (klen - 1) / 2, q, nrows);
  EAV_CHECK_LAUNCH("eav_eegnet_fir_fwd_fft");
  return EAV_OK;
}

// floats of the spectrum workspace of eav_eegnet_fir_wgrad_fft: one row per workgroup + one, the sum of the others
extern "C" int64_t eav_eegnet_fir_wgrad_fft_ws_floats(int B, int C, int S) {
  const int gp = fft_grid(wgrad_groups(fft_units(B, C, S, K_PACKS))), gn = fft_grid(wgrad_groups(fft_units(B, C, S, K_NEVER)));
  return ((int64_t)std::max(gp, gn) + 1) * F1 * 2 * NF;      // (fewer groups can mean MORE workgroups: 1740 -> 249, 1800 -> 225)
}

// dW [8, klen] = d loss / d firstConv.weight (written, not accumulated).  g1 = d loss / d(firstBN output) [B,8,C,S];
// y1 = the saved FIR output, or NULL for BatchNorm in eval mode (dy = scale g); bn_params as eav_bn_finalize /
// eav_bn_bwd_finalize leave them (mean, invstd, scale at 0 / 8 / 16, the backward means m1 / m2 at 32 / 40).
extern "C" int eav_eegnet_fir_wgrad_fft(const float* x, const int64_t* xidx, const float* y1, const float* g1,
                                        const float* bn_params, float* ws, float* dW, int B, int C, int S, int klen,
                                        void* stream) {
  EAV_REQUIRE(x && g1 && bn_params && ws && dW && B > 0 && C > 0 && S > 0, "eav_eegnet_fir_wgrad_fft: bad arguments");
  EAV_REQUIRE(klen >= 1 && klen <= MAXK, "eav_eegnet_fir_wgrad_fft: kernLength %d outside [1,%d]", klen, MAXK);
  const Units q = fft_units(B, C, S, klen);
  const int grid = fft_grid(wgrad_groups(q));
  hipStream_t st = (hipStream_t)stream;
  if (y1)
    hipLaunchKernelGGL(fir_fft_wgrad_kernel<false>, dim3(grid), dim3(512), 0, st, x, xidx, y1, g1, bn_params, ws, C, S,
                       (klen - 1) / 2, q);
  else
    hipLaunchKernelGGL(fir_fft_wgrad_kernel<true>, dim3(grid), dim3(512), 0, st, x, xidx, y1, g1, bn_params, ws, C, S,
                       (klen - 1) / 2, q);
  EAV_CHECK_LAUNCH("eav_eegnet_fir_wgrad_fft");
  hipLaunchKernelGGL(fir_fft_wgrad_sum_kernel, dim3(F1 * 32), dim3(512), 0, st, ws, grid);
  EAV_CHECK_LAUNCH("eav_eegnet_fir_wgrad_fft(sum)");
  hipLaunchKernelGGL(fir_fft_wgrad_finish_kernel, dim3(F1), dim3(64), 0, st, ws, grid, dW, klen);
  EAV_CHECK_LAUNCH("eav_eegnet_fir_wgrad_fft(finish)");
  return EAV_OK;
}

// floats of the input tables of N trials: per trial A_b [klen][klen] row-major, then X1_b [klen]
extern "C" int64_t eav_eegnet_fir_xtab_floats(int N, int klen) { return (int64_t)N * xtab_stride(klen); }

// tab [N][klen klen + klen] = the tables of the trials x [N,C,S] (float64 sums, rounded once; deterministic).  Once per data
// set - and again whenever x changes - never inside a step.
extern "C" int eav_eegnet_fir_xtab_build(const float* x, int N, int C, int S, int klen, float* tab, void* stream) {
  EAV_REQUIRE(x && tab && N > 0 && C > 0 && S > 0, "eav_eegnet_fir_xtab_build: bad arguments");
  EAV_REQUIRE(klen >= 1 && klen <= MAXK, "eav_eegnet_fir_xtab_build: kernLength %d outside [1,%d]", klen, MAXK);
  EAV_REQUIRE((int64_t)N * klen < (int64_t)1 << 31, "eav_eegnet_fir_xtab_build: %d trials are too many", N);
  hipLaunchKernelGGL(fir_xtab_build_kernel, dim3(N * klen), dim3(256), 0, (hipStream_t)stream, x, tab, C, S, klen);
  EAV_CHECK_LAUNCH("eav_eegnet_fir_xtab_build");
  return EAV_OK;
}

// workspace of eav_eegnet_fir_wgrad_fft_xtab: that of eav_eegnet_fir_wgrad_fft, then klen klen + klen doubles (A and X1)
extern "C" int64_t eav_eegnet_fir_wgrad_fft_xtab_ws_floats(int B, int C, int S, int klen) {
  return eav_eegnet_fir_wgrad_fft_ws_floats(B, C, S) + 2 * xtab_stride(klen);
}

// The train-mode dW of eav_eegnet_fir_wgrad_fft without its y1 read, for y1 = firstConv(x; w1): the main kernel walks the
// raw g1 as in eval mode, the share of y1 comes from the tables tab (eav_eegnet_fir_xtab_build of the array x points to; row
// xidx[b], or b, is the table of sample b of the batch - repeated indices count as often as they occur) in the two finishing
// launches.  ws: eav_eegnet_fir_wgrad_fft_xtab_ws_floats floats, 8-byte aligned.  Agrees with eav_eegnet_fir_wgrad_fft to
// rounding, not bit for bit; bit-reproducible run to run.
extern "C" int eav_eegnet_fir_wgrad_fft_xtab(const float* x, const int64_t* xidx, const float* tab, const float* w1,
                                             const float* g1, const float* bn_params, float* ws, float* dW, int B, int C,
                                             int S, int klen, void* stream) {
  EAV_REQUIRE(x && tab && w1 && g1 && bn_params && ws && dW && B > 0 && C > 0 && S > 0,
              "eav_eegnet_fir_wgrad_fft_xtab: bad arguments");
  EAV_REQUIRE(klen >= 1 && klen <= MAXK, "eav_eegnet_fir_wgrad_fft_xtab: kernLength %d outside [1,%d]", klen, MAXK);
  EAV_REQUIRE(((uintptr_t)ws & 7) == 0, "eav_eegnet_fir_wgrad_fft_xtab: ws is not 8-byte aligned");
  const Units q = fft_units(B, C, S, klen);
  const int grid = fft_grid(wgrad_groups(q));
  double* acc = reinterpret_cast<double*>(ws + eav_eegnet_fir_wgrad_fft_ws_floats(B, C, S));
  hipStream_t st = (hipStream_t)stream;
  const float* none = nullptr;
  hipLaunchKernelGGL((fir_fft_wgrad_kernel<true, true>), dim3(grid), dim3(512), 0, st, x, xidx, none, g1, none, ws, C, S,
                     (klen - 1) / 2, q);
  EAV_CHECK_LAUNCH("eav_eegnet_fir_wgrad_fft_xtab");
  hipLaunchKernelGGL(fir_fft_wgrad_sum_tab_kernel, dim3(F1 * 32), dim3(512), 0, st, ws, grid, tab, xidx, B, klen, acc);
  EAV_CHECK_LAUNCH("eav_eegnet_fir_wgrad_fft_xtab(sum)");
  hipLaunchKernelGGL(fir_fft_wgrad_finish_tab_kernel, dim3(F1, cdiv(klen, 64)), dim3(1024), 0, st, ws, grid, acc, w1,
                     bn_params, dW, klen);
  EAV_CHECK_LAUNCH("eav_eegnet_fir_wgrad_fft_xtab(finish)");
  return EAV_OK;
}
