// Row pieces of the cross-entropy "finish" family (ce.hip), which follows the logits GEMM's softmax epilogue (gemm_bf16.hip).  Per session
// row and column group the epilogue left one float2 pair — grouped form: (m_g, s_g) = (group maximum, sum of exp(x - m_g)); anchored
// form: (sum of the plane's ROUNDED entries, sum of the exponentials) — and the bf16 plane of exponentials.  Every kernel of the family
// is a front end over these functions, so the forms that must agree bit for bit (one launch / two launches, whole catalog / shard) do
// so by construction: one fold order, one label rule, one rounding of a piece, one row tail.
// Folds: ONE WAVE per row; lane `lane` owns the pairs of groups lane, lane + 64, ... and hands them over through an accessor
// pair(j) = its j-th pair (registers or memory), `n` of them.  Per lane in that order, then the shuffle tree: the same bits everywhere.
#pragma once
#include "tcar_common.h"
#include "tcar_bf16_layout.h"

typedef __attribute__((ext_vector_type(4))) __bf16 ce_bf16x4;

constexpr int CE_NG = 8;                       // pairs per lane and row a register path holds: ngroups <= 512
constexpr int CE_NO_LABEL = -(1 << 30);        // "the row's label is not a column of this plane"

// the lane's pairs of one row into registers; beyond ngroups: `none`, the identity of the fold that follows
__device__ __forceinline__ void ce_load_pairs(float2 (&pr)[CE_NG], const float2* __restrict__ st, int ngroups, int lane, float2 none) {
#pragma unroll
  for (int j = 0; j < CE_NG; ++j) {
    const int g = lane + 64 * j;
    pr[j] = g < ngroups ? st[g] : make_float2(none.x, none.y);      // (a prvalue: the pair stays ONE 8-byte load)
  }
}
// how many pairs of a row the lane owns (the trip count of `for (g = lane; g < ngroups; g += 64)`)
__device__ __forceinline__ int ce_lane_pairs(int ngroups, int lane) { return (ngroups - lane + 63) >> 6; }

// grouped pairs -> (M, S) = (max_g m_g, sum_g s_g exp(m_g - M)); an empty group (m_g = -inf: the identity) is skipped
template <class Pair>
__device__ __forceinline__ float2 ce_fold_max_sumexp(int n, Pair pair) {
  float m = -INFINITY;
  for (int j = 0; j < n; ++j) m = fmaxf(m, pair(j).x);
  m = wave_max(m);
  float s = 0.f;
  for (int j = 0; j < n; ++j) {
    const float2 v = pair(j);
    if (v.x != -INFINITY) s += v.y * expf(v.x - m);
  }
  return make_float2(m, wave_sum(s));
}
// ... over the row's pairs in memory
__device__ __forceinline__ float2 ce_row_max_sumexp(const float2* __restrict__ st, int ngroups, int lane) {
  return ce_fold_max_sumexp(ce_lane_pairs(ngroups, lane), [&](int j) { return st[lane + 64 * j]; });
}

// anchored pairs -> (sum of .x, sum of .y): plain sums (identity (0, 0)); the lane's part ...
template <class Pair>
__device__ __forceinline__ float2 ce_lane_sums(int n, Pair pair) {
  float a = 0.f, b = 0.f;
  for (int j = 0; j < n; ++j) {
    const float2 v = pair(j);
    a += v.x;
    b += v.y;
  }
  return make_float2(a, b);
}
// ... and one row's fold: out of registers, every load issued before the first use, while the row's pairs fit; the loop beyond
__device__ __forceinline__ float2 ce_row_sums(const float2* __restrict__ st, int ngroups, int lane) {
  float2 s;
  if (ngroups <= 64 * CE_NG) {
    float2 pr[CE_NG];
    ce_load_pairs(pr, st, ngroups, lane, make_float2(0.f, 0.f));
    s = ce_lane_sums(CE_NG, [&](int j) { return pr[j]; });
  } else {
    s = ce_lane_sums(ce_lane_pairs(ngroups, lane), [&](int j) { return st[lane + 64 * j]; });
  }
  s.x = wave_sum(s.x);
  s.y = wave_sum(s.y);
  return s;
}

// the label's column in a plane of N columns that starts at catalog item lab_off.  lab_window == 0: clamped into the plane;
// lab_window != 0 (catalog shard): a label of another shard matches nothing
__device__ __forceinline__ int ce_label_col(int label, int lab_off, int N, int lab_window) {
  const int lraw = label - lab_off;
  return lab_window ? ((lraw >= 0 && lraw < N) ? lraw : CE_NO_LABEL) : clampi(lraw, 0, N - 1);
}

// (a launch that carries a completion flag — the fork to the dE GEMM's stream — stores the plane write-through; tcar_common.h)
__device__ __forceinline__ void ce_store16(uint4* p, uint4 v, bool wt) {
  if (wt) {
    typedef unsigned u4_t __attribute__((ext_vector_type(4)));
    const u4_t x = {v.x, v.y, v.z, v.w};
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(x) : "memory");
  } else {
    *p = v;
  }
}

// One 16-byte piece of the grouped plane in place: eight entries e -> bf16(e * exp(m_g - M) / S - [column == label]) = softmax - onehot.
// x: the piece's bits; rs = (M, 1 / S) of the row; strow: the row's pairs; col0: first column of the piece's 32-column block;
// labc: ce_label_col of the row; piece: the LOGICAL piece (columns col0 + 8 piece ..; storage position q holds piece q ^ swizzle).
// Padding blocks of the plane — columns at or beyond N, or beyond the groups the GEMM wrote statistics for — scale to zero: no
// statistic outside [0, ngroups) is ever read.
template <int GW>
__device__ __forceinline__ uint4 ce_rescale_piece(uint4 x, float2 rs, const float* __restrict__ strow, int ngroups, int N, int col0,
                                                  int labc, int piece) {
  const int gi = col0 / GW;
  const float mg = (gi < ngroups && col0 < N) ? strow[2 * gi] : -INFINITY;
  const float c = (mg == -INFINITY) ? 0.f : expf(mg - rs.x) * rs.y;
  const int lab = labc - col0 - piece * 8;                      // the label among this piece's eight columns, if 0 <= lab < 8
  unsigned w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    // two bf16 per dword: low half = even element
    float lo = __uint_as_float(w[e] << 16) * c, hi = __uint_as_float(w[e] & 0xffff0000u) * c;
    if (2 * e == lab) lo -= 1.f;
    if (2 * e + 1 == lab) hi -= 1.f;
    const __bf16 bl = (__bf16)lo, bh = (__bf16)hi;
    w[e] = (unsigned)__builtin_bit_cast(unsigned short, bl) | ((unsigned)__builtin_bit_cast(unsigned short, bh) << 16);
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// ---- anchored row work: one wave per row b of the scaled attout plane aps [., ap_cols] (KB32, inner 32 ap_in32) --------------------
// Rows [B, ceil32(B)) are k-rows of dE beyond the batch: their attout rows are ZERO (the plane's own padding rows hold finite
// leftovers of earlier batches — the epilogue's exponent is clamped —, and finite times zero is zero).  True: b was such a row or beyond.
__device__ __forceinline__ bool ce_anchor_pad_row(long b, int B, __bf16* __restrict__ aps, int ap_cols, int ap_in32, int lane) {
  if (b < B) return false;
  if (b < ((B + 31) & ~31))
    for (int c = lane * 4; c < ap_cols; c += 256) {
      ce_bf16x4 z;
#pragma unroll
      for (int j = 0; j < 4; ++j) z[j] = (__bf16)0.f;
      *reinterpret_cast<ce_bf16x4*>(aps + kb32_off(b, c, ap_in32)) = z;
    }
  return true;
}
// The tail of a live row (ce.hip: ANCHORED form) with S = s, the sum of its plane's rounded entries, and inv = 1 / s (0: a padding
// session — zero gradient row): patch the label's entry, scale2[b] = (inv, residual / S), aps[b, :] = bf16(attout[b, :] / S').
// lab == CE_NO_LABEL (the label lives in another shard's plane): no patch, no residual, plain inv on attout's row.
__device__ __forceinline__ void ce_anchor_row_tail(long b, int lab, float s, float inv, float* __restrict__ scale2,
                                                   __bf16* __restrict__ plane, int in32, const __bf16* __restrict__ ap_hi,
                                                   const __bf16* __restrict__ ap_lo, __bf16* __restrict__ aps, int ap_cols, int ap_in32,
                                                   int lane) {
  float inv_e = inv, resid = 0.f;
  if (lab != CE_NO_LABEL) {
    __bf16* q = plane + kb32_off(b, lab, in32);
    const float el = (float)*q;                   // (every lane: the same address, the same bits)
    const float t = el - s;
    const __bf16 v = (__bf16)t;
    inv_e = 1.0f / (el - (float)v);
    resid = (t - (float)v) * inv;
    if (lane == 0) *q = v;                        // (v depends on the wave's one load of the entry: it has returned for every lane)
  }
  if (lane == 0) { scale2[2 * b] = inv; scale2[2 * b + 1] = resid; }
  for (int c = lane * 4; c < ap_cols; c += 256) {
    const long o = kb32_off(b, c, ap_in32);
    const ce_bf16x4 h = *reinterpret_cast<const ce_bf16x4*>(ap_hi + o), l = *reinterpret_cast<const ce_bf16x4*>(ap_lo + o);
    ce_bf16x4 y;
#pragma unroll
    for (int j = 0; j < 4; ++j) y[j] = (__bf16)(inv_e * ((float)h[j] + (float)l[j]));
    *reinterpret_cast<ce_bf16x4*>(aps + o) = y;
  }
}
