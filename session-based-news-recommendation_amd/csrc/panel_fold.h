// The vocabulary of a streamed panel fold: what select_panel_kernel (select.hip) and retrieve_panel_kernel (retrieve.hip) share.
// Both fold a column panel [n0, n0 + n) of scores into a per-session state row, and which columns a session may be offered at all —
// not in its exclusion list, inside its window lo <= key < hi — they decide HERE, once.  The kernels keep their own loops.
#pragma once
#include "tcar_common.h"

// ---- the state row of one session, 2 m + 4 words: score[m] | id[m] (-1: empty) | four tail words that belong to the selector
__host__ __device__ inline int fold_row_words(int m) { return 2 * m + 4; }
struct FoldTail { uint32_t w[4]; };      // the tail of a state that has folded nothing
inline bool bad_fold_bm(int B, int m, int m_max) { return B < 0 || m < 1 || m > m_max; }
// select.hip: every row of `state` to the empty list and `tail`; behind tcar_select_reset and tcar_retrieve_reset
int tcar_fold_reset(int B, int m, int m_max, FoldTail tail, void* state, void* stream);

// The argument checks of one fold, m list entries of at most m_max: TCAR_E_ARG, or TCAR_OK with *empty = "nothing to fold" (no
// session or no column: decided before the pointers are looked at).  Launches nothing.
inline int check_fold_args(int B, int m, int m_max, int n0, int n, const float* panel, int64_t ld, const int32_t* excl, int X,
                           const int32_t* key, const int32_t* lo, const int32_t* hi, const void* state, bool* empty) {
  *empty = B == 0 || n == 0;
  if ((key ? (!lo || !hi) : (lo || hi)) || bad_fold_bm(B, m, m_max) || n0 < 0 || n < 0 || n > SEL_MAX_N) return TCAR_E_ARG;
  if ((long)n0 + n > 0x7fffffffL || (ld & 3) || ld < n || X < 0 || (excl && X <= 0)) return TCAR_E_ARG;
  return *empty || (panel && state && tcar_aligned16(panel) && !((uintptr_t)state & 3)) ? TCAR_OK : TCAR_E_ARG;
}

// ---- exclusion bitmap of the slice in LDS: bit c is set iff item n0 + c is in excl[b, :] (integer LDS atomics; idempotent: repeats,
// -1 slots and ids outside the slice name nothing; untouched where excl == NULL).  build() holds the barrier between the zeroing and
// the scatter; the one in front of the first excl_bits4() is the caller's.  ANY: the LDS flag *any says "a bit was set at all".
struct ExclBitmap {
  unsigned (&exb)[SEL_MAX_N / 32];
  template <bool ANY = false>
  __device__ __forceinline__ void build(const int32_t* __restrict__ excl, int X, int b, int n0, int n, int tid, int NT,
                                        int* any = nullptr) const {
    if (ANY && tid == 0) *any = 0;
    for (int i = tid; excl && i < (n + 31) / 32; i += NT) exb[i] = 0u;
    __syncthreads();
    for (int i = tid; excl && i < X; i += NT) {
      const int e = excl[(long)b * X + i] - n0;
      if (e >= 0 && e < n) atomicOr(&exb[e >> 5], 1u << (e & 31));
      if (ANY && e >= 0 && e < n) *any = 1;
    }
  }
  // bits 0 .. 3: the columns c .. c + 3 are excluded (c % 4 == 0: the four bits sit in one word; c < n)
  __device__ __forceinline__ unsigned excl_bits4(int c) const { return exb[c >> 5] >> (c & 31); }
};

// ---- p[c .. c + 3] of a slice p[0 .. n), n >= 1, c % 4 == 0: one 16-byte load where the slice is 16-byte aligned and the group is
// whole, else four scalar loads clamped into the slice (no branch; the caller masks what lies at or past n).  No load leaves [0, n).
__device__ __forceinline__ bool slice_aligned(const int32_t* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
__device__ __forceinline__ int4 slice4(const int32_t* __restrict__ p, int c, int n, bool aligned) {
  if (aligned && c + 3 < n) return *reinterpret_cast<const int4*>(p + c);
  return make_int4(p[min(c, n - 1)], p[min(c + 1, n - 1)], p[min(c + 2, n - 1)], p[min(c + 3, n - 1)]);
}

// ---- bit j: key j of q is inside the window lo <= key < hi (include/tcar_window.h)
__device__ __forceinline__ unsigned window_bits4(int lo, int hi, int4 q) {
  return (unsigned)((lo <= q.x) & (q.x < hi)) | (unsigned)((lo <= q.y) & (q.y < hi)) << 1 | (unsigned)((lo <= q.z) & (q.z < hi)) << 2 |
         (unsigned)((lo <= q.w) & (q.w < hi)) << 3;
}

// ---- the sortable key of a list entry: what the admitting selectors (retrieve.hip, sections.hip) keep in LDS
typedef unsigned long long rt_key_t;

// (score, id) -> a 64-bit key whose UNSIGNED order is the list order.  High word: the score's bits made monotone (negative: all bits
// flipped, else the sign bit set), with -0.0 folded onto +0.0 first — the two compare equal, so the id must decide between them.  Low
// word: id << 1 (ids are >= 0) with the folded sign of a zero in bit 0, so that rt_score gives back the score's own bits.  Every real
// key is > 0 (the smallest high word, -inf's, is 0x007fffff): 0 is "nothing", the padding of the sort and the threshold of a list
// that is not full.  NaN never gets here.
__device__ __forceinline__ rt_key_t rt_key(float v, int id) {
  unsigned u = __float_as_uint(v);
  const unsigned nz = u == 0x80000000u;
  if (nz) u = 0u;
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((rt_key_t)u << 32) | (rt_key_t)(((unsigned)id << 1) | nz);
}
__device__ __forceinline__ int rt_id(rt_key_t k) { return (int)((unsigned)k >> 1); }
__device__ __forceinline__ float rt_score(rt_key_t k) {
  const unsigned u = (unsigned)(k >> 32);
  if ((unsigned)k & 1u) return -0.f;
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// ---- the section codes of a sectioned fold (include/tcar_sections.h): 1 .. 16 of them, pairwise distinct, in host memory
constexpr int SEC_MAX_G = 16;
inline bool bad_sections(int G, const int32_t* sections) {
  if (G < 1 || G > SEC_MAX_G || !sections) return true;
  for (int i = 1; i < G; ++i)
    for (int j = 0; j < i; ++j)
      if (sections[i] == sections[j]) return true;
  return false;
}
