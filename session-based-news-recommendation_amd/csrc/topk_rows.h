// Row-resident exact top-k: the one device implementation behind rank_topk_rows_kernel (score.hip) and select_panel_kernel
// (select.hip), and the one definition of the LIST ORDER every selector of the library follows.
//
// A workgroup of NT threads holds a slice of one row in registers: thread `tid` keeps float4 v[R], where v[r].{x,y,z,w} are the columns
// (tid + r NT) 4 + {0,1,2,3} of the slice and column c is item n0 + c.  On top of the slice a thread may hold ONE extra entry (sv, si)
// — the fold's entry of the running list.  A candidate that must not be picked is NaN: a NaN compares false with everything, so it
// never passes a key comparison (padding columns, excluded items, columns out of a window, an empty extra entry).
//
// topk(k, ...) extracts the k best candidates in list order and hands each to a sink as (round, value, index); when the candidates
// run out the remaining rounds deliver the "nothing" key (-inf, -1).  k is a run-time int with no upper bound here.
//   phase A  threshold(): L = the k-th largest of the per-thread bests.  At least k candidates are at or above L, so the k best are.
//   phase B  compact():   the candidates at or above L go to LDS (integer counter; the order they land in does not matter).
//   phase C  extract_lds(): at most CAP = 2 NT of them: k block-wide arg-max rounds over <= 2 LDS candidates per thread.
//   fallback extract_regs(): more than CAP (the largest values sit in the columns of fewer than k threads; L is exact in the index,
//            so ties alone never overflow): one entry per round from the registers; only the owner of the extracted entry rescans.
#pragma once
#include "tcar_common.h"

// ---- list order: score descending, then item id descending (np.argsort(x)[::-1]).  Item ids are unique, so it is a TOTAL order.
__device__ __forceinline__ bool key_gt(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai > bi); }
constexpr float KEY_NONE_V = -__builtin_inff();      // "nothing": below every real key (ids are >= 0, so (-inf, i) still beats it)
constexpr int KEY_NONE_I = -1;
constexpr float KEY_ALL_V = __builtin_inff();        // above every key: "strictly below it" is everything
constexpr int KEY_ALL_I = 0x7fffffff;

// what a sink of extract_lds answers: go on; stop (the entry was not taken); go on and drop every LDS candidate with this entry's payload
enum { TOPK_NEXT = 0, TOPK_STOP = 1, TOPK_KILL = 2 };

template <int NT>
struct TopkShared {
  float candv[2 * NT];      // phase B (first: a candidate's LDS address is then its position alone)
  int candi[2 * NT];
  int ncand;
  float bv[NT / 64];        // block arg-max: one key per wave
  int bi[NT / 64];
  int bp[NT / 64];          // ... and its payload (touched by the payload form only)
};

template <int NT, int R>
struct TopkRows {
  static constexpr int NWV = NT / 64, CAP = 2 * NT;
  TopkShared<NT>& sh;
  float4 (&v)[R];           // the slice (the caller may kill more candidates between calls)
  float& sv;                // the extra entry: (NaN, -1) when there is none
  int& si;
  const int n0, tid;
  float lv = KEY_NONE_V;    // threshold L
  int li = KEY_NONE_I;
  float cbv = KEY_NONE_V;   // the thread's best candidate strictly below the key of the last scan()
  int cbi = KEY_NONE_I;

  __device__ __forceinline__ void scan(float pv, int pi) {
    cbv = KEY_NONE_V; cbi = KEY_NONE_I;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int c = n0 + (tid + r * NT) * 4;
      const float e[4] = {v[r].x, v[r].y, v[r].z, v[r].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = c + j;
        if (key_gt(pv, pi, e[j], i) && key_gt(e[j], i, cbv, cbi)) { cbv = e[j]; cbi = i; }
      }
    }
    if (key_gt(pv, pi, sv, si) && key_gt(sv, si, cbv, cbi)) { cbv = sv; cbi = si; }
  }

  // block-wide arg-max of one key per thread (KEY_NONE: the thread has nothing); P: a payload travels with the key.  Result to every
  // thread.  Two barriers; uniform control flow required.
  template <bool P>
  __device__ __forceinline__ void best(float bv, int bi, int bp, float& fv, int& fi, int& fp) const {
    const int lane = tid & 63, w = tid >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o);
      const int oi = __shfl_xor(bi, o);
      int op = 0;
      if constexpr (P) op = __shfl_xor(bp, o);
      if (key_gt(ov, oi, bv, bi)) { bv = ov; bi = oi; bp = op; }
    }
    if (lane == 0) {
      sh.bv[w] = bv; sh.bi[w] = bi;
      if constexpr (P) sh.bp[w] = bp;
    }
    __syncthreads();
    fv = sh.bv[0]; fi = sh.bi[0];
    if constexpr (P) fp = sh.bp[0];
#pragma unroll
    for (int j = 1; j < NWV; ++j)
      if (key_gt(sh.bv[j], sh.bi[j], fv, fi)) {
        fv = sh.bv[j]; fi = sh.bi[j];
        if constexpr (P) fp = sh.bp[j];
      }
    __syncthreads();
  }
  __device__ __forceinline__ void best(float bv, int bi, float& fv, int& fi) const {
    int fp = 0;
    best<false>(bv, bi, 0, fv, fi, fp);
  }

  // phase A.  Fewer than k threads hold anything: L = nothing, every candidate qualifies.
  __device__ __forceinline__ void threshold(int k) {
    scan(KEY_ALL_V, KEY_ALL_I);
    float av = cbv;
    int ai = cbi;
    lv = KEY_NONE_V; li = KEY_NONE_I;
    for (int r = 0; r < k; ++r) {
      float fv; int fi;
      best(av, ai, fv, fi);
      if (fi < 0) { lv = KEY_NONE_V; li = KEY_NONE_I; break; }
      lv = fv; li = fi;
      if (ai == fi) { av = KEY_NONE_V; ai = KEY_NONE_I; }
    }
  }

  // phase B: returns the number of candidates at or above L; the first CAP of them are in LDS
  __device__ __forceinline__ int compact() const {
    if (tid == 0) sh.ncand = 0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int c = n0 + (tid + r * NT) * 4;
      const float e[4] = {v[r].x, v[r].y, v[r].z, v[r].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = c + j;
        if (e[j] > lv || (e[j] == lv && i >= li)) {
          const int pos = atomicAdd(&sh.ncand, 1);
          if (pos < CAP) { sh.candv[pos] = e[j]; sh.candi[pos] = i; }
        }
      }
    }
    if (sv > lv || (sv == lv && si >= li)) {
      const int pos = atomicAdd(&sh.ncand, 1);
      if (pos < CAP) { sh.candv[pos] = sv; sh.candi[pos] = si; }
    }
    __syncthreads();
    const int nc = sh.ncand;
    __syncthreads();
    return nc;
  }

  // phases A + B.  bounded: the caller's (lv, li) already has at least k candidates at or above it (a full running list: its last
  // entry); phase A then runs only when too many candidates pass it.
  __device__ __forceinline__ int candidates(int k, bool bounded) {
    if (!bounded) threshold(k);
    int nc = compact();
    if (nc > CAP && bounded) {
      threshold(k);
      nc = compact();
    }
    return nc;
  }

  // phase C (nc <= CAP).  P: pay(index) is the payload of a candidate, loaded once, and the sink is sink(round, value, index, payload)
  // -> TOPK_*; else sink(round, value, index) and all k rounds run.  Returns the number of rounds the sink did not stop.
  template <bool P, class Pay, class Sink>
  __device__ __forceinline__ int extract_lds(int nc, int k, Pay pay, Sink sink) const {
    float c0v = tid < nc ? sh.candv[tid] : KEY_NONE_V, c1v = tid + NT < nc ? sh.candv[tid + NT] : KEY_NONE_V;
    int c0i = tid < nc ? sh.candi[tid] : KEY_NONE_I, c1i = tid + NT < nc ? sh.candi[tid + NT] : KEY_NONE_I;
    int c0p = 0, c1p = 0;
    if constexpr (P) {
      if (c0i >= 0) c0p = pay(c0i);
      if (c1i >= 0) c1p = pay(c1i);
    }
    int r = 0, fi = 0;
    for (; r < k; ++r) {
      const bool first = key_gt(c0v, c0i, c1v, c1i);
      float fv = KEY_NONE_V;
      int fp = 0, act = TOPK_NEXT;
      if (fi >= 0) best<P>(first ? c0v : c1v, first ? c0i : c1i, first ? c0p : c1p, fv, fi, fp);      // (dry: the rest is "nothing")
      if constexpr (P) act = sink(r, fv, fi, fp);
      else sink(r, fv, fi);
      if (act == TOPK_STOP) break;
      if (c0i == fi || (act == TOPK_KILL && c0p == fp)) { c0v = KEY_NONE_V; c0i = KEY_NONE_I; }
      if (c1i == fi || (act == TOPK_KILL && c1p == fp)) { c1v = KEY_NONE_V; c1i = KEY_NONE_I; }
    }
    return r;
  }

  // fallback: k rounds straight from the registers.  (Reached only with more than CAP candidates at or above a threshold of phase A,
  // whose scan left every thread's best in (cbv, cbi).)  Once a round finds nothing the rest of the list is "nothing": no more arg-max.
  template <class Sink>
  __device__ __forceinline__ void extract_regs(int k, Sink sink) {
    int fi = 0;
    for (int r = 0; r < k; ++r) {
      float fv = KEY_NONE_V;
      if (fi >= 0) best(cbv, cbi, fv, fi);
      sink(r, fv, fi);
      if (fi >= 0 && cbi == fi) scan(fv, fi);
    }
  }

  // the k best of the candidates, in list order, to sink(round, value, index); k <= 0 extracts nothing
  template <class Sink>
  __device__ __forceinline__ void topk(int k, bool bounded, Sink sink) {
    if (k <= 0) return;
    const int nc = candidates(k, bounded);
    if (nc <= CAP) extract_lds<false>(nc, k, 0, sink);
    else extract_regs(k, sink);
  }
};
