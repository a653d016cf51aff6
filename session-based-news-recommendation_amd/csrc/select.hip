// Streamed selection (include/tcar_serve.h): the catalog's scores arrive in column panels; every panel is folded into a small running
// state per session — the k best (score, index) entries so far in list order, the count of scores strictly above the label's, and the
// online softmax pair (max, sum exp) — and one finishing launch turns the state into top-k / rank / cross entropy.  No [B, N] matrix.
//
// List order: score descending, then index descending (np.argsort(x)[::-1]; key_gt of topk_rows.h).  It is a TOTAL order
// over (score, item id), and a fold computes the exact k best of (state entries + panel columns) under it, so the list after the last
// panel is the k best of the catalog whatever the partition and whatever order candidates arrive in LDS.
#include "tcar_common.h"
#include "tcar_bf16_layout.h"
#include "topk_rows.h"
#include "panel_fold.h"
#include "../../include/tcar_serve_shard.h"

namespace {

// state row of one session (fold_row_words of panel_fold.h): score[k] | index[k] (-1: empty) | count, max, sum, pad
constexpr FoldTail SEL_TAIL = {{0u, 0xff800000u, 0u, 0u}};       // count 0, max -inf, sum 0

// the reset of every streamed fold: m empty entries (-inf, -1), then the selector's tail
__global__ __launch_bounds__(256) void fold_reset_kernel(int B, int m, FoldTail tail, uint32_t* __restrict__ state) {
  const int rw = fold_row_words(m);
  const long n = (long)B * rw;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int w = (int)(i % rw);
    state[i] = w < m ? 0xff800000u : w < 2 * m ? 0xffffffffu : tail.w[w - 2 * m];
  }
}

// One workgroup per session.  The row slice is read ONCE into registers; columns outside the slice and excluded items become NaN after
// the statistics: a NaN compares false with everything, so it is never a candidate.  The extraction is the core of topk_rows.h, which
// rank_topk_rows_kernel (score.hip) shares.
//
// W (include/tcar_window.h): item n0 + j is in the POOL of session b iff wlo[b] <= key[n0 + j] < whi[b], or it is the label of a
// labelled call.  Columns out of the pool do not exist: -inf in the statistics (no count, no max, exp = 0; a NaN would poison the
// sum), NaN among the candidates (a -inf would still beat the (-inf, -1) "nothing" key and enter a short list).  Which of its 4 R
// columns are in the pool a thread keeps as 4 R bits (`pool`), from ONE read of the key slice; the slice has no second copy.
//
// Q (include/tcar_quota.h): at most `cap` entries of one category in the list.  The statistics are the shared code above the
// extraction; only the extraction differs (the capped walk at the end of the kernel).  Q = false compiles none of it.
template <int R, bool W = false, bool Q = false>
__global__ __launch_bounds__(TOPK_NT) void select_panel_kernel(int n0, int n, const float* __restrict__ panel, long ld, int k,
                                                              const int32_t* __restrict__ label, const float* __restrict__ lab_score,
                                                              const int32_t* __restrict__ excl, int X, float* __restrict__ state,
                                                              const int32_t* __restrict__ key, const int32_t* __restrict__ wlo,
                                                              const int32_t* __restrict__ whi, const int32_t* __restrict__ cat,
                                                              int cap) {
  constexpr int NT = TOPK_NT, NWV = NT / 64;
  __shared__ TopkShared<NT> sh;
  __shared__ float shv[NWV];        // the statistics' per-wave partials: max, count, "any column in the pool", sum exp
  __shared__ int shc[NWV];
  __shared__ int shi[NWV];
  __shared__ float shs[NWV];
  __shared__ int any_excl;
  __shared__ unsigned exb[SEL_MAX_N / 32];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float* row = panel + (long)b * ld;
  float* st = state + (long)b * fold_row_words(k);
  int* sti = reinterpret_cast<int*>(st);
  const float ninf = -INFINITY, dead = __builtin_nanf("");
  unsigned pool[W ? (4 * R + 31) / 32 : 1] = {};      // W: bit 4 r + j = column (tid + r NT) 4 + j is in the pool
  if constexpr (W) {
    // The key slice key[n0 .. n0 + n), read once; no load leaves the slice
    const int32_t* kp = key + n0;
    const int lo = wlo[b], hi = whi[b];
    const int labc = lab_score ? label[b] - n0 : -1;          // a labelled call: the label's column is always in the pool
    auto bits4 = [&](int c, int4 q) __attribute__((always_inline)) -> unsigned {
      const unsigned lab = (unsigned)(c + 0 == labc) | (unsigned)(c + 1 == labc) << 1 | (unsigned)(c + 2 == labc) << 2 |
                           (unsigned)(c + 3 == labc) << 3;
      const unsigned cols = (unsigned)(c + 0 < n) | (unsigned)(c + 1 < n) << 1 | (unsigned)(c + 2 < n) << 2 | (unsigned)(c + 3 < n) << 3;
      return (window_bits4(lo, hi, q) | lab) & cols;
    };
    auto clamped = [&](bool tail) __attribute__((always_inline)) {       // every group, or the one partial group at the end alone
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int c = (tid + r * NT) * 4;
        if (!tail || (c < n && c + 3 >= n)) pool[(4 * r) >> 5] |= bits4(c, slice4(kp, c, n, false)) << ((4 * r) & 31);
      }
    };
    // Aligned: straight 16-byte loads of the whole groups, then the partial one.  (slice4 alone with `aligned` set compiles to four
    // 4-byte loads per group: the compiler folds its two arms into the clamped form.  All 4 R reads are in flight here.)
    if (!slice_aligned(kp)) clamped(false);
    else {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int c = (tid + r * NT) * 4;
        const int4 q = (c + 3 < n) ? *reinterpret_cast<const int4*>(kp + c) : make_int4(0, 0, 0, 0);
        pool[(4 * r) >> 5] |= (c + 3 < n ? bits4(c, q) : 0u) << ((4 * r) & 31);
      }
      if (n & 3) clamped(true);
    }
    __builtin_amdgcn_sched_barrier(0);               // the keys are bits before the slice takes its 4 R registers
  }
  // ---- load: the slice, this thread's entry of the running list, the running statistics
  float4 v[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int c = (tid + r * NT) * 4;
    v[r] = (c < n) ? ld4(row + c) : make_float4(ninf, ninf, ninf, ninf);     // (c + 3 < ld: ld % 4 == 0 and n <= ld)
  }
  float sv = dead;                  // state entry `tid` of the list (tid < k), NaN when empty
  int si = -1;
  if (tid < k) {
    si = sti[k + tid];
    if (si >= 0) sv = st[tid];
  }
  int sc = 0;                       // Q: the category of the state entry, re-read by index
  if constexpr (Q) {
    if (si >= 0) sc = cat[si];
  }
  const int old_cnt = sti[2 * k];
  const float old_m = st[2 * k + 1], old_s = st[2 * k + 2];
  const bool full = sti[2 * k - 1] >= 0;          // k entries so far: the last one bounds what can still enter
  const float lastv = st[k - 1];
  const int lasti = sti[2 * k - 1];
  // exclusion bitmap of this slice; any_excl: it has a bit set at all (read behind the statistics' barrier)
  const ExclBitmap ex{exb};
  ex.build<true>(excl, X, b, n0, n, tid, NT, &any_excl);
  // ---- statistics of the slice: strict-greater count (the label's own column left out by index), max, sum exp
  const bool counting = lab_score != nullptr;
  const float xl = counting ? lab_score[b] : 0.f;
  const int labc = counting ? label[b] - n0 : -1;
  int cnt = 0;
  float m = ninf;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int c = (tid + r * NT) * 4;
    if (c + 0 >= n) v[r].x = ninf;
    if (c + 1 >= n) v[r].y = ninf;
    if (c + 2 >= n) v[r].z = ninf;
    if (c + 3 >= n) v[r].w = ninf;
    if constexpr (W) {                    // out of the pool: -inf IN PLACE (the value is never needed again; the bits say which)
      const unsigned p = pool[(4 * r) >> 5] >> ((4 * r) & 31);
      if (!(p & 1u)) v[r].x = ninf;
      if (!(p & 2u)) v[r].y = ninf;
      if (!(p & 4u)) v[r].z = ninf;
      if (!(p & 8u)) v[r].w = ninf;
    }
    if (counting)
      cnt += (v[r].x > xl && c + 0 != labc) + (v[r].y > xl && c + 1 != labc) + (v[r].z > xl && c + 2 != labc) +
             (v[r].w > xl && c + 3 != labc);
    m = fmaxf(m, fmaxf(fmaxf(v[r].x, v[r].y), fmaxf(v[r].z, v[r].w)));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  m = wave_max(m);
  if (lane == 0) { shc[w] = cnt; shv[w] = m; }
  if constexpr (W) {
    unsigned any = 0u;
#pragma unroll
    for (int i = 0; i < (4 * R + 31) / 32; ++i) any |= pool[i];
    const bool wave_any = __any(any != 0u);
    if (lane == 0) shi[w] = wave_any;
  }
  __syncthreads();
  int tot = 0;
  float gm = old_m;
#pragma unroll
  for (int i = 0; i < NWV; ++i) { tot += shc[i]; gm = fmaxf(gm, shv[i]); }
  const int has_excl = any_excl;
  if constexpr (W) {
    // A slice wholly out of the pool folds nothing: count, max, sum and list stay the bits they are.  (With an empty state, old_m =
    // -inf, its maximum is -inf as well and exp(x - gm) would be exp(-inf + inf).)  Uniform over the workgroup.
    int pooled_waves = 0;
#pragma unroll
    for (int i = 0; i < NWV; ++i) pooled_waves += shi[i];
    if (!pooled_waves) return;
  }
  __syncthreads();
  {
    // online softmax: m' = max(m, slice max), s = s exp(m - m') + sum exp(x - m'); fixed order within a launch
    float se = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) se += (expf(v[r].x - gm) + expf(v[r].y - gm)) + (expf(v[r].z - gm) + expf(v[r].w - gm));
    se = wave_sum(se);
    if (lane == 0) shs[w] = se;
    __syncthreads();
    if (tid == 0) {
      float gs = 0.f;
#pragma unroll
      for (int i = 0; i < NWV; ++i) gs += shs[i];
      if (gm > ninf) {
        st[2 * k + 1] = gm;
        st[2 * k + 2] = (old_m > ninf ? old_s * expf(old_m - gm) : 0.f) + gs;
      }
      sti[2 * k] = old_cnt + tot;
    }
    __syncthreads();
  }
  // ---- from here on the registers hold CANDIDATES: padding columns, excluded items and (W) columns out of the pool die
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int c = (tid + r * NT) * 4;
    unsigned bits = 0u;
    if (has_excl && c < n) bits = ex.excl_bits4(c);
    if constexpr (W) bits |= ~(pool[(4 * r) >> 5] >> ((4 * r) & 31));
    if (c + 0 >= n || (bits & 1u)) v[r].x = dead;
    if (c + 1 >= n || (bits & 2u)) v[r].y = dead;
    if (c + 2 >= n || (bits & 4u)) v[r].z = dead;
    if (c + 3 >= n || (bits & 8u)) v[r].w = dead;
  }
  // ---- the k best of (columns + state entries) under the list order: the shared core (topk_rows.h).  A full list gives the threshold
  // for free (its last entry: the k entries themselves are at or above it), so a panel that cannot improve the list costs one compaction.
  TopkRows<NT, R> core{sh, v, sv, si, n0, tid, lastv, lasti};
  if constexpr (!Q) {
    core.topk(k, full, [&](int r, float fv, int fi) __attribute__((always_inline)) {
      if (tid == 0) { st[r] = fv; sti[k + r] = fi; }
    });
  } else {
    const int nc = core.candidates(k, full);
    // ---- the capped walk (include/tcar_quota.h): candidates in list order, one taken iff fewer than `cap` of its category are.
    // Lane j of EVERY wave keeps the category of list entry j (`mycat`), so "how many of category c are taken" is one ballot and the
    // decision is uniform over the workgroup.  When a category reaches the cap its remaining candidates can be KILLED, after which
    // every extracted best is acceptable: the number of block-wide rounds of a fold is bounded by k alone, never by n.
    //   stage 1: the candidates at or above L, from LDS (the core's phase C; the category is the payload of the arg-max)
    //   stage 2: when those run dry before k are taken (L only bounds the UNCAPPED k best) or do not fit the LDS: everything strictly
    //            below the last key walked, from the registers, one entry per round as in the core's fallback
    //            (kills there cost a pass over the category slice, so they are put off: see below)
    const int32_t* cp = cat + n0;
    const bool cal = slice_aligned(cp);
    int taken = 0, mycat = 0;
    auto accept = [&](float fv, int fi, int fc) __attribute__((always_inline)) -> bool {      // true: fc has reached the cap
      if (tid == 0) { st[taken] = fv; sti[k + taken] = fi; }
      if (lane == taken) mycat = fc;
      ++taken;
      return __popcll(__ballot(lane < taken && mycat == fc)) >= cap;
    };
    float pv = KEY_ALL_V;             // everything not walked yet is strictly below the key (pv, pi)
    int pi = KEY_ALL_I;
    if (nc <= core.CAP) {
      core.template extract_lds<true>(
          nc, k, [&](int i) __attribute__((always_inline)) { return cat[i]; },
          [&](int, float fv, int fi, int fc) __attribute__((always_inline)) -> int {
            if (fi < 0) return TOPK_STOP;
            return accept(fv, fi, fc) ? TOPK_KILL : TOPK_NEXT;
          });
      pv = core.lv; pi = core.li;     // what is left lies strictly below L; L = (-inf, -1): nothing is
    }
    if (taken < k && pi >= 0) {
      // columns (and the state entry) of category kc die; `hit`: the thread's current best was one of them
      bool hit = false;
      auto kill_pass = [&](int kc) __attribute__((always_inline)) {
        int t4 = tid * 4;
        asm volatile("" : "+v"(t4));       // the 4 R load addresses are computed HERE, pass by pass: hoisted out of the rounds' loop
                                           // they would be 2 R more live registers than the slice leaves
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int c = t4 + r * NT * 4;
          if (c < n) {
            const int4 q = slice4(cp, c, n, cal);
            if (q.x == kc) { v[r].x = dead; hit |= n0 + c + 0 == core.cbi; }
            if (q.y == kc) { v[r].y = dead; hit |= n0 + c + 1 == core.cbi; }
            if (q.z == kc) { v[r].z = dead; hit |= n0 + c + 2 == core.cbi; }
            if (q.w == kc) { v[r].w = dead; hit |= n0 + c + 3 == core.cbi; }
          }
          if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);     // four category loads in flight, not 4 R registers of them
        }
        if (si >= 0 && sc == kc) { hit |= si == core.cbi; sv = dead; si = -1; }
      };
      // A kill pass reads the whole category slice, so stage 2 starts LAZY: the categories that are full keep their columns, and an
      // extracted best of such a category is rejected (one wasted round; its owner rescans).  Typically a handful of entries are
      // missing and the next bests are acceptable.  After k rejected rounds the fold stops being lazy: every full category is killed,
      // one pass each (at most k / cap of them, now and later), and from then on every extracted best is acceptable again.  So
      // stage 2 spends at most k accepting and k + 1 rejecting rounds whatever the slice holds.
      core.scan(pv, pi);
      bool lazy = true;
      int rejected = 0;
      while (taken < k) {
        float fv; int fi;
        core.best(core.cbv, core.cbi, fv, fi);
        if (fi < 0) break;
        const int fc = cat[__builtin_amdgcn_readfirstlane(fi)];
        hit = core.cbi == fi;
        int j0 = 0, j1 = 0;                     // list entries whose category is to be killed now, if it is full
        bool one = false;
        if (lazy && __popcll(__ballot(lane < taken && mycat == fc)) >= cap) {
          if (++rejected > k) { lazy = false; j1 = taken; }         // every full category, each once (at its first list entry)
        } else {
          const bool sat = accept(fv, fi, fc);
          if (taken == k) break;
          if (sat && !lazy) { j0 = taken - 1; j1 = taken; one = true; }        // the one that has just become full
        }
        for (int j = j0; j < j1; ++j) {
          const int cj = __shfl(mycat, j);
          const bool same = mycat == cj;
          if ((one || __ballot(lane < j && same) == 0) && __popcll(__ballot(lane < taken && same)) >= cap) kill_pass(cj);
        }
        if (hit) core.scan(fv, fi);
      }
    }
    if (tid >= taken && tid < k) { st[tid] = ninf; sti[k + tid] = -1; }
  }
}

__global__ __launch_bounds__(64) void select_finish_kernel(int k, const float* __restrict__ state, const float* __restrict__ lab_score,
                                                           int32_t* __restrict__ topk, float* __restrict__ score,
                                                           int32_t* __restrict__ rank, float* __restrict__ ce) {
  const int b = blockIdx.x, t = threadIdx.x;
  const float* st = state + (long)b * fold_row_words(k);
  const int* sti = reinterpret_cast<const int*>(st);
  if (t < k) {
    const int i = sti[k + t];
    if (topk) topk[(long)b * k + t] = i;
    if (score && i >= 0) score[(long)b * k + t] = st[t];
  }
  if (t == 0) {
    if (rank) rank[b] = 1 + sti[2 * k];
    if (ce) ce[b] = st[2 * k + 1] + logf(st[2 * k + 2]) - lab_score[b];
  }
}

// Merge of S select states into one (include/tcar_serve_shard.h).  ONE wave per session: lane s walks the list of shard s — every
// input list is already in list order, so the merged list is an S-way merge.  A round takes the wave-wide best of the S heads (shuffles
// only: no LDS, no barrier) and its owner moves on; Q (include/tcar_quota.h): a head whose category already holds `cap` entries of the
// merged list is rejected and only moves its owner on, which is the capped walk over the S k entries.  Every round advances one cursor,
// so a merge ends after at most S k rounds (k where nothing is rejected).  A lane keeps its head AND the entry behind it in registers:
// the load that refills them is in flight during the next round's arg-max.  Lane j keeps entry j of the merged list (and, Q, its
// category: "how many of this category are taken" is one ballot), written once at the end.  Scores are copied.
// Statistics: counts add; (max, sum exp) pairs combine in ascending shard order — a fixed rounding order — and a pair with max = -inf
// (a state that never folded a pooled column) is left out, so no exp(-inf + inf) is ever formed.
template <bool Q>
__global__ __launch_bounds__(64) void select_merge_kernel(int k, int S, const float* __restrict__ states, long stride,
                                                          float* __restrict__ out, const int32_t* __restrict__ cat, int cap) {
  const int b = blockIdx.x, lane = threadIdx.x, rw = fold_row_words(k);
  const float ninf = -INFINITY;
  const bool live = lane < S;
  const float* st = states + (live ? (long)lane * stride : 0L) + (long)b * rw;       // (lanes >= S point at shard 0 and read nothing)
  const int* sti = reinterpret_cast<const int*>(st);
  int cnt = live ? sti[2 * k] : 0;
  const float ms = live ? st[2 * k + 1] : ninf;
  const float ss = live ? st[2 * k + 2] : 0.f;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  const float M = wave_max(ms);
  const float part = ms > ninf ? ss * expf(ms - M) : 0.f;
  float sum = 0.f;
  for (int s = 0; s < S; ++s) sum += __shfl(part, s);
  // entry j of this lane's list; (-inf, -1): the list has ended
  auto entry = [&](int j, float& v, int& i) __attribute__((always_inline)) {
    v = ninf; i = -1;
    if (live && j < k) {
      i = sti[k + j];
      if (i >= 0) v = st[j];
    }
  };
  float hv, nv, ov = ninf;
  int hi, ni, oi = -1, cur = 0, taken = 0, mycat = 0;
  entry(0, hv, hi);
  entry(1, nv, ni);
  while (taken < k) {
    // wave-wide arg-max of the heads in list order; equal keys (the same item in two lists) go to the lower lane
    float bv = hv;
    int bi = hi, bl = lane;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float xv = __shfl_xor(bv, o);
      const int xi = __shfl_xor(bi, o), xl = __shfl_xor(bl, o);
      if (key_gt(xv, xi, bv, bi) || (xv == bv && xi == bi && xl < bl)) { bv = xv; bi = xi; bl = xl; }
    }
    if (bi < 0) break;                      // every list has ended
    bool ok = true;
    int fc = 0;
    if constexpr (Q) {
      fc = cat[__builtin_amdgcn_readfirstlane(bi)];
      ok = __popcll(__ballot(lane < taken && mycat == fc)) < cap;
    }
    if (ok) {
      if (lane == taken) { ov = bv; oi = bi; mycat = fc; }
      ++taken;
    }
    if (lane == bl) {
      hv = nv; hi = ni;
      ++cur;
      entry(cur + 1, nv, ni);
    }
  }
  float* o = out + (long)b * rw;
  int* oint = reinterpret_cast<int*>(o);
  if (lane < k) { o[lane] = ov; oint[k + lane] = oi; }
  if (lane == 0) { oint[2 * k] = cnt; o[2 * k + 1] = M; o[2 * k + 2] = sum; o[2 * k + 3] = 0.f; }
}

// lab_score[b] = attout[b] . E[label[b]] over K columns, from the operands the panel GEMM contracts: one wave per session
__global__ __launch_bounds__(64) void label_score_f32_kernel(int N, int K, const float* __restrict__ att, long ld_att,
                                                             const float* __restrict__ E, long ldE, const int32_t* __restrict__ label,
                                                             float* __restrict__ out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int lab = clampi(label[b], 0, N - 1);
  const float* a = att + (long)b * ld_att;
  const float* e = E + (long)lab * ldE;
  float s = 0.f;
  for (int c = lane * 4; c < K; c += 256) s += dot4(ld4(a + c), ld4(e + c));
  s = wave_sum(s);
  if (lane == 0) out[b] = s;
}
__global__ __launch_bounds__(64) void label_score_bf16_kernel(int N, int K, const __bf16* __restrict__ a_hi, const __bf16* __restrict__ a_lo,
                                                              int a_in32, const __bf16* __restrict__ e_hi,
                                                              const __bf16* __restrict__ e_lo, int e_in32, int nsplit,
                                                              const int32_t* __restrict__ label, float* __restrict__ out, int lab0,
                                                              int owned_only) {
  const int b = blockIdx.x, lane = threadIdx.x;
  // owned_only (a catalog shard whose planes hold the rows [lab0, lab0 + N)): a label outside them — another shard's, or the -1 of a
  // padding session — reads no row and scores 0
  int lab = label[b] - lab0;
  if (owned_only && (lab < 0 || lab >= N)) {
    if (lane == 0) out[b] = 0.f;
    return;
  }
  lab = clampi(lab, 0, N - 1);
  float s = 0.f;
  for (int c = lane; c < K; c += 64) {
    const long oa = kb32_off(b, c, a_in32), oe = kb32_off(lab, c, e_in32);
    const float ah = (float)a_hi[oa], eh = (float)e_hi[oe];
    float p = ah * eh;
    if (nsplit == 3) p += ah * (float)e_lo[oe] + (float)a_lo[oa] * eh;       // the three products of the split-bf16 GEMM
    s += p;
  }
  s = wave_sum(s);
  if (lane == 0) out[b] = s;
}

// a cap goes with a category table (then >= 1), and with nothing else
inline bool bad_quota(const int32_t* cat, int cap) { return cat ? cap < 1 : cap != 0; }
// the (B, k) every entry point of the streamed selection takes
inline bool bad_bk(int B, int k) { return bad_fold_bm(B, k, SEL_MAX_K); }

}  // namespace

extern "C" int tcar_serve_abi_version(void) { return TCAR_SERVE_ABI_VERSION; }

extern "C" int64_t tcar_select_state_bytes(int B, int k) {
  if (bad_bk(B, k)) return -1;
  return (int64_t)B * fold_row_words(k) * 4;
}

int tcar_fold_reset(int B, int m, int m_max, FoldTail tail, void* state, void* stream) {
  if (bad_fold_bm(B, m, m_max)) return TCAR_E_ARG;
  if (B == 0) return TCAR_OK;
  if (!state || ((uintptr_t)state & 3)) return TCAR_E_ARG;
  long blocks = ((long)B * fold_row_words(m) + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  TCAR_LAUNCH(fold_reset_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, B, m, tail, (uint32_t*)state);
  TCAR_CHECK_LAUNCH();
  return TCAR_OK;
}

extern "C" int tcar_select_reset(int B, int k, void* state, void* stream) { return tcar_fold_reset(B, k, SEL_MAX_K, SEL_TAIL, state, stream); }

extern "C" int tcar_window_abi_version(void) { return TCAR_WINDOW_ABI_VERSION; }
extern "C" int tcar_quota_abi_version(void) { return TCAR_QUOTA_ABI_VERSION; }

// one fold; key == NULL: the unwindowed kernels; cat == NULL or cap >= k (no list of k entries can break such a cap): the uncapped ones
extern "C" int tcar_select_panel_quota(int B, int n0, int n, const float* panel, int64_t ld, int k, const int32_t* label,
                                       const float* lab_score, const int32_t* excl, int X, void* state, void* stream,
                                       const int32_t* key, const int32_t* lo, const int32_t* hi, const int32_t* cat, int cap) {
  if (bad_quota(cat, cap)) return TCAR_E_ARG;
  if (lab_score && !label) return TCAR_E_ARG;
  bool empty;
  if (const int rc = check_fold_args(B, k, SEL_MAX_K, n0, n, panel, ld, excl, X, key, lo, hi, state, &empty); rc != TCAR_OK || empty)
    return rc;
  // the kernel: [rung of the R ladder that holds n columns][windowed][capped]
  static constexpr decltype(&select_panel_kernel<2>) fold[3][2][2] = {
      {{select_panel_kernel<TOPK_R_SMALL, false, false>, select_panel_kernel<TOPK_R_SMALL, false, true>},
       {select_panel_kernel<TOPK_R_SMALL, true, false>, select_panel_kernel<TOPK_R_SMALL, true, true>}},
      {{select_panel_kernel<TOPK_R_MID, false, false>, select_panel_kernel<TOPK_R_MID, false, true>},
       {select_panel_kernel<TOPK_R_MID, true, false>, select_panel_kernel<TOPK_R_MID, true, true>}},
      {{select_panel_kernel<TOPK_R_WIDE, false, false>, select_panel_kernel<TOPK_R_WIDE, false, true>},
       {select_panel_kernel<TOPK_R_WIDE, true, false>, select_panel_kernel<TOPK_R_WIDE, true, true>}}};
  const int rung = n <= topk_cols(TOPK_R_SMALL) ? 0 : n <= topk_cols(TOPK_R_MID) ? 1 : 2;
  const bool capped = cat && cap < k;
  TCAR_LAUNCH(fold[rung][key != nullptr][capped], dim3(B), dim3(TOPK_NT), 0, (hipStream_t)stream, n0, n, panel, (long)ld, k, label,
              lab_score, excl, X, (float*)state, key, lo, hi, cat, cap);
  TCAR_CHECK_LAUNCH();
  return TCAR_OK;
}

extern "C" int tcar_select_panel_window(int B, int n0, int n, const float* panel, int64_t ld, int k, const int32_t* label,
                                        const float* lab_score, const int32_t* excl, int X, void* state, void* stream,
                                        const int32_t* key, const int32_t* lo, const int32_t* hi) {
  return tcar_select_panel_quota(B, n0, n, panel, ld, k, label, lab_score, excl, X, state, stream, key, lo, hi, nullptr, 0);
}

extern "C" int tcar_select_panel(int B, int n0, int n, const float* panel, int64_t ld, int k, const int32_t* label,
                                 const float* lab_score, const int32_t* excl, int X, void* state, void* stream) {
  return tcar_select_panel_window(B, n0, n, panel, ld, k, label, lab_score, excl, X, state, stream, nullptr, nullptr, nullptr);
}

extern "C" int tcar_select_finish(int B, int k, const void* state, const float* lab_score, int32_t* topk, float* score, int32_t* rank,
                                  float* ce, void* stream) {
  if (bad_bk(B, k) || (ce && !lab_score)) return TCAR_E_ARG;
  if (B == 0) return TCAR_OK;
  if (!state || !topk) return TCAR_E_ARG;
  TCAR_LAUNCH(select_finish_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, k, (const float*)state, lab_score, topk, score, rank, ce);
  TCAR_CHECK_LAUNCH();
  return TCAR_OK;
}

extern "C" int tcar_serve_shard_abi_version(void) { return TCAR_SERVE_SHARD_ABI_VERSION; }

extern "C" int tcar_select_merge(int B, int k, int S, const void* states, int64_t stride_words, void* out, const int32_t* cat, int cap,
                                 void* stream) {
  if (bad_quota(cat, cap)) return TCAR_E_ARG;
  if (bad_bk(B, k) || S < 1 || S > 64) return TCAR_E_ARG;
  const int64_t rows = (int64_t)B * fold_row_words(k);
  if (S > 1 && stride_words < rows) return TCAR_E_ARG;
  if (B == 0) return TCAR_OK;
  if (!states || !out || ((uintptr_t)states & 3) || ((uintptr_t)out & 3)) return TCAR_E_ARG;
  const uintptr_t in0 = (uintptr_t)states, in1 = in0 + (uintptr_t)(((int64_t)(S - 1) * stride_words + rows) * 4);
  const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)(rows * 4);
  if (o0 < in1 && in0 < o1) return TCAR_E_ARG;            // out overlaps the inputs
  hipStream_t s = (hipStream_t)stream;
  if (cat && cap < k)
    TCAR_LAUNCH((select_merge_kernel<true>), dim3(B), dim3(64), 0, s, k, S, (const float*)states, (long)stride_words, (float*)out, cat, cap);
  else
    TCAR_LAUNCH((select_merge_kernel<false>), dim3(B), dim3(64), 0, s, k, S, (const float*)states, (long)stride_words, (float*)out, cat,
                cap);
  TCAR_CHECK_LAUNCH();
  return TCAR_OK;
}

// planes: hi / lo KB32 of attout [ceil128(B), a_inner] and of E [ceil128(N), e_inner] (nsplit 1: hi only); NULL a_hi: fp32 operands
int tcar_label_scores(int B, int N, int K, const float* att, int64_t ld_att, const float* E, int64_t ldE, const void* a_hi,
                      const void* a_lo, int64_t a_inner, const void* e_hi, const void* e_lo, int64_t e_inner, int nsplit,
                      const int32_t* label, float* out, void* stream) {
  return tcar_label_scores_owned(B, N, K, att, ld_att, E, ldE, a_hi, a_lo, a_inner, e_hi, e_lo, e_inner, nsplit, label, out, 0, 0, stream);
}

// owned_only != 0 (bf16 planes only): the e planes hold the catalog rows [lab0, lab0 + N) of a shard; out[b] = 0 for a label outside
int tcar_label_scores_owned(int B, int N, int K, const float* att, int64_t ld_att, const float* E, int64_t ldE, const void* a_hi,
                            const void* a_lo, int64_t a_inner, const void* e_hi, const void* e_lo, int64_t e_inner, int nsplit,
                            const int32_t* label, float* out, int lab0, int owned_only, void* stream) {
  if (B <= 0) return TCAR_OK;
  if (owned_only && !a_hi) return TCAR_E_ARG;
  if (N <= 0 || K <= 0 || !label || !out) return TCAR_E_ARG;
  if (a_hi) {
    if (!e_hi || (nsplit == 3 && (!a_lo || !e_lo)) || (nsplit != 1 && nsplit != 3) || (a_inner & 31) || (e_inner & 31) ||
        a_inner < K || e_inner < K)
      return TCAR_E_ARG;
    TCAR_LAUNCH(label_score_bf16_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, N, K, (const __bf16*)a_hi, (const __bf16*)a_lo,
                (int)(a_inner >> 5), (const __bf16*)e_hi, (const __bf16*)e_lo, (int)(e_inner >> 5), nsplit, label, out, lab0, owned_only);
  } else {
    if (!att || !E || (K & 3) || (ld_att & 3) || (ldE & 3) || !tcar_aligned16(att) || !tcar_aligned16(E)) return TCAR_E_ARG;
    TCAR_LAUNCH(label_score_f32_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, N, K, att, (long)ld_att, E, (long)ldE, label, out);
  }
  TCAR_CHECK_LAUNCH();
  return TCAR_OK;
}
