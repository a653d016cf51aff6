// Streamed top-C selection, 1 <= C <= 1024 (include/tcar_retrieve.h): the first stage of retrieve-then-rank.  The catalog's scores
// arrive in column panels; every panel is folded into a per-session state of the C best (score, item) entries so far, and a finishing
// launch copies the state out as a shortlist.  The row-resident selector of select.hip extracts k entries in k block-wide arg-max
// rounds, which ends at k = 64; this one ADMITS what beats a threshold into an LDS buffer and sorts the buffer now and then.
//
// List order: key_gt of topk_rows.h — score descending, then item id descending; -0.0 == +0.0.  A (score, id) pair is packed into ONE
// sortable 64-bit key (rt_key) whose unsigned order IS the list order, so admission is one compare and the sort moves one word.  The
// order is total over the items and a prune keeps the exact C best of what the buffer holds, so by induction the state after any
// sequence of folds is the C best of everything folded so far: the same bits for every partition into panels and whatever order the
// admitted elements landed in the buffer (the LDS counter decides positions, the sort forgets them).
#include "tcar_common.h"
#include "topk_rows.h"
#include "panel_fold.h"
#include "../../include/tcar_retrieve_shard.h"

namespace {

constexpr int RT_MAX_C = CAND_MAX_C;           // a shortlist is a candidate list of cand.hip
constexpr int RT_NT = 512, RT_NWV = RT_NT / 64;
constexpr int RT_U = 4;                        // float4 per thread and sweep: a sweep is RT_NT * 4 * RT_U = 8,192 columns
constexpr int RT_SWEEP = RT_NT * 4 * RT_U;
constexpr int RT_MIN_CAP = 256;                // the buffer of a small C: 2 Cp entries would prune every few admissions
constexpr int RT_MAX_CAP = 2 * RT_MAX_C;       // 2,048 keys: 16 KB

// state row (fold_row_words of panel_fold.h): score[C] | id[C] (-1: empty) | held, threshold key (low, high word), pad; reset: zeros
__host__ __device__ inline int rt_cap(int C) {
  int p = 1;
  while (p < C) p <<= 1;
  return 2 * p < RT_MIN_CAP ? RT_MIN_CAP : 2 * p;
}

// One workgroup per session.  LDS: the key buffer (cap = max(2 Cp, 256) entries used, Cp = C rounded up to a power of two) and the
// exclusion bitmap of the slice.  The buffer starts as the state's entries; the row slice streams by in sweeps of 8,192 columns
// (16-byte loads, the next sweep's in flight while this one is tested); an element is admitted iff it is eligible and its key beats
// the threshold `thr`; admitted elements are appended at an LDS counter (one atomic per wave).  When an append does not fit, the
// buffer is PRUNED — bitonic sort, descending; the best C stay; thr = the C-th key once C are held — and the elements that did not
// fit are tested against the new threshold and tried again: a prune frees at least cap - C >= cap / 2 places, so this ends.  At the
// end of the panel one more prune, and the state goes back in list order.  A panel that admitted nothing writes nothing.
//
// Bounds: a buffer index is < cap <= RT_MAX_CAP by the `pos < cap` test of the append and the loops of the prune; the bitmap index is
// < (n + 31) / 32 <= SEL_MAX_N / 32 by the 0 <= e < n test; row loads are guarded by c < n (c % 4 == 0, ld % 4 == 0, n <= ld); key
// loads are clamped into [0, n).  live: NULL, or one word per session — live[b] < 0: the session is padding, its workgroup returns
// before it reads anything else (uniform: ahead of every barrier) and its state stays as it was.
template <bool W>
__global__ __launch_bounds__(RT_NT) void retrieve_panel_kernel(int n0, int n, const float* __restrict__ panel, long ld, int C,
                                                               const int32_t* __restrict__ excl, int X, float* __restrict__ state,
                                                               const int32_t* __restrict__ key, const int32_t* __restrict__ wlo,
                                                               const int32_t* __restrict__ whi, const int32_t* __restrict__ live) {
  __shared__ rt_key_t buf[RT_MAX_CAP];
  __shared__ unsigned exb[SEL_MAX_N / 32];
  __shared__ int cnt;               // entries in the buffer + elements that asked for a place
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  if (live && live[b] < 0) return;
  const int cap = rt_cap(C);
  const float* row = panel + (long)b * ld;
  float* st = state + (long)b * fold_row_words(C);
  int* sti = reinterpret_cast<int*>(st);
  int held = sti[2 * C];            // uniform: entries of the buffer that are settled (after a prune: all of them)
  rt_key_t thr = ((rt_key_t)(unsigned)sti[2 * C + 2] << 32) | (unsigned)sti[2 * C + 1];
  for (int i = tid; i < held; i += RT_NT) buf[i] = rt_key(st[i], sti[C + i]);
  if (tid == 0) cnt = held;
  const ExclBitmap ex{exb};
  ex.build(excl, X, b, n0, n, tid, RT_NT);
  int wl = 0, wh = 0;
  if constexpr (W) { wl = wlo[b]; wh = whi[b]; }
  const int32_t* kp = W ? key + n0 : nullptr;
  const bool kal = W && slice_aligned(kp);
  __syncthreads();

  // the buffer's first `m` entries -> the best min(m, C) of them in list order; returns how many.  Uniform control flow.
  auto prune = [&](int m) __attribute__((always_inline)) -> int {
    int M = 2;
    while (M < m) M <<= 1;                                   // (m <= cap, and cap is a power of two: M <= cap)
    for (int i = m + tid; i < M; i += RT_NT) buf[i] = 0ull;
    __syncthreads();
    for (int k = 2; k <= M; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = tid; t < (M >> 1); t += RT_NT) {
          const int i = 2 * t - (t & (j - 1)), l = i + j;    // the pair (i, i + j), bit j of i clear
          const rt_key_t x = buf[i], y = buf[l];
          const bool desc = (i & k) == 0;                    // this run sorts descending (the last stage: all of them)
          if (desc ? x < y : x > y) { buf[i] = y; buf[l] = x; }
        }
        __syncthreads();
      }
    }
    const int keep = m < C ? m : C;
    if (keep == C) thr = buf[C - 1];
    return keep;
  };

  bool dirty = false;
  float4 v[RT_U], nv[RT_U];
  auto load = [&](int base, float4 (&d)[RT_U]) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < RT_U; ++u) {
      const int c = base + (tid + u * RT_NT) * 4;
      d[u] = c < n ? ld4(row + c) : zero4();
    }
  };
  load(0, nv);
  for (int base = 0; base < n; base += RT_SWEEP) {
#pragma unroll
    for (int u = 0; u < RT_U; ++u) v[u] = nv[u];
    if (base + RT_SWEEP < n) load(base + RT_SWEEP, nv);
    // bit 4 u + j of `pend`: column base + (tid + u NT) 4 + j is eligible and beats the threshold
    auto key_of = [&](int e) __attribute__((always_inline)) -> rt_key_t {
      const int u = e >> 2, j = e & 3;
      const float x = j == 0 ? v[u].x : j == 1 ? v[u].y : j == 2 ? v[u].z : v[u].w;
      return rt_key(x, n0 + base + (tid + u * RT_NT) * 4 + j);
    };
    unsigned pend = 0u;
#pragma unroll
    for (int u = 0; u < RT_U; ++u) {
      const int c = base + (tid + u * RT_NT) * 4;
      if (c >= n) continue;
      unsigned ok = (unsigned)(v[u].x == v[u].x) | (unsigned)(v[u].y == v[u].y) << 1 | (unsigned)(v[u].z == v[u].z) << 2 |
                    (unsigned)(v[u].w == v[u].w) << 3;                               // not NaN
      ok &= (c + 3 < n) ? 15u : (1u << (n - c)) - 1u;
      if (excl) ok &= ~ex.excl_bits4(c);
      if constexpr (W) ok &= window_bits4(wl, wh, slice4(kp, c, n, kal));
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if ((ok >> j & 1u) && key_of(4 * u + j) > thr) pend |= 1u << (4 * u + j);
    }
    for (;;) {
      // ---- append: one LDS atomic per wave; lane l's elements take the places behind those of the lanes below it
      const int mine = __popc(pend);
      if (__any(mine != 0)) {
        int incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const int t = __shfl_up(incl, o);
          if (lane >= o) incl += t;
        }
        int wbase = 0;
        if (lane == 63) wbase = atomicAdd(&cnt, incl);
        wbase = __shfl(wbase, 63);
        int pos = wbase + incl - mine;
#pragma unroll
        for (int e = 0; e < 4 * RT_U; ++e) {
          if (pend >> e & 1u) {
            if (pos < cap) { buf[pos] = key_of(e); pend &= ~(1u << e); }
            ++pos;
          }
        }
      }
      __syncthreads();
      const int total = cnt;        // what the buffer was asked to hold: beyond cap, elements are still pending
      __syncthreads();              // (everyone has read cnt before the next append or the reset below touches it)
      if (total != held) dirty = true;
      if (total <= cap) { held = total; break; }
      held = prune(cap);
      if (tid == 0) cnt = held;
#pragma unroll
      for (int e = 0; e < 4 * RT_U; ++e)
        if ((pend >> e & 1u) && !(key_of(e) > thr)) pend &= ~(1u << e);
      __syncthreads();
    }
  }
  if (!dirty) return;               // uniform: nothing was admitted, state and threshold are what they were
  held = prune(held);
  for (int i = tid; i < C; i += RT_NT) {
    const bool in = i < held;
    const rt_key_t k = in ? buf[i] : 0ull;
    st[i] = in ? rt_score(k) : -INFINITY;
    sti[C + i] = in ? rt_id(k) : -1;
  }
  if (tid == 0) {
    sti[2 * C] = held;
    sti[2 * C + 1] = (int)(unsigned)thr;
    sti[2 * C + 2] = (int)(unsigned)(thr >> 32);
  }
}

__global__ __launch_bounds__(256) void retrieve_finish_kernel(int C, const float* __restrict__ state, int32_t* __restrict__ ids,
                                                              float* __restrict__ scores) {
  const int b = blockIdx.x;
  const float* st = state + (long)b * fold_row_words(C);
  const int* sti = reinterpret_cast<const int*>(st);
  for (int i = threadIdx.x; i < C; i += 256) {
    const int id = sti[C + i];
    ids[(long)b * C + i] = id;
    if (scores) scores[(long)b * C + i] = id >= 0 ? st[i] : -INFINITY;
  }
}

// topk[b, j] = ids[b, order[b, j]] for the first k ranks of a list (tcar_cand_rank's `order`), -1 / untouched behind its end
__global__ __launch_bounds__(64) void rerank_take_kernel(int C, int k, const int32_t* __restrict__ ids, const float* __restrict__ cand_score,
                                                         const int32_t* __restrict__ order, int32_t* __restrict__ topk,
                                                         float* __restrict__ score) {
  const int b = blockIdx.x, j = threadIdx.x;
  if (j >= k) return;
  const int s = order[(long)b * C + j];
  const bool in = s >= 0 && s < C;
  topk[(long)b * k + j] = in ? ids[(long)b * C + s] : -1;
  if (score && in) score[(long)b * k + j] = cand_score[(long)b * C + s];
}

// S states of one session -> one (include/tcar_retrieve_shard.h).  One workgroup per session.  Every input list is already in list
// order, so a shard is taken in by ONE bitonic merge step, not a sort: the running best sits in buf[0, Cp) descending, zero-padded at
// the end (Cp = C rounded up to a power of two; 0 = "nothing" sorts below every key); shard s's entries go REVERSED into buf[Cp, 2 Cp),
// zero-padded at the front — descending then ascending is a bitonic sequence —, the log2(2 Cp) compare-exchange stages leave
// buf[0, 2 Cp) descending, and what lies past the first C is dropped.  11 stages per shard at C = 1,024 against 66 of a full sort.
// A shard that holds nothing is skipped, and so is one whose best key does not beat the C-th key once C entries are held (its list
// is descending: nothing of it can enter); both tests read one word every thread sees alike, so control flow stays uniform.  The
// items of the shards are disjoint, so all keys differ and the result does not depend on the order of the shards.
//
// Bounds: a buffer index is < 2 Cp <= RT_MAX_CAP (the loops run over [0, Cp) and the pair (i, i + j) of stage j has i + j < 2 Cp);
// of an input row the words [0, hs), [C, C + hs) and 2 C are read with hs clamped into [0, C]; the row of (s, b) starts at
// s * stride + b * (2 C + 4) words, inside what the host checked; the output row takes its 2 C + 4 words and nothing else.
__global__ __launch_bounds__(RT_NT) void retrieve_merge_kernel(int C, int S, const float* __restrict__ states, long stride,
                                                               float* __restrict__ out) {
  __shared__ rt_key_t buf[RT_MAX_CAP];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int rw = fold_row_words(C);
  int Cp = 1;
  while (Cp < C) Cp <<= 1;
  for (int i = tid; i < Cp; i += RT_NT) buf[i] = 0ull;
  __syncthreads();
  int held = 0;                     // uniform: entries of buf[0, Cp) that are real
  for (int s = 0; s < S; ++s) {
    const float* st = states + (long)s * stride + (long)b * rw;
    const int* sti = reinterpret_cast<const int*>(st);
    int hs = sti[2 * C];
    hs = hs < 0 ? 0 : hs > C ? C : hs;
    if (hs == 0) continue;
    if (held == C && !(rt_key(st[0], sti[C]) > buf[C - 1])) continue;
    for (int i = tid; i < Cp; i += RT_NT) {
      const int j = Cp - 1 - i;     // entry j of the shard's list lands at Cp + i
      buf[Cp + i] = j < hs ? rt_key(st[j], sti[C + j]) : 0ull;
    }
    __syncthreads();
    for (int j = Cp; j > 0; j >>= 1) {
      for (int t = tid; t < Cp; t += RT_NT) {
        const int i = 2 * t - (t & (j - 1)), l = i + j;
        const rt_key_t x = buf[i], y = buf[l];
        if (x < y) { buf[i] = y; buf[l] = x; }
      }
      __syncthreads();
    }
    held = held + hs < C ? held + hs : C;
    for (int i = C + tid; i < Cp; i += RT_NT) buf[i] = 0ull;      // (keep the first C: the zero padding of the next step)
    __syncthreads();
  }
  float* o = out + (long)b * rw;
  int* oi = reinterpret_cast<int*>(o);
  for (int i = tid; i < C; i += RT_NT) {
    const bool in = i < held;
    const rt_key_t k = in ? buf[i] : 0ull;
    o[i] = in ? rt_score(k) : -INFINITY;
    oi[C + i] = in ? rt_id(k) : -1;
  }
  if (tid == 0) {
    const rt_key_t thr = held == C ? buf[C - 1] : 0ull;
    oi[2 * C] = held;
    oi[2 * C + 1] = (int)(unsigned)thr;
    oi[2 * C + 2] = (int)(unsigned)(thr >> 32);
    oi[2 * C + 3] = 0;
  }
}

inline bool bad_bc(int B, int C) { return bad_fold_bm(B, C, RT_MAX_C); }

}  // namespace

extern "C" int tcar_retrieve_abi_version(void) { return TCAR_RETRIEVE_ABI_VERSION; }

extern "C" int64_t tcar_retrieve_state_bytes(int B, int C) {
  if (bad_bc(B, C)) return -1;
  return (int64_t)B * fold_row_words(C) * 4;
}

extern "C" int tcar_retrieve_reset(int B, int C, void* state, void* stream) {
  return tcar_fold_reset(B, C, RT_MAX_C, FoldTail{}, state, stream);
}

extern "C" int tcar_retrieve_panel_live(int B, int n0, int n, const float* panel, int64_t ld, int C, const int32_t* excl, int X,
                                        const int32_t* key, const int32_t* lo, const int32_t* hi, void* state, const int32_t* live,
                                        void* stream) {
  bool empty;
  if (const int rc = check_fold_args(B, C, RT_MAX_C, n0, n, panel, ld, excl, X, key, lo, hi, state, &empty); rc != TCAR_OK || empty)
    return rc;
  TCAR_LAUNCH((key ? retrieve_panel_kernel<true> : retrieve_panel_kernel<false>), dim3(B), dim3(RT_NT), 0, (hipStream_t)stream, n0, n,
              panel, (long)ld, C, excl, X, (float*)state, key, lo, hi, live);
  TCAR_CHECK_LAUNCH();
  return TCAR_OK;
}

extern "C" int tcar_retrieve_panel(int B, int n0, int n, const float* panel, int64_t ld, int C, const int32_t* excl, int X,
                                   const int32_t* key, const int32_t* lo, const int32_t* hi, void* state, void* stream) {
  return tcar_retrieve_panel_live(B, n0, n, panel, ld, C, excl, X, key, lo, hi, state, nullptr, stream);
}

extern "C" int tcar_retrieve_finish(int B, int C, const void* state, int32_t* ids, float* scores, void* stream) {
  if (bad_bc(B, C)) return TCAR_E_ARG;
  if (B == 0) return TCAR_OK;
  if (!state || !ids || ((uintptr_t)state & 3)) return TCAR_E_ARG;
  TCAR_LAUNCH(retrieve_finish_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, C, (const float*)state, ids, scores);
  TCAR_CHECK_LAUNCH();
  return TCAR_OK;
}

extern "C" int tcar_retrieve_shard_abi_version(void) { return TCAR_RETRIEVE_SHARD_ABI_VERSION; }

extern "C" int tcar_retrieve_merge(int B, int C, int S, const void* states, int64_t stride_words, void* out, void* stream) {
  if (bad_bc(B, C) || S < 1 || S > 64) return TCAR_E_ARG;
  const int64_t rows = (int64_t)B * fold_row_words(C);
  if (S > 1 && stride_words < rows) return TCAR_E_ARG;
  if (B == 0) return TCAR_OK;
  if (!states || !out || ((uintptr_t)states & 3) || ((uintptr_t)out & 3)) return TCAR_E_ARG;
  const uintptr_t in0 = (uintptr_t)states, in1 = in0 + (uintptr_t)(((int64_t)(S - 1) * stride_words + rows) * 4);
  const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)(rows * 4);
  if (o0 < in1 && in0 < o1) return TCAR_E_ARG;            // out overlaps the inputs
  TCAR_LAUNCH(retrieve_merge_kernel, dim3(B), dim3(RT_NT), 0, (hipStream_t)stream, C, S, (const float*)states, (long)stride_words,
              (float*)out);
  TCAR_CHECK_LAUNCH();
  return TCAR_OK;
}

// the closing launch of tcar_retrieve_rerank_step (step.hip) and of the sharded two-stage call (include/tcar_retrieve_shard.h)
extern "C" int tcar_rerank_take(int B, int C, int k, const int32_t* ids, const float* cand_score, const int32_t* order, int32_t* topk, float* score,
                     void* stream) {
  if (B <= 0) return TCAR_OK;
  if (k < 1 || k > SEL_MAX_K || k > C || !ids || !cand_score || !order || !topk) return TCAR_E_ARG;
  TCAR_LAUNCH(rerank_take_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, C, k, ids, cand_score, order, topk, score);
  TCAR_CHECK_LAUNCH();
  return TCAR_OK;
}
