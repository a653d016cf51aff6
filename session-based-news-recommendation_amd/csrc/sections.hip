// Sectioned streamed selection (include/tcar_sections.h): G lists per session, one per category code, from ONE pass over a panel.
// The state is B G rows of the select state of select.hip (row b G + g: score[k] | id[k] | four tail words this fold never
// touches), so tcar_select_reset / tcar_select_finish / tcar_select_merge serve it unchanged.  The selector is retrieve.hip's — ADMIT
// what beats a threshold into an LDS buffer, sort the buffer now and then — segmented by section: a buffer, a counter and a
// threshold per section, and a column goes to the section whose code its category equals, or nowhere.
//
// List order: key_gt of topk_rows.h as ONE sortable 64-bit key (rt_key of panel_fold.h).  The order is total over the items, the
// sections are disjoint (distinct codes), and a prune keeps the exact k best of what a section's buffer holds, so by induction a state
// row after any sequence of folds is the k best of its section over everything folded so far: the same bits for every partition into
// panels, every panel order and whatever place an admitted element took in its buffer (the LDS counter decides places, the sort
// forgets them).  No float is ever added.
#include "tcar_common.h"
#include "topk_rows.h"
#include "panel_fold.h"
#include "../../include/tcar_sections.h"

namespace {

constexpr int SC_NT = 512, SC_NWV = SC_NT / 64;
constexpr int SC_U = 4;                        // float4 per thread and sweep: a sweep is SC_NT * 4 * SC_U = 8,192 columns
constexpr int SC_SWEEP = SC_NT * 4 * SC_U;
constexpr int SC_CAP = 128;                    // keys of one section's buffer: 2 x 64, the k state entries plus admissions
static_assert(SC_CAP >= 2 * SEL_MAX_K && SC_CAP == 128, "a prune sorts 128 keys, two per lane, and frees at least half of them");
static_assert(SEC_MAX_G == TCAR_MAX_SECTIONS && SEC_MAX_G <= 16, "a column's section is a 4-bit number");

struct SecCodes { int32_t code[SEC_MAX_G]; };  // the section codes, by value in the launch arguments

__device__ __forceinline__ rt_key_t shfl_xor_key(rt_key_t x, int j) {
  const unsigned lo = __shfl_xor((unsigned)x, j), hi = __shfl_xor((unsigned)(x >> 32), j);
  return ((rt_key_t)hi << 32) | lo;
}

// 128 keys of ONE wave, element i in lane i & 63 (x0: i < 64, x1: i >= 64) -> descending.  A bitonic network on shuffles: no LDS, no
// barrier.  Stage (k, j) pairs element i with i ^ j; the run of element i sorts descending iff (i & k) == 0 (k = 128: every run).
__device__ __forceinline__ void sort128(rt_key_t& x0, rt_key_t& x1, int lane) {
#pragma unroll
  for (int k = 2; k <= 128; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (j == 64) {                           // (k = 128) the pair sits in one lane
        const rt_key_t a = x0 > x1 ? x0 : x1, c = x0 > x1 ? x1 : x0;
        x0 = a; x1 = c;
      } else {
        const bool low = (lane & j) == 0;                                // this lane holds the pair's lower element
        const bool d0 = k == 128 || (lane & k) == 0;                     // element lane      (k = 64: bit 6 of it is clear)
        const bool d1 = k == 128 || (k < 64 && (lane & k) == 0);         // element lane + 64 (k = 64: bit 6 of it is set)
        const rt_key_t y0 = shfl_xor_key(x0, j), y1 = shfl_xor_key(x1, j);
        x0 = (low == d0) == (x0 > y0) ? x0 : y0;                         // the lower element of a descending pair keeps the maximum
        x1 = (low == d1) == (x1 > y1) ? x1 : y1;
      }
    }
  }
}

// One workgroup per session, one launch per panel.  LDS: G key buffers of SC_CAP entries (16 KB at G = 16), per section a counter
// `cnt` (entries in the buffer + elements that asked for a place) and a threshold `thr` (the k-th key once k are held, 0 = "nothing"
// before), and the exclusion bitmap of the slice (6 KB).  Wave w loads the state rows of the sections w, w + 8 into their buffers.
// The row slice streams by in sweeps of 8,192 columns (16-byte loads, the next sweep's in flight while this one is tested) beside the
// category slice cat[n0 .. n0 + n); a column's section is the g with cat == code[g] (G compares per column, the codes in scalar
// registers), an element is admitted iff it is eligible, has a section and its key beats that section's threshold, and an admitted
// element takes a place at its section's counter (one LDS atomic).  A section whose counter passed SC_CAP is PRUNED by one wave —
// sort128, the best k stay, thr = the k-th — up to eight sections at once, and the elements that found no place are tested against
// the raised threshold and try again: a prune frees SC_CAP - k >= 64 places, so this ends.  At the end of the panel every section
// that admitted anything is pruned once more and written back in list order; a section that admitted nothing writes nothing.
//
// Bounds: a buffer index is g * SC_CAP + pos with g < G <= 16 (a 4-bit field that is only ever set from the loop over g < G) and
// 0 <= pos < SC_CAP by the append's test, or the prune's lane / lane + 64 < SC_CAP; cnt and thr are indexed by such a g or by
// lane < G; the bitmap index is < (n + 31) / 32 <= SEL_MAX_N / 32 by the 0 <= e < n test; row loads are guarded by c < n (c % 4 ==
// 0, ld % 4 == 0, n <= ld); cat and key loads are clamped into their slices [0, n) (slice4); a state row is (b G + g) (2 k + 4)
// words into `state`, of which the words [0, 2 k) are read and written, lane < k.
template <bool W>
__global__ __launch_bounds__(SC_NT) void section_panel_kernel(int n0, int n, const float* __restrict__ panel, long ld, int k, int G,
                                                              SecCodes codes, const int32_t* __restrict__ cat,
                                                              const int32_t* __restrict__ excl, int X, float* __restrict__ state,
                                                              const int32_t* __restrict__ key, const int32_t* __restrict__ wlo,
                                                              const int32_t* __restrict__ whi) {
  __shared__ rt_key_t buf[SEC_MAX_G * SC_CAP];
  __shared__ rt_key_t thr[SEC_MAX_G];
  __shared__ int cnt[SEC_MAX_G];
  __shared__ unsigned exb[SEL_MAX_N / 32];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float* row = panel + (long)b * ld;
  const int rw = fold_row_words(k);
  float* st0 = state + (long)b * G * rw;
  // ---- the state rows -> the buffers (an entry is real iff its id is >= 0; the real ones are packed to the front).  The threshold of
  // a full row is its LAST entry: a row is in list order, because between a reset (all empty) and a finish only this fold's closing
  // prune writes it.  (A row tcar_select_merge wrote is in list order too, but a merged state is finished, not folded into again.)
  for (int g = w; g < G; g += SC_NWV) {
    const float* st = st0 + (long)g * rw;
    const int* sti = reinterpret_cast<const int*>(st);
    const int id = lane < k ? sti[k + lane] : -1;
    const bool real = id >= 0;
    const unsigned long long have = __ballot(real);
    const int held = __popcll(have), pos = __popcll(have & ((1ull << lane) - 1ull));
    const rt_key_t kk = real ? rt_key(st[lane], id) : 0ull;
    if (real) buf[g * SC_CAP + pos] = kk;
    if (held == k && lane == k - 1) thr[g] = kk;                       // (k entries: every lane < k is real, lane k - 1 the last)
    if (held < k && lane == 0) thr[g] = 0ull;
    if (lane == 0) cnt[g] = held;
  }
  const ExclBitmap ex{exb};
  ex.build(excl, X, b, n0, n, tid, SC_NT);
  int wl = 0, wh = 0;
  if constexpr (W) { wl = wlo[b]; wh = whi[b]; }
  const int32_t* kp = W ? key + n0 : nullptr;
  const bool kal = W && slice_aligned(kp);
  const int32_t* cp = cat + n0;
  const bool cal = slice_aligned(cp);
  __syncthreads();
  const int held0 = lane < G ? cnt[lane] : 0;      // section `lane` as the state had it
  unsigned dirty = 0u;                              // uniform: bit g = section g has admitted something

  // section g's buffer -> the best min(m, k) of its first m = min(cnt, SC_CAP) entries in list order.  One wave; uniform in it.
  // last: the entries go to the state row (and -inf / -1 behind them); else: back to the buffer, with the counter and the threshold.
  auto prune = [&](int g, bool last) __attribute__((always_inline)) {
    rt_key_t* bg = buf + g * SC_CAP;
    const int have = cnt[g], m = have < SC_CAP ? have : SC_CAP;
    rt_key_t x0 = lane < m ? bg[lane] : 0ull, x1 = lane + 64 < m ? bg[lane + 64] : 0ull;
    sort128(x0, x1, lane);
    const int keep = m < k ? m : k;               // (k <= 64: what stays is in x0)
    if (!last) {
      if (lane < keep) bg[lane] = x0;
      if (keep == k && lane == k - 1) thr[g] = x0;
      if (lane == 0) cnt[g] = keep;
    } else if (lane < k) {
      float* st = st0 + (long)g * rw;
      const bool in = lane < keep;
      st[lane] = in ? rt_score(x0) : -INFINITY;
      reinterpret_cast<int*>(st)[k + lane] = in ? rt_id(x0) : -1;
    }
  };
  // the sections of `mask`, dealt to the waves in turn: wave w takes the w-th, the (w + 8)-th, ... set bit
  auto prune_all = [&](unsigned mask, bool last) __attribute__((always_inline)) {
    for (int turn = 0; mask; mask &= mask - 1u, ++turn)
      if ((turn & (SC_NWV - 1)) == w) prune(__ffs(mask) - 1, last);
  };

  float4 v[SC_U], nv[SC_U];
  auto load = [&](int base, float4 (&d)[SC_U]) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < SC_U; ++u) {
      const int c = base + (tid + u * SC_NT) * 4;
      d[u] = c < n ? ld4(row + c) : zero4();
    }
  };
  load(0, nv);
  for (int base = 0; base < n; base += SC_SWEEP) {
#pragma unroll
    for (int u = 0; u < SC_U; ++u) v[u] = nv[u];
    if (base + SC_SWEEP < n) load(base + SC_SWEEP, nv);
    auto key_of = [&](int e) __attribute__((always_inline)) -> rt_key_t {
      const int u = e >> 2, j = e & 3;
      const float x = j == 0 ? v[u].x : j == 1 ? v[u].y : j == 2 ? v[u].z : v[u].w;
      return rt_key(x, n0 + base + (tid + u * SC_NT) * 4 + j);
    };
    // bit 4 u + j of `pend`: column base + (tid + u NT) 4 + j is eligible, has a section and beats its threshold; its section is the
    // 4-bit field 4 u + j of `sec`
    unsigned pend = 0u;
    unsigned long long sec = 0ull;
#pragma unroll
    for (int u = 0; u < SC_U; ++u) {
      const int c = base + (tid + u * SC_NT) * 4;
      if (c >= n) continue;
      unsigned ok = (unsigned)(v[u].x == v[u].x) | (unsigned)(v[u].y == v[u].y) << 1 | (unsigned)(v[u].z == v[u].z) << 2 |
                    (unsigned)(v[u].w == v[u].w) << 3;                               // not NaN
      ok &= (c + 3 < n) ? 15u : (1u << (n - c)) - 1u;
      if (excl) ok &= ~ex.excl_bits4(c);
      if constexpr (W) ok &= window_bits4(wl, wh, slice4(kp, c, n, kal));
      const int4 q = slice4(cp, c, n, cal);
      int sx = -1, sy = -1, sz = -1, sw = -1;
#pragma unroll
      for (int g = 0; g < SEC_MAX_G; ++g) {
        if (g < G) {                              // (uniform; the unrolled g indexes the launch arguments with a constant)
          const int code = codes.code[g];
          sx = q.x == code ? g : sx;
          sy = q.y == code ? g : sy;
          sz = q.z == code ? g : sz;
          sw = q.w == code ? g : sw;
        }
      }
      ok &= (unsigned)(sx >= 0) | (unsigned)(sy >= 0) << 1 | (unsigned)(sz >= 0) << 2 | (unsigned)(sw >= 0) << 3;
      const unsigned s4 = (unsigned)(sx & 15) | (unsigned)(sy & 15) << 4 | (unsigned)(sz & 15) << 8 | (unsigned)(sw & 15) << 12;
      sec |= (unsigned long long)s4 << (16 * u);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int g = (int)(s4 >> (4 * j)) & 15;
        if ((ok >> j & 1u) && key_of(4 * u + j) > thr[g]) pend |= 1u << (4 * u + j);      // (ok: g < G)
      }
    }
    for (;;) {
      // ---- append: an element takes the next place of its section's buffer, or stays pending where the buffer is full
#pragma unroll
      for (int e = 0; e < 4 * SC_U; ++e) {
        if (pend >> e & 1u) {
          const int g = (int)(sec >> (4 * e)) & 15;
          const int pos = atomicAdd(&cnt[g], 1);
          if (pos < SC_CAP) { buf[g * SC_CAP + pos] = key_of(e); pend &= ~(1u << e); }
        }
      }
      __syncthreads();
      const int have = lane < G ? cnt[lane] : 0;   // what buffer `lane` was asked to hold: beyond SC_CAP, elements are still pending
      __syncthreads();                             // (everyone has read cnt before the next append or a prune touches it)
      dirty |= (unsigned)__ballot(lane < G && have != held0);
      const unsigned over = (unsigned)__ballot(have > SC_CAP);     // the same word in every wave
      if (!over) break;
      prune_all(over, false);
      __syncthreads();
#pragma unroll
      for (int e = 0; e < 4 * SC_U; ++e)
        if ((pend >> e & 1u) && !(key_of(e) > thr[(int)(sec >> (4 * e)) & 15])) pend &= ~(1u << e);
    }
  }
  // (the sweep's last barrier stands between the appends and these reads; each touched section belongs to one wave from here on)
  prune_all(dirty, true);
}

}  // namespace

extern "C" int tcar_sections_abi_version(void) { return TCAR_SECTIONS_ABI_VERSION; }

extern "C" int tcar_section_panel(int B, int n0, int n, const float* panel, int64_t ld, int k, int G, const int32_t* sections,
                                  const int32_t* cat, const int32_t* excl, int X, const int32_t* key, const int32_t* lo,
                                  const int32_t* hi, void* state, void* stream) {
  if (bad_sections(G, sections) || !cat) return TCAR_E_ARG;
  bool empty;
  if (const int rc = check_fold_args(B, k, SEL_MAX_K, n0, n, panel, ld, excl, X, key, lo, hi, state, &empty); rc != TCAR_OK || empty)
    return rc;
  SecCodes codes{};
  for (int g = 0; g < G; ++g) codes.code[g] = sections[g];
  TCAR_LAUNCH((key ? section_panel_kernel<true> : section_panel_kernel<false>), dim3(B), dim3(SC_NT), 0, (hipStream_t)stream, n0, n,
              panel, (long)ld, k, G, codes, cat, excl, X, (float*)state, key, lo, hi);
  TCAR_CHECK_LAUNCH();
  return TCAR_OK;
}
