// Diversity re-ranking (include/tcar_mmr.h): the greedy MMR walk over a session's shortlist.  One launch, one workgroup per session.
//
// Layout.  The pool holds at most 256 slots and a content row at most 1,000 bytes of fp32: 256 rows do not fit the LDS, they do fit
// the register file.  TWO adjacent lanes own one pool slot; a row is cut into CHUNKS of four columns and lane half h holds the chunks
// 2 i + h (the columns 8 i + 4 h .. + 3) — interleaved, so that the two halves read neighbouring 16-byte LDS slots, never one bank.
// The rows are gathered ONCE from the table; a round then
//   1. reduces the sortable key of csrc/panel_fold.h, extended by the slot, over the workgroup (xor butterfly, one LDS word pair per
//      wave, every thread folds the wave results itself);
//   2. the two lanes of the pick copy its row into a 1 KB LDS buffer and write the outputs;
//   3. every remaining slot dots its registers with the LDS row (each wave reads two addresses per instruction: a broadcast), the two
//      halves are added with one cross-lane move, and m_c = max(m_c, sim).
// Two barriers per round; nothing but LDS is read in the rounds.  A workgroup has 2 * min(C, 256) threads (rounded up to a wave), a
// wave whose slots lie past the pool computes no dot, and a session with an empty pool writes its -1s and leaves.
//
// Summation order of one dot (fixed by H alone, tcar_mmr.h): per half four fma chains, chain q over the columns 8 i + 4 h + q in
// ascending i, (c0 + c1) + (c2 + c3), then half 0 + half 1 (commutative: both lanes hold the same bits).  Chunks past H contribute
// fma(0, 0, acc) = acc.  NC is the chunks per lane of the register form (H <= 8 NC); NC == 0 is the form for any H, which keeps
// nothing and re-reads both rows from the table in every round — same order, no register budget.
// Row arithmetic is written on scalars: the library carries no packed fp32 math (DESIGN.md §7 observation 1).
#include "tcar_common.h"
#include "panel_fold.h"
#include "../../include/tcar_mmr.h"
#include <math.h>

namespace {

constexpr int MM_POOL = TCAR_MMR_MAX_POOL;
constexpr int MM_NT = 2 * MM_POOL, MM_NWV = MM_NT / 64;
constexpr int MM_NC = 32;                    // chunks per lane of the widest register form: H <= 256
static_assert(MM_POOL == 256, "the pool position travels in the low 8 bits of the key's extension");

// the extension of a key: slot ascending wins among equal (value, id), so the LARGER word must be the smaller slot; the pool position
// rides in the low bits (one position per slot: it decides nothing)
__device__ __forceinline__ unsigned mm_aux(int slot, int pos) { return ((unsigned)(CAND_MAX_C - 1 - slot) << 8) | (unsigned)pos; }
__device__ __forceinline__ bool mm_gt(rt_key_t ak, unsigned aa, rt_key_t bk, unsigned ba) { return ak > bk || (ak == bk && aa > ba); }

// chunk j of a row of H columns: one 16-byte load where the table allows it (vec: 16-byte aligned rows) and the chunk is whole, else
// four scalar loads; columns >= H are never read and count as 0
__device__ __forceinline__ float4 mm_chunk(const float* __restrict__ row, int j, int H, bool vec) {
  const int c = 4 * j;
  if (vec && c + 3 < H) return *reinterpret_cast<const float4*>(row + c);
  float4 v;
  v.x = c < H ? row[c] : 0.f;
  v.y = c + 1 < H ? row[c + 1] : 0.f;
  v.z = c + 2 < H ? row[c + 2] : 0.f;
  v.w = c + 3 < H ? row[c + 3] : 0.f;
  return v;
}
__device__ __forceinline__ void mm_fma4(float4 a, float4 b, float4& acc) {
  acc.x = fmaf(a.x, b.x, acc.x);
  acc.y = fmaf(a.y, b.y, acc.y);
  acc.z = fmaf(a.z, b.z, acc.z);
  acc.w = fmaf(a.w, b.w, acc.w);
}
// the four chains of one half -> the half's sum -> the dot (in both lanes of the pair)
__device__ __forceinline__ float mm_close(float4 acc) {
  const float h = (acc.x + acc.y) + (acc.z + acc.w);
  return h + __shfl_xor(h, 1);
}
__device__ __forceinline__ float mm_rnorm(float ss) { return ss > 0.f ? __fdiv_rn(1.f, __fsqrt_rn(ss)) : 0.f; }

template <int NC>
__global__ __launch_bounds__(MM_NT) void mmr_walk_kernel(int C, int k, float mu, int N, int H, const float* __restrict__ content, long ldc,
                                                         int vec, const int32_t* __restrict__ cand, long ld_cand,
                                                         const float* __restrict__ score, long ld_score,
                                                         const int32_t* __restrict__ order, int32_t* __restrict__ topk,
                                                         float* __restrict__ out_score, float* __restrict__ msim) {
  __shared__ int pslot[MM_POOL];             // the pool: slots in list order
  __shared__ int wcnt[MM_NWV];
  __shared__ rt_key_t wkey[MM_NWV];
  __shared__ unsigned waux[MM_NWV];
  __shared__ float4 prow[2 * (NC > 0 ? NC : 1)];      // the pick's row (register form)
  __shared__ float pr;                       // ... and its 1 / norm
  __shared__ int pid;                        // ... and its id (the form for any H reads the row from the table)
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nt = blockDim.x, nwv = nt >> 6;
  const int32_t* cb = cand + (long)b * ld_cand;
  const float* sb = score + (long)b * ld_score;
  const int32_t* ob = order + (long)b * C;
  topk += (long)b * k;
  if (out_score) out_score += (long)b * k;
  if (msim) msim += (long)b * k;

  // ---- the pool: the first 256 eligible slots of the order, compacted in order (ballot prefix per wave, wave counts through LDS)
  int P = 0;
  for (int base = 0; base < C && P < MM_POOL; base += nt) {
    const int j = base + tid;
    const int s = j < C ? ob[j] : -1;
    bool ok = false;
    if (s >= 0 && s < C) {
      const int id = cb[s];
      const float v = sb[s];
      ok = (unsigned)id < (unsigned)N && v == v && v != -INFINITY;
    }
    const unsigned long long bal = __ballot(ok);
    if (lane == 0) wcnt[w] = __popcll(bal);
    __syncthreads();
    int off = P, tot = P;
    for (int i = 0; i < nwv; ++i) {
      const int c = wcnt[i];
      off += i < w ? c : 0;
      tot += c;
    }
    const int at = off + __popcll(bal & ((1ull << lane) - 1ull));
    if (ok && at < MM_POOL) pslot[at] = s;
    __syncthreads();
    P = min(tot, MM_POOL);
  }
  if (P == 0) {
    for (int j = tid; j < k; j += nt) topk[j] = -1;
    return;
  }

  // ---- this lane's slot, its half of the row and the row's 1 / norm
  const int p = tid >> 1, half = tid & 1;
  const bool active = p < P;
  const bool wave_on = (w << 5) < P;         // wave-uniform: the wave holds a pool slot
  const int slot = active ? pslot[p] : 0;
  const int id = active ? cb[slot] : 0;
  const float sc = active ? sb[slot] : 0.f;
  const float* row = content + (long)id * ldc;          // (id == 0 where the lane is idle: row 0 exists, and is not read)
  const int nj = (H + 3) >> 2;               // chunks of a row
  float4 x[NC > 0 ? NC : 1];
  float r = 0.f;
  if (wave_on) {
    float4 acc = zero4();
    if constexpr (NC > 0) {
#pragma unroll
      for (int i = 0; i < NC; ++i) x[i] = active && 2 * i + half < nj ? mm_chunk(row, 2 * i + half, H, vec != 0) : zero4();
#pragma unroll
      for (int i = 0; i < NC; ++i) mm_fma4(x[i], x[i], acc);
    } else {
      for (int j = half; j < nj; j += 2) {
        const float4 a = active ? mm_chunk(row, j, H, vec != 0) : zero4();
        mm_fma4(a, a, acc);
      }
    }
    r = mm_rnorm(mm_close(acc));
  }

  // ---- the walk
  float m = 0.f;
  bool taken = !active;
  for (int t = 0; t < k; ++t) {
    if (t >= P) {                            // the pool is used up
      for (int j = t + tid; j < k; j += nt) topk[j] = -1;
      break;
    }
    rt_key_t key = 0;
    unsigned aux = 0u;
    if (!taken && half == 0) {
      key = rt_key(__fsub_rn(sc, __fmul_rn(mu, m)), id);
      aux = mm_aux(slot, p);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const rt_key_t ok = __shfl_xor(key, o);
      const unsigned oa = __shfl_xor(aux, o);
      if (mm_gt(ok, oa, key, aux)) { key = ok; aux = oa; }
    }
    if (lane == 0) { wkey[w] = key; waux[w] = aux; }
    __syncthreads();
    key = wkey[0];
    aux = waux[0];
    for (int i = 1; i < nwv; ++i) {
      const rt_key_t ok = wkey[i];
      const unsigned oa = waux[i];
      if (mm_gt(ok, oa, key, aux)) { key = ok; aux = oa; }
    }
    const int pw = (int)(aux & 255u);        // t < P: a slot is left, and every real key is > 0
    if (active && p == pw) {
      taken = true;
      if constexpr (NC > 0) {
#pragma unroll
        for (int i = 0; i < NC; ++i) prow[2 * i + half] = x[i];
      }
      if (half == 0) {
        pr = r;
        pid = id;
        topk[t] = id;
        if (out_score) out_score[t] = sc;
        if (msim) msim[t] = m;
      }
    }
    if (t == k - 1) break;
    __syncthreads();
    if (wave_on) {
      float4 acc = zero4();
      if constexpr (NC > 0) {
#pragma unroll
        for (int i = 0; i < NC; ++i) mm_fma4(x[i], prow[2 * i + half], acc);
      } else {
        const float* prw = content + (long)pid * ldc;
        for (int j = half; j < nj; j += 2) {
          const float4 a = active ? mm_chunk(row, j, H, vec != 0) : zero4();
          const float4 y = active ? mm_chunk(prw, j, H, vec != 0) : zero4();
          mm_fma4(a, y, acc);
        }
      }
      const float sim = mm_close(acc) * (r * pr);
      if (!taken) m = fmaxf(m, sim);
    }
  }
}

}  // namespace

extern "C" int tcar_mmr_abi_version(void) { return TCAR_MMR_ABI_VERSION; }

extern "C" int tcar_mmr_walk(int B, int C, int k, float mu, int N, int H, const float* content, int64_t ld_content, const int32_t* cand,
                             int64_t ld_cand, const float* score, int64_t ld_score, const int32_t* order, int32_t* topk, float* out_score,
                             float* msim, void* stream) {
  if (B < 0 || C < 1 || C > CAND_MAX_C || k < 1 || k > SEL_MAX_K || k > C || N < 1 || H < 1) return TCAR_E_ARG;
  if (!(mu >= 0.f) || isinf(mu) || ld_content < H || ld_cand < C || ld_score < C) return TCAR_E_ARG;
  if ((int64_t)(N - 1) * ld_content + H > 0x7fffffffffffL) return TCAR_E_ARG;
  if (B == 0) return TCAR_OK;
  if (!content || !cand || !score || !order || !topk || ((uintptr_t)content & 3)) return TCAR_E_ARG;
  const int vec = tcar_aligned16(content) && !(ld_content & 3);
  const int slots = C < MM_POOL ? C : MM_POOL;
  const dim3 grid((unsigned)B), block((unsigned)((2 * slots + 63) & ~63));
  hipStream_t s = (hipStream_t)stream;
#define MMR_GO(NC)                                                                                                                     \
  TCAR_LAUNCH((mmr_walk_kernel<NC>), grid, block, 0, s, C, k, mu, N, H, content, (long)ld_content, vec, cand, (long)ld_cand, score, \
              (long)ld_score, order, topk, out_score, msim)
  if (H <= 32) MMR_GO(4);
  else if (H <= 128) MMR_GO(16);
  else if (H <= 8 * MM_NC) MMR_GO(MM_NC);
  else MMR_GO(0);
#undef MMR_GO
  TCAR_CHECK_LAUNCH();
  return TCAR_OK;
}
