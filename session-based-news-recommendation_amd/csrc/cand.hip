// Candidate-list scoring (include/tcar_cand.h): every session names C catalog items and only those rows are read — a GATHER, not a
// GEMM, since every session has rows of its own.  cand_scores_kernel computes the [B, C] dots from the operands the panel GEMM of the
// streamed selection contracts (fp32 rows or KB32 planes); cand_rank_kernel turns a list's scores into ranks, the list order and the
// impression metrics (AUC pair counts, MRR, nDCG@5, nDCG@10).  Neither kernel uses LDS for the operands or an MFMA: the first is
// bound by the gathered bytes, the second by C^2 comparisons on LDS broadcasts.
//
// List order of the slots: score descending, then item id descending (key_gt of topk_rows.h, the library's one list order), then slot
// ascending — reached by repeats of one id only.  A total order over the slots: the ranks are a permutation.
#include "tcar_common.h"
#include "tcar_bf16_layout.h"
#include "topk_rows.h"
#include "../../include/tcar_retrieve_shard.h"

namespace {

// ---- scores.  A row of K columns is K / 4 CHUNKS of four columns: 16 contiguous bytes of an fp32 row, 8 contiguous bytes of a KB32
// plane (kb32_off with k % 4 == 0).  Lane l of a wave owns the chunks l, l + 64, l + 128, ...; one wave computes one dot.
//   * The session's own row is loop-invariant: a wave converts its chunks to floats ONCE, into registers (CS_NI chunks per lane: rows
//     of up to 1,024 columns; longer rows take the form that re-reads the session chunk beside every pair of candidates).
//   * A wave keeps CS_U candidates in flight: all their loads are issued before the first is consumed (CS_U x CS_NI x 2 planes
//     independent 8-byte loads per lane at most), which is what a latency-bound gather needs.
//   * Summation order of one dot: per lane its chunks in ascending order, inside a chunk x, y, z, w, as one fma chain per KIND of
//     product — hi hi into `acc`, and hi lo then lo hi of every chunk into `acs` — then acc + acs and the xor butterfly 32 .. 1.
//     It depends on K and nsplit alone (they pick the form), never on the slot, C, B or the rest of the list; skipped chunks
//     (4 j >= K) contribute fma(0, 0, acc) = acc.
constexpr int CS_NT = 256, CS_NWV = CS_NT / 64;
constexpr int CS_U = 2;            // candidates a wave has in flight
constexpr int CS_WG = 64;          // slots of one workgroup: the session chunks a wave converts serve 16 dots
constexpr int CS_NI = 4;           // chunks per lane the register form holds
enum { CS_F32 = 0, CS_HI = 1, CS_X3 = 3 };

template <int MODE> struct CsRaw { typedef uint2 T; };
template <> struct CsRaw<CS_F32> { typedef float4 T; };
template <int MODE> __device__ __forceinline__ typename CsRaw<MODE>::T cs_zero() {
  if constexpr (MODE == CS_F32) return zero4();
  else return make_uint2(0u, 0u);
}
__device__ __forceinline__ float4 cs_cvt(float4 v) { return v; }
// four bf16 (element 0 in the low half of .x) -> four floats, exactly
__device__ __forceinline__ float4 cs_cvt(uint2 q) {
  return make_float4(__uint_as_float(q.x << 16), __uint_as_float(q.x & 0xffff0000u), __uint_as_float(q.y << 16),
                     __uint_as_float(q.y & 0xffff0000u));
}
// chunk j of row `row`: fp32 — base is the matrix, ld its row stride in floats; planes — base is the plane, ld its inner / 32
template <int MODE> __device__ __forceinline__ typename CsRaw<MODE>::T cs_load(const void* base, long row, long ld, int j) {
  if constexpr (MODE == CS_F32) return *reinterpret_cast<const float4*>(static_cast<const float*>(base) + row * ld + 4 * j);
  else return *reinterpret_cast<const uint2*>(static_cast<const __bf16*>(base) + kb32_off(row, 4 * j, (int)ld));
}
__device__ __forceinline__ float cs_chain(float4 a, float4 e, float acc) {
  return fmaf(a.w, e.w, fmaf(a.z, e.z, fmaf(a.y, e.y, fmaf(a.x, e.x, acc))));
}

// grid (B, ceil(C / CS_WG)).  NI > 0: the register form for K <= 256 NI; NI == 0: any K.  a0 / a1, e0 / e1: hi / lo planes (a1, e1 read
// by CS_X3 only), or the fp32 matrices in a0 / e0.  id0: the catalog id of the operands' first row (0: the whole catalog) — slot id i reads
// local row i - id0 iff (unsigned)(i - id0) < N; the dot itself knows nothing of it.
template <int MODE, int NI>
__global__ __launch_bounds__(CS_NT) void cand_scores_kernel(int C, int N, int K, const void* __restrict__ a0, const void* __restrict__ a1,
                                                            long a_ld, const void* __restrict__ e0, const void* __restrict__ e1, long e_ld,
                                                            const int32_t* __restrict__ cand, long ld_cand, float* __restrict__ out,
                                                            long ld_out, int id0) {
  typedef typename CsRaw<MODE>::T raw_t;
  constexpr bool X3 = MODE == CS_X3;
  constexpr int NR = NI > 0 ? NI : 1;
  const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int nj = K >> 2;
  const int c0 = blockIdx.y * CS_WG, c1 = min(C, c0 + CS_WG);
  const int32_t* cb = cand + (long)b * ld_cand;
  float* ob = out + (long)b * ld_out;
  float4 ah[NR], al[X3 ? NR : 1];
  if constexpr (NI > 0) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int j = lane + 64 * i;
      ah[i] = j < nj ? cs_cvt(cs_load<MODE>(a0, b, a_ld, j)) : zero4();
      if constexpr (X3) al[i] = j < nj ? cs_cvt(cs_load<MODE>(a1, b, a_ld, j)) : zero4();
    }
  }
  for (int c = c0 + w * CS_U; c < c1; c += CS_NWV * CS_U) {
    int id[CS_U];
    bool ok[CS_U];                 // wave-uniform: an id outside the catalog reads no row
#pragma unroll
    for (int u = 0; u < CS_U; ++u) {
      const unsigned loc = (unsigned)(c + u < c1 ? __builtin_amdgcn_readfirstlane(cb[c + u]) : -1) - (unsigned)id0;
      ok[u] = c + u < c1 && loc < (unsigned)N;
      id[u] = (int)loc;
    }
    float acc[CS_U], acs[CS_U];
#pragma unroll
    for (int u = 0; u < CS_U; ++u) acc[u] = acs[u] = 0.f;
    if constexpr (NI > 0) {
      raw_t rh[CS_U][NI], rl[CS_U][X3 ? NI : 1];
#pragma unroll
      for (int u = 0; u < CS_U; ++u) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          const int j = lane + 64 * i;
          const bool on = ok[u] && j < nj;
          rh[u][i] = on ? cs_load<MODE>(e0, id[u], e_ld, j) : cs_zero<MODE>();
          if constexpr (X3) rl[u][i] = on ? cs_load<MODE>(e1, id[u], e_ld, j) : cs_zero<MODE>();
        }
      }
#pragma unroll
      for (int u = 0; u < CS_U; ++u) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          const float4 eh = cs_cvt(rh[u][i]);
          acc[u] = cs_chain(ah[i], eh, acc[u]);
          if constexpr (X3) {
            acs[u] = cs_chain(ah[i], cs_cvt(rl[u][i]), acs[u]);
            acs[u] = cs_chain(al[i], eh, acs[u]);
          }
        }
      }
    } else {
      for (int j = lane; j < ((nj + 63) & ~63); j += 64) {
        const bool in = j < nj;
        const float4 xh = in ? cs_cvt(cs_load<MODE>(a0, b, a_ld, j)) : zero4();
        float4 xl = zero4();
        if constexpr (X3) xl = in ? cs_cvt(cs_load<MODE>(a1, b, a_ld, j)) : zero4();
        raw_t rh[CS_U], rl[CS_U];
#pragma unroll
        for (int u = 0; u < CS_U; ++u) {
          const bool on = ok[u] && in;
          rh[u] = on ? cs_load<MODE>(e0, id[u], e_ld, j) : cs_zero<MODE>();
          rl[u] = cs_zero<MODE>();
          if constexpr (X3) rl[u] = on ? cs_load<MODE>(e1, id[u], e_ld, j) : cs_zero<MODE>();
        }
#pragma unroll
        for (int u = 0; u < CS_U; ++u) {
          const float4 eh = cs_cvt(rh[u]);
          acc[u] = cs_chain(xh, eh, acc[u]);
          if constexpr (X3) {
            acs[u] = cs_chain(xh, cs_cvt(rl[u]), acs[u]);
            acs[u] = cs_chain(xl, eh, acs[u]);
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < CS_U; ++u) {
      const float s = wave_sum(X3 ? acc[u] + acs[u] : acc[u]);
      if (lane == 0 && c + u < c1) ob[c + u] = ok[u] ? s : -INFINITY;
    }
  }
}

// ---- ranks and metrics.  One workgroup per session; the list (score, id, class) sits in LDS and every thread counts, for each of its
// at most four slots, the slots that PRECEDE it in the list order: all lanes read the same LDS word in an iteration (a broadcast),
// C^2 comparisons per session, no sort network, exact by construction.  The same sweep counts, for a positive slot, the negatives it
// beats (2) or ties (1) by score alone.  `order` is the scatter of the slots by rank through LDS; the integer totals are LDS atomic
// adds (integers: no order to fix); the float sums run over RANKS in a fixed shape — mrr: thread t adds ranks t + 1, t + 257, ... in
// ascending order, xor butterfly, the four waves in ascending order; the two DCG sums: ranks 1 .. 10 in ascending order by one thread.
// (A form with one 16-byte LDS entry per slot, read once for the thread's four slots, measured SLOWER: docs/EXPERIMENTS.md.)
constexpr int CR_NT = 256, CR_NWV = CR_NT / 64, CR_R = CAND_MAX_C / CR_NT;
enum { CR_EMPTY = 0, CR_NEG = 1, CR_POS = 2 };

__global__ __launch_bounds__(CR_NT) void cand_rank_kernel(int C, const float* __restrict__ score, long ld_score,
                                                          const int32_t* __restrict__ cand, long ld_cand,
                                                          const int32_t* __restrict__ clicked, long ld_clicked,
                                                          int32_t* __restrict__ rank_of, int32_t* __restrict__ order,
                                                          int32_t* __restrict__ counts, float* __restrict__ metrics) {
  __shared__ float sv[CAND_MAX_C];
  __shared__ int si[CAND_MAX_C];
  __shared__ int sf[CAND_MAX_C];            // CR_EMPTY / CR_NEG (every non-empty slot of an unlabelled call) / CR_POS
  __shared__ int byrank[CAND_MAX_C];        // the slot with rank r at r - 1; -1 behind the last
  __shared__ int tot[3];                    // npos, nneg, auc2
  __shared__ float part[CR_NWV];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid < 3) tot[tid] = 0;
  for (int j = tid; j < C; j += CR_NT) {
    const float v = score[(long)b * ld_score + j];
    const int id = cand[(long)b * ld_cand + j];
    const bool empty = id < 0 || v == -INFINITY;
    sv[j] = v;
    si[j] = id;
    sf[j] = empty ? CR_EMPTY : (clicked && clicked[(long)b * ld_clicked + j] != 0) ? CR_POS : CR_NEG;
    byrank[j] = -1;
  }
  __syncthreads();
  int npos = 0, nneg = 0, auc2 = 0;
#pragma unroll
  for (int r = 0; r < CR_R; ++r) {
    const int j = tid + r * CR_NT;
    if (j >= C) break;
    const float v = sv[j];
    const int id = si[j], f = sf[j];
    int rank = 0;
    if (f != CR_EMPTY) {
      int before = 0, won = 0;
      for (int i = 0; i < C; ++i) {
        const float xv = sv[i];
        const int xi = si[i], xf = sf[i];
        before += xf != CR_EMPTY && (key_gt(xv, xi, v, id) || (xv == v && xi == id && i < j));
        won += xf == CR_NEG ? 2 * (v > xv) + (v == xv) : 0;
      }
      rank = before + 1;
      byrank[before] = j;
      npos += f == CR_POS;
      nneg += f == CR_NEG;
      if (f == CR_POS) auc2 += won;
    }
    if (rank_of) rank_of[(long)b * C + j] = rank;
  }
  if (counts || metrics) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      npos += __shfl_xor(npos, o);
      nneg += __shfl_xor(nneg, o);
      auc2 += __shfl_xor(auc2, o);
    }
    if (lane == 0) { atomicAdd(&tot[0], npos); atomicAdd(&tot[1], nneg); atomicAdd(&tot[2], auc2); }
  }
  __syncthreads();
  if (order) {
    for (int j = tid; j < C; j += CR_NT) order[(long)b * C + j] = byrank[j];
  }
  if (counts && tid < 3) counts[(long)b * 3 + tid] = tot[tid];
  if (metrics) {
    float rr = 0.f;
    for (int r = tid; r < C; r += CR_NT) {
      const int s = byrank[r];
      if (s >= 0 && sf[s] == CR_POS) rr += 1.f / (float)(r + 1);
    }
    rr = wave_sum(rr);
    if (lane == 0) part[w] = rr;
    __syncthreads();
    if (tid == 0) {
      const int np = tot[0];
      float mrr = 0.f, d5 = 0.f, d10 = 0.f, i5 = 0.f, i10 = 0.f;
#pragma unroll
      for (int i = 0; i < CR_NWV; ++i) mrr += part[i];
      for (int r = 0; r < 10 && r < C; ++r) {
        const float g = 1.f / log2f((float)(r + 2));
        const int s = byrank[r];
        if (s >= 0 && sf[s] == CR_POS) { d10 += g; if (r < 5) d5 += g; }
        if (r < np) { i10 += g; if (r < 5) i5 += g; }
      }
      float* m = metrics + (long)b * 3;
      m[0] = np > 0 ? mrr / (float)np : 0.f;
      m[1] = np > 0 ? d5 / i5 : 0.f;
      m[2] = np > 0 ? d10 / i10 : 0.f;
    }
  }
}

inline bool bad_bc(int B, int C) { return B < 0 || C < 1 || C > CAND_MAX_C; }

template <int MODE>
void launch_scores(int B, int C, int N, int K, const void* a0, const void* a1, long a_ld, const void* e0, const void* e1, long e_ld,
                   const int32_t* cand, long ld_cand, float* out, long ld_out, int id0, hipStream_t s) {
  const dim3 grid((unsigned)B, (unsigned)((C + CS_WG - 1) / CS_WG)), block(CS_NT);
  if (K <= 256)
    TCAR_LAUNCH((cand_scores_kernel<MODE, 1>), grid, block, 0, s, C, N, K, a0, a1, a_ld, e0, e1, e_ld, cand, ld_cand, out, ld_out, id0);
  else if (K <= 512)
    TCAR_LAUNCH((cand_scores_kernel<MODE, 2>), grid, block, 0, s, C, N, K, a0, a1, a_ld, e0, e1, e_ld, cand, ld_cand, out, ld_out, id0);
  else if (K <= 256 * CS_NI)
    TCAR_LAUNCH((cand_scores_kernel<MODE, CS_NI>), grid, block, 0, s, C, N, K, a0, a1, a_ld, e0, e1, e_ld, cand, ld_cand, out, ld_out, id0);
  else
    TCAR_LAUNCH((cand_scores_kernel<MODE, 0>), grid, block, 0, s, C, N, K, a0, a1, a_ld, e0, e1, e_ld, cand, ld_cand, out, ld_out, id0);
}

// ---- the shards' score parts of a list -> the list's scores (include/tcar_retrieve_shard.h): slot (b, c) takes the WORD its owner wrote,
// owner = id / rows_per_shard; an id outside [0, N) or an owner >= S: -inf.  A copy of bits (NaN payloads and -0.0 included), one thread
// per slot.  Bounds: c < C <= ld of every matrix, owner < S, the part's row b starts at owner * stride + b * C.
constexpr int CC_NT = 256;
__global__ __launch_bounds__(CC_NT) void cand_combine_kernel(int C, int S, int rows_per_shard, int N, const int32_t* __restrict__ cand,
                                                             long ld_cand, const uint32_t* __restrict__ parts, long stride,
                                                             uint32_t* __restrict__ out, long ld_out) {
  const int b = blockIdx.x;
  for (int c = blockIdx.y * CC_NT + threadIdx.x; c < C; c += gridDim.y * CC_NT) {
    const int id = cand[(long)b * ld_cand + c];
    const int owner = (unsigned)id < (unsigned)N ? id / rows_per_shard : S;
    out[(long)b * ld_out + c] = owner < S ? parts[(long)owner * stride + (long)b * C + c] : 0xff800000u;
  }
}

}  // namespace

extern "C" int tcar_cand_combine(int B, int C, int S, int rows_per_shard, int N, const int32_t* cand, int64_t ld_cand, const float* parts,
                                 int64_t stride, float* out, int64_t ld_out, void* stream) {
  if (bad_bc(B, C) || S < 1 || S > 64 || rows_per_shard < 1 || N < 1 || ld_cand < C || ld_out < C) return TCAR_E_ARG;
  if (S > 1 && stride < (int64_t)B * C) return TCAR_E_ARG;
  if (B == 0) return TCAR_OK;
  if (!cand || !parts || !out || ((uintptr_t)parts & 3) || ((uintptr_t)out & 3)) return TCAR_E_ARG;
  const uintptr_t in0 = (uintptr_t)parts, in1 = in0 + (uintptr_t)(((int64_t)(S - 1) * stride + (int64_t)B * C) * 4);
  const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)((((int64_t)B - 1) * ld_out + C) * 4);
  if (o0 < in1 && in0 < o1) return TCAR_E_ARG;            // out overlaps the parts
  TCAR_LAUNCH(cand_combine_kernel, dim3((unsigned)B, (unsigned)((C + CC_NT - 1) / CC_NT)), dim3(CC_NT), 0, (hipStream_t)stream, C, S,
              rows_per_shard, N, cand, (long)ld_cand, (const uint32_t*)parts, (long)stride, (uint32_t*)out, (long)ld_out);
  TCAR_CHECK_LAUNCH();
  return TCAR_OK;
}

extern "C" int tcar_cand_abi_version(void) { return TCAR_CAND_ABI_VERSION; }

extern "C" int tcar_cand_scores(int B, int C, int N, int K, const float* att, int64_t ld_att, const float* E, int64_t ldE,
                                const void* a_hi, const void* a_lo, int64_t a_inner, const void* e_hi, const void* e_lo, int64_t e_inner,
                                int nsplit, const int32_t* cand, int64_t ld_cand, float* out, int64_t ld_out, void* stream) {
  return tcar_cand_scores_owned(B, C, N, K, att, ld_att, E, ldE, a_hi, a_lo, a_inner, e_hi, e_lo, e_inner, nsplit, cand, ld_cand, out,
                                ld_out, 0, stream);
}

extern "C" int tcar_cand_scores_owned(int B, int C, int N, int K, const float* att, int64_t ld_att, const float* E, int64_t ldE,
                                      const void* a_hi, const void* a_lo, int64_t a_inner, const void* e_hi, const void* e_lo,
                                      int64_t e_inner, int nsplit, const int32_t* cand, int64_t ld_cand, float* out, int64_t ld_out,
                                      int id0, void* stream) {
  if (id0 < 0 || (int64_t)id0 + N > 0x7fffffffL) return TCAR_E_ARG;
  if (bad_bc(B, C) || N <= 0 || K <= 0 || (K & 3) || ld_cand < C || ld_out < C) return TCAR_E_ARG;
  if (B == 0) return TCAR_OK;
  if (a_hi) {
    if (!e_hi || (nsplit != 1 && nsplit != 3) || (nsplit == 3 && (!a_lo || !e_lo)) || (a_inner & 31) || (e_inner & 31) || a_inner < K ||
        e_inner < K || ((uintptr_t)a_hi & 7) || ((uintptr_t)e_hi & 7) || (nsplit == 3 && (((uintptr_t)a_lo | (uintptr_t)e_lo) & 7)))
      return TCAR_E_ARG;
  } else {
    if ((ld_att & 3) || (ldE & 3) || ld_att < K || ldE < K) return TCAR_E_ARG;
  }
  if (!cand || !out) return TCAR_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (a_hi) {
    if (nsplit == 3)
      launch_scores<CS_X3>(B, C, N, K, a_hi, a_lo, (long)(a_inner >> 5), e_hi, e_lo, (long)(e_inner >> 5), cand, (long)ld_cand, out,
                           (long)ld_out, id0, s);
    else
      launch_scores<CS_HI>(B, C, N, K, a_hi, nullptr, (long)(a_inner >> 5), e_hi, nullptr, (long)(e_inner >> 5), cand, (long)ld_cand, out,
                           (long)ld_out, id0, s);
  } else {
    if (!att || !E || !tcar_aligned16(att) || !tcar_aligned16(E)) return TCAR_E_ARG;
    launch_scores<CS_F32>(B, C, N, K, att, nullptr, (long)ld_att, E, nullptr, (long)ldE, cand, (long)ld_cand, out, (long)ld_out, id0, s);
  }
  TCAR_CHECK_LAUNCH();
  return TCAR_OK;
}

extern "C" int tcar_cand_rank(int B, int C, const float* score, int64_t ld_score, const int32_t* cand, int64_t ld_cand,
                              const int32_t* clicked, int64_t ld_clicked, int32_t* rank_of, int32_t* order, int32_t* counts,
                              float* metrics, void* stream) {
  if (bad_bc(B, C) || ld_score < C || ld_cand < C) return TCAR_E_ARG;
  if (clicked ? ld_clicked < C : (counts || metrics)) return TCAR_E_ARG;
  if (B == 0) return TCAR_OK;
  if (!score || !cand) return TCAR_E_ARG;
  if (!rank_of && !order && !counts && !metrics) return TCAR_OK;          // nothing is asked for
  TCAR_LAUNCH(cand_rank_kernel, dim3((unsigned)B), dim3(CR_NT), 0, (hipStream_t)stream, C, score, (long)ld_score, cand, (long)ld_cand,
              clicked, (long)ld_clicked, rank_of, order, counts, metrics);
  TCAR_CHECK_LAUNCH();
  return TCAR_OK;
}
