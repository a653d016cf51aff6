// Related items (include/tcar_similar.h): the cosine panels.  tcar_sim_queries copies the Q query rows into xq and computes their
// 1 / norm; tcar_sim_panel writes panel[q, j] = sim(query q, item n0 + j), the [Q, n] block a fold of tcar_serve.h reads.
//
// Summation order (fixed by H alone, tcar_mmr.h): every dot is EIGHT fma chains, chain j over the columns c % 8 == j in ascending
// order from +0, closed as ((c0 + c1) + (c2 + c3)) + ((c4 + c5) + (c6 + c7)) — csrc/mmr.hip's two halves of four chains.  Columns
// past H contribute fma(0, 0, acc) = acc.  Here the chains are plain scalar fmaf on the VALU, eight accumulators per output: this
// form is certain to give the bits of mmr.hip (docs/KERNELS.md has the MFMA form that was not built).
//
// The panel kernel.  A workgroup of 256 threads owns a 64 x 64 tile (queries x items); thread (tq, tn) = (tid >> 4, tid & 15) owns
// the 4 x 4 outputs (tq + 16 i, tn + 16 m), 128 accumulators.  K runs in chunks of 32 columns = 4 steps of 8 (one column per chain):
// both operand tiles of a chunk sit in LDS as [64][32 + 4] floats (the pad makes the 16 rows a wave reads in one 16-byte LDS
// instruction fall into 16 distinct bank quads), the next chunk's global loads are in flight in registers while the chunk is
// contracted.  The item side's r comes from the same LDS tile: thread t adds chains 2 (t >> 6) and 2 (t >> 6) + 1 of item t & 63
// as the chunks pass, the eight chains meet in LDS behind the K loop and every thread closes the four items it owns.
// Row arithmetic is written on scalars: the library carries no packed fp32 math (DESIGN.md §7 observation 1).
#include "tcar_common.h"
#include "../../include/tcar_similar.h"
#include <math.h>

namespace {

constexpr int SM_T = 64;                     // rows of a tile, queries and items alike
constexpr int SM_KC = 32, SM_LD = SM_KC + 4; // columns of a K chunk; floats per LDS row
constexpr int SM_NT = 256;
constexpr int SM_R = 4;                      // outputs per thread and side: rows tq + 16 i, items tn + 16 m

__device__ __forceinline__ float sm_rnorm(float ss) { return ss > 0.f ? __fdiv_rn(1.f, __fsqrt_rn(ss)) : 0.f; }
__device__ __forceinline__ float sm_close(const float (&c)[8]) { return ((c[0] + c[1]) + (c[2] + c[3])) + ((c[4] + c[5]) + (c[6] + c[7])); }

// columns c .. c + 3 of a row of H columns (row == nullptr: a row that does not exist): one 16-byte load where the table allows it
// (vec: 16-byte aligned rows) and the four columns exist, else scalar loads; columns >= H are never read and count as 0
__device__ __forceinline__ float4 sm_chunk(const float* __restrict__ row, int c, int H, bool vec) {
  if (!row) return zero4();
  if (vec && c + 3 < H) return *reinterpret_cast<const float4*>(row + c);
  float4 v;
  v.x = c < H ? row[c] : 0.f;
  v.y = c + 1 < H ? row[c + 1] : 0.f;
  v.z = c + 2 < H ? row[c + 2] : 0.f;
  v.w = c + 3 < H ? row[c + 3] : 0.f;
  return v;
}

// ---- the prologue: eight lanes per query, lane j is chain j
__global__ __launch_bounds__(SM_NT) void sim_queries_kernel(int Q, int N, int H, const float* __restrict__ content, long ldc,
                                                            const int32_t* __restrict__ qid, const float* __restrict__ qrow, long ldq,
                                                            float* __restrict__ xq, long ldx, float* __restrict__ rq) {
  const int q = blockIdx.x * (SM_NT / 8) + (threadIdx.x >> 3), j = threadIdx.x & 7;
  const float* src = nullptr;
  if (q < Q) {
    if (qid) {
      const int id = qid[q];
      if ((unsigned)id < (unsigned)N) src = content + (long)id * ldc;
    } else {
      src = qrow + (long)q * ldq;
    }
  }
  float acc = 0.f;
  for (int c = j; c < H; c += 8) {
    const float v = src ? src[c] : 0.f;
    if (q < Q) xq[(long)q * ldx + c] = v;
    acc = fmaf(v, v, acc);
  }
  // lanes 8 g .. 8 g + 7 hold c0 .. c7: (c0 + c1), then + (c2 + c3), then half 0 + half 1 — every add commutative, so all eight
  // lanes end with the same bits
  acc = acc + __shfl_xor(acc, 1);
  acc = acc + __shfl_xor(acc, 2);
  acc = acc + __shfl_xor(acc, 4);
  if (q < Q && j == 0) rq[q] = sm_rnorm(acc);
}

// ---- the panel
__global__ __launch_bounds__(SM_NT) void sim_panel_kernel(int Q, int n0, int n, int H, const float* __restrict__ content, long ldc, int vecc,
                                                          const float* __restrict__ xq, long ldx, int vecq, const float* __restrict__ rq,
                                                          float* __restrict__ panel, long ld) {
  __shared__ __attribute__((aligned(16))) float xs[SM_T * SM_LD];        // the query tile of the chunk
  __shared__ __attribute__((aligned(16))) float ys[SM_T * SM_LD];        // the item tile of the chunk
  __shared__ float nrm[SM_T * 8];                                        // the eight chains of every item's x . x
  const int tid = threadIdx.x, tn = tid & 15, tq = tid >> 4;
  const int q0 = blockIdx.x * SM_T, j0 = blockIdx.y * SM_T;
  // what this thread loads of a chunk: two 4-column pieces per tile — piece e = tid + 256 u is columns 4 (e & 7) .. + 3 of row e >> 3
  const float* xrow[2];
  const float* yrow[2];
  int lcol[2], lat[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int e = tid + SM_NT * u, row = e >> 3;
    lcol[u] = 4 * (e & 7);
    lat[u] = row * SM_LD + lcol[u];
    xrow[u] = q0 + row < Q ? xq + (long)(q0 + row) * ldx : nullptr;
    yrow[u] = j0 + row < n ? content + ((long)n0 + j0 + row) * ldc : nullptr;
  }
  const int nitem = tid & 63, npair = 2 * (tid >> 6);                    // the item and the two chains of the norm this thread adds

  float acc[SM_R][SM_R][8];
#pragma unroll
  for (int i = 0; i < SM_R; ++i)
#pragma unroll
    for (int m = 0; m < SM_R; ++m)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[i][m][j] = 0.f;
  float na = 0.f, nb = 0.f;

  float4 px[2], py[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    px[u] = sm_chunk(xrow[u], lcol[u], H, vecq != 0);
    py[u] = sm_chunk(yrow[u], lcol[u], H, vecc != 0);
  }
  for (int k0 = 0; k0 < H; k0 += SM_KC) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      *reinterpret_cast<float4*>(xs + lat[u]) = px[u];
      *reinterpret_cast<float4*>(ys + lat[u]) = py[u];
    }
    __syncthreads();
    if (k0 + SM_KC < H) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        px[u] = sm_chunk(xrow[u], k0 + SM_KC + lcol[u], H, vecq != 0);
        py[u] = sm_chunk(yrow[u], k0 + SM_KC + lcol[u], H, vecc != 0);
      }
    }
#pragma unroll
    for (int s = 0; s < SM_KC / 8; ++s) {
      float b[SM_R][8];
#pragma unroll
      for (int m = 0; m < SM_R; ++m) {
        const float4 lo = *reinterpret_cast<const float4*>(ys + (tn + 16 * m) * SM_LD + 8 * s);
        const float4 hi = *reinterpret_cast<const float4*>(ys + (tn + 16 * m) * SM_LD + 8 * s + 4);
        b[m][0] = lo.x; b[m][1] = lo.y; b[m][2] = lo.z; b[m][3] = lo.w;
        b[m][4] = hi.x; b[m][5] = hi.y; b[m][6] = hi.z; b[m][7] = hi.w;
      }
#pragma unroll
      for (int i = 0; i < SM_R; ++i) {
        const float4 lo = *reinterpret_cast<const float4*>(xs + (tq + 16 * i) * SM_LD + 8 * s);
        const float4 hi = *reinterpret_cast<const float4*>(xs + (tq + 16 * i) * SM_LD + 8 * s + 4);
        const float a[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (int m = 0; m < SM_R; ++m)
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[i][m][j] = fmaf(a[j], b[m][j], acc[i][m][j]);
      }
      const float ya = ys[nitem * SM_LD + 8 * s + npair], yb = ys[nitem * SM_LD + 8 * s + npair + 1];
      na = fmaf(ya, ya, na);
      nb = fmaf(yb, yb, nb);
    }
    __syncthreads();
  }

  nrm[nitem * 8 + npair] = na;
  nrm[nitem * 8 + npair + 1] = nb;
  __syncthreads();
  float ry[SM_R];
#pragma unroll
  for (int m = 0; m < SM_R; ++m) {
    float c[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) c[j] = nrm[(tn + 16 * m) * 8 + j];
    ry[m] = sm_rnorm(sm_close(c));
  }
#pragma unroll
  for (int i = 0; i < SM_R; ++i) {
    const int q = q0 + tq + 16 * i;
    if (q >= Q) continue;
    const float r = rq[q];
    float* out = panel + (long)q * ld;
#pragma unroll
    for (int m = 0; m < SM_R; ++m) {
      const int j = j0 + tn + 16 * m;
      if (j < n) out[j] = sm_close(acc[i][m]) * (r * ry[m]);
    }
  }
}

bool sm_bad_table(int H, const float* t, int64_t ld) { return !t || ((uintptr_t)t & 3) || ld < H; }

}  // namespace

extern "C" int tcar_similar_abi_version(void) { return TCAR_SIMILAR_ABI_VERSION; }

extern "C" int tcar_sim_queries(int Q, int N, int H, const float* content, int64_t ld_content, const int32_t* qid, const float* qrow,
                                int64_t ld_qrow, float* xq, int64_t ld_xq, float* rq, void* stream) {
  if (Q < 0 || N < 1 || H < 1 || !qid == !qrow) return TCAR_E_ARG;
  if (qid ? sm_bad_table(H, content, ld_content) || ((uintptr_t)qid & 3) : sm_bad_table(H, qrow, ld_qrow)) return TCAR_E_ARG;
  if (qid && (int64_t)(N - 1) * ld_content + H > 0x7fffffffffffL) return TCAR_E_ARG;
  if (sm_bad_table(H, xq, ld_xq) || !rq || ((uintptr_t)rq & 3)) return TCAR_E_ARG;
  if (Q == 0) return TCAR_OK;
  const dim3 grid((unsigned)((Q + SM_NT / 8 - 1) / (SM_NT / 8))), block(SM_NT);
  TCAR_LAUNCH(sim_queries_kernel, grid, block, 0, (hipStream_t)stream, Q, N, H, content, (long)ld_content, qid, qrow, (long)ld_qrow, xq,
              (long)ld_xq, rq);
  TCAR_CHECK_LAUNCH();
  return TCAR_OK;
}

extern "C" int tcar_sim_panel(int Q, int n0, int n, int H, const float* content, int64_t ld_content, const float* xq, int64_t ld_xq,
                              const float* rq, float* panel, int64_t ld, void* stream) {
  if (Q < 0 || n0 < 0 || n < 0 || n > SEL_MAX_N || H < 1 || (ld & 3) || ld < n) return TCAR_E_ARG;
  if (sm_bad_table(H, content, ld_content) || sm_bad_table(H, xq, ld_xq) || !rq || ((uintptr_t)rq & 3)) return TCAR_E_ARG;
  if (!panel || !tcar_aligned16(panel)) return TCAR_E_ARG;
  if ((int64_t)n0 + n > 0x7fffffffL || ((int64_t)n0 + n) * ld_content > 0x7fffffffffffL) return TCAR_E_ARG;
  if (Q == 0 || n == 0) return TCAR_OK;
  const int vecc = tcar_aligned16(content) && !(ld_content & 3), vecq = tcar_aligned16(xq) && !(ld_xq & 3);
  const dim3 grid((unsigned)((Q + SM_T - 1) / SM_T), (unsigned)((n + SM_T - 1) / SM_T)), block(SM_NT);
  TCAR_LAUNCH(sim_panel_kernel, grid, block, 0, (hipStream_t)stream, Q, n0, n, H, content, (long)ld_content, vecc, xq, (long)ld_xq, vecq, rq,
              panel, (long)ld);
  TCAR_CHECK_LAUNCH();
  return TCAR_OK;
}
