// Related items (include/tcar_similar.h): the cosine panels.  tcar_sim_queries copies the Q query rows into xq and computes their
// 1 / norm; tcar_sim_panel writes panel[q, j] = sim(query q, item n0 + j), the [Q, n] block a fold of tcar_serve.h reads.
//
// The summation order of every dot, the 64 x 64 tile and its K loop are those of csrc/sim_tile.h, which csrc/dupes.hip shares.  The
// item side's r comes from the same LDS tile: thread t adds chains 2 (t >> 6) and 2 (t >> 6) + 1 of item t & 63 as the chunks pass
// (sm_contract<true>), the eight chains meet in LDS behind the K loop and every thread closes the four items it owns.
#include "sim_tile.h"
#include "../../include/tcar_similar.h"
#include <math.h>

namespace {

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
  const float* xrow[2];
  const float* yrow[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int row = sm_piece_row(tid, u);
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
  sm_contract<true>(H, xrow, vecq != 0, yrow, vecc != 0, xs, ys, acc, na, nb);

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
