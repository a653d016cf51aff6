// The 64 x 64 cosine tile that csrc/similar.hip (the panels of tcar_similar.h) and csrc/dupes.hip (the audit of tcar_dupes.h) share:
// the pieces of `sim` (include/tcar_mmr.h) and ONE K loop, so both kernels give the same bits for the same pair of rows.
//
// Summation order (fixed by H alone): every dot is EIGHT fma chains, chain j over the columns c % 8 == j in ascending order from +0,
// closed as ((c0 + c1) + (c2 + c3)) + ((c4 + c5) + (c6 + c7)).  Columns past H contribute fma(0, 0, acc) = acc.  The chains are plain
// scalar fmaf on the VALU, eight accumulators per output.
//
// The tile.  A workgroup of SM_NT = 256 threads owns 64 x 64 outputs (x rows by y rows); thread (tq, tn) = (tid >> 4, tid & 15) owns
// the 4 x 4 outputs (tq + 16 i, tn + 16 m), 128 accumulators.  K runs in chunks of 32 columns = 4 steps of 8 (one column per chain):
// both operand tiles of a chunk sit in LDS as [64][32 + 4] floats (the pad makes the 16 rows a wave reads in one 16-byte LDS
// instruction fall into 16 distinct bank quads), the next chunk's global loads are in flight in registers while the chunk is
// contracted.  Row arithmetic is written on scalars: the library carries no packed fp32 math (DESIGN.md §7 observation 1).
#ifndef TCAR_SIM_TILE_H
#define TCAR_SIM_TILE_H

#include "tcar_common.h"

namespace {

constexpr int SM_T = 64;                     // rows of a tile, on both sides
constexpr int SM_KC = 32, SM_LD = SM_KC + 4; // columns of a K chunk; floats per LDS row
constexpr int SM_NT = 256;
constexpr int SM_R = 4;                      // outputs per thread and side: rows tq + 16 i of x, rows tn + 16 m of y

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

// what thread tid loads of a chunk: two 4-column pieces per tile — piece e = tid + 256 u is columns 4 (e & 7) .. + 3 of row e >> 3
__device__ __forceinline__ int sm_piece_row(int tid, int u) { return (tid + SM_NT * u) >> 3; }

// The K loop: acc[i][m][j] += chain j of x row (tq + 16 i) . y row (tn + 16 m) over the H columns.  xrow[u] / yrow[u]: the global
// row of this thread's piece u on either side (sm_piece_row; nullptr: a row that does not exist and counts as zeros); xs / ys: the
// two [SM_T][SM_LD] LDS tiles, free again behind the call (it ends on a barrier).  NORM: thread t also adds chains 2 (t >> 6) and
// 2 (t >> 6) + 1 of y row t & 63 's x . x into (na, nb) as the chunks pass — the item-norm side sum of the panel kernel.
template <bool NORM>
__device__ __forceinline__ void sm_contract(int H, const float* const (&xrow)[2], bool vecx, const float* const (&yrow)[2], bool vecy,
                                            float* __restrict__ xs, float* __restrict__ ys, float (&acc)[SM_R][SM_R][8], float& na,
                                            float& nb) {
  const int tid = threadIdx.x, tn = tid & 15, tq = tid >> 4;
  int lcol[2], lat[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int e = tid + SM_NT * u;
    lcol[u] = 4 * (e & 7);
    lat[u] = (e >> 3) * SM_LD + lcol[u];
  }
  const int nitem = tid & 63, npair = 2 * (tid >> 6);                    // the y row and the two chains of the norm this thread adds

  float4 px[2], py[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    px[u] = sm_chunk(xrow[u], lcol[u], H, vecx);
    py[u] = sm_chunk(yrow[u], lcol[u], H, vecy);
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
        px[u] = sm_chunk(xrow[u], k0 + SM_KC + lcol[u], H, vecx);
        py[u] = sm_chunk(yrow[u], k0 + SM_KC + lcol[u], H, vecy);
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
      if (NORM) {
        const float ya = ys[nitem * SM_LD + 8 * s + npair], yb = ys[nitem * SM_LD + 8 * s + npair + 1];
        na = fmaf(ya, ya, na);
        nb = fmaf(yb, yb, nb);
      }
    }
    __syncthreads();
  }
}

}  // namespace
#endif
