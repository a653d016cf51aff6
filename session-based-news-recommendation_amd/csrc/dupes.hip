// The duplicate audit (include/tcar_dupes.h): count, best partner and its similarity for every item, from ONE pass over the upper
// triangle of the all-pairs cosine matrix of the content table.  Nothing of that matrix is written.
//
// tcar_dup_rnorm writes r = 1 / norm of every row with the chains, the close, the sqrt and the division of sim_queries_kernel
// (csrc/similar.hip).  tcar_dup_tiles runs one workgroup of 256 threads per 64 x 64 tile (rows i0 .. i0 + 63 against rows
// j0 .. j0 + 63, column block >= row block) through the K loop of csrc/sim_tile.h — the loop of sim_panel_kernel, so the dot has its
// bits — and closes sim = close(acc) * (r_i * r_j) from the r table instead of a norm side sum.
//
// The epilogue.  A thread tests its 16 sims against t, the membership of both rows and, in a diagonal tile, i < j; it keeps a count
// and a best key per row it owns (four on either side) in registers and adds the non-empty ones into cnt[128] / best[128] in LDS
// (integer atomics; slots 0 .. 63 the tile's i rows, 64 .. 127 its j rows; the operand tiles' LDS, free behind the K loop's last
// barrier).  Then 128 threads flush the non-zero slots: one global integer add and one global 64-bit max per touched row and tile,
// relaxed, agent scope, no value returned.  A tile without a match issues no global atomic.  Integer sums and maxima do not depend on
// the order of arrival, so the state is the same bits for every schedule and every partition into launches.
//
// The key of a pair as seen from row i: (float bits of sim) << 32 | j.  sim >= t > 0, so the bits order as the floats do and the larger
// key is the earlier place in the list order (sim descending, then id descending).  0 is no key: an admitted sim is > 0.
#include "sim_tile.h"
#include "../../include/tcar_dupes.h"
#include <math.h>

namespace {

typedef unsigned long long u64;

// ---- r of every row: eight lanes per row, lane j is chain j (the arithmetic of sim_queries_kernel)
__global__ __launch_bounds__(SM_NT) void dup_rnorm_kernel(int N, int H, const float* __restrict__ content, long ldc, float* __restrict__ r) {
  const long n = (long)blockIdx.x * (SM_NT / 8) + (threadIdx.x >> 3);
  const int j = threadIdx.x & 7;
  const float* src = n < N ? content + n * ldc : nullptr;
  float acc = 0.f;
  for (int c = j; c < H; c += 8) {
    const float v = src ? src[c] : 0.f;
    acc = fmaf(v, v, acc);
  }
  acc = acc + __shfl_xor(acc, 1);
  acc = acc + __shfl_xor(acc, 2);
  acc = acc + __shfl_xor(acc, 4);
  if (n < N && j == 0) r[n] = sm_rnorm(acc);
}

__global__ __launch_bounds__(SM_NT) void dup_reset_kernel(int N, int32_t* __restrict__ count, u64* __restrict__ best) {
  const long n = (long)blockIdx.x * SM_NT + threadIdx.x;
  if (n < N) {
    count[n] = 0;
    best[n] = 0ull;
  }
}

__global__ __launch_bounds__(SM_NT) void dup_finish_kernel(int N, const u64* __restrict__ best, int32_t* __restrict__ partner,
                                                           float* __restrict__ psim) {
  const long n = (long)blockIdx.x * SM_NT + threadIdx.x;
  if (n < N) {
    const u64 b = best[n];
    partner[n] = b ? (int32_t)(unsigned)(b & 0xffffffffull) : -1;
    psim[n] = b ? __uint_as_float((unsigned)(b >> 32)) : 0.f;
  }
}

// ---- the tiles: blockIdx.y = row block - b0, blockIdx.x = column block - b0; below the diagonal a workgroup has nothing to do
__global__ __launch_bounds__(SM_NT) void dup_tile_kernel(int N, int H, const float* __restrict__ content, long ldc, int vec,
                                                         const float* __restrict__ r, int b0, float t, const int32_t* __restrict__ key,
                                                         int lo, int hi, int32_t* __restrict__ count, u64* __restrict__ best) {
  if (blockIdx.x < blockIdx.y) return;
  __shared__ __attribute__((aligned(16))) float xs[SM_T * SM_LD];        // the i rows of the chunk; behind the K loop cnt[128]
  __shared__ __attribute__((aligned(16))) float ys[SM_T * SM_LD];        // the j rows of the chunk; behind the K loop best[128]
  __shared__ int memb[2 * SM_T];                                         // slot s is a member (and a row of the table)
  const int tid = threadIdx.x, tn = tid & 15, tq = tid >> 4;
  const bool diag = blockIdx.x == blockIdx.y;
  const long i0 = ((long)b0 + blockIdx.y) * SM_T, j0 = ((long)b0 + blockIdx.x) * SM_T;

  // membership of the 128 rows of the tile; with a window a tile with no member on one side has no pair to offer
  int mine = 0;
  if (tid < 2 * SM_T) {
    const long n = tid < SM_T ? i0 + tid : j0 + tid - SM_T;
    if (n < N) mine = key ? (lo <= key[n] && key[n] < hi) : 1;
    memb[tid] = mine;
  }
  const int any_i = __syncthreads_or(tid < SM_T && mine);
  const int any_j = __syncthreads_or(tid >= SM_T && mine);
  if (!any_i || !any_j) return;

  const float* xrow[2];
  const float* yrow[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int row = sm_piece_row(tid, u);
    xrow[u] = i0 + row < N ? content + (i0 + row) * ldc : nullptr;
    yrow[u] = j0 + row < N ? content + (j0 + row) * ldc : nullptr;
  }
  float acc[SM_R][SM_R][8];
#pragma unroll
  for (int i = 0; i < SM_R; ++i)
#pragma unroll
    for (int m = 0; m < SM_R; ++m)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[i][m][j] = 0.f;
  float na = 0.f, nb = 0.f;
  sm_contract<false>(H, xrow, vec != 0, yrow, vec != 0, xs, ys, acc, na, nb);

  int* cnt = reinterpret_cast<int*>(xs);
  u64* bst = reinterpret_cast<u64*>(ys);
  if (tid < 2 * SM_T) {
    cnt[tid] = 0;
    bst[tid] = 0ull;
  }
  __syncthreads();

  float rj[SM_R];
  int okj[SM_R], cj[SM_R];
  u64 bj[SM_R];
#pragma unroll
  for (int m = 0; m < SM_R; ++m) {
    const int lj = tn + 16 * m;
    okj[m] = memb[SM_T + lj];
    rj[m] = okj[m] ? r[j0 + lj] : 0.f;                                    // (a member is a row of the table)
    cj[m] = 0;
    bj[m] = 0ull;
  }
#pragma unroll
  for (int i = 0; i < SM_R; ++i) {
    const int li = tq + 16 * i;
    if (!memb[li]) continue;
    const float ri = r[i0 + li];
    int ci = 0;
    u64 bi = 0ull;
#pragma unroll
    for (int m = 0; m < SM_R; ++m) {
      const int lj = tn + 16 * m;
      const float sim = sm_close(acc[i][m]) * (ri * rj[m]);
      if (okj[m] && (!diag || li < lj) && sim >= t) {                     // (NaN >= t is false)
        const u64 bits = (u64)__float_as_uint(sim) << 32;
        const u64 ki = bits | (u64)(unsigned)(j0 + lj), kj = bits | (u64)(unsigned)(i0 + li);
        ++ci;
        ++cj[m];
        bi = ki > bi ? ki : bi;
        bj[m] = kj > bj[m] ? kj : bj[m];
      }
    }
    if (ci) {
      atomicAdd(&cnt[li], ci);
      atomicMax(&bst[li], bi);
    }
  }
#pragma unroll
  for (int m = 0; m < SM_R; ++m)
    if (cj[m]) {
      atomicAdd(&cnt[SM_T + tn + 16 * m], cj[m]);
      atomicMax(&bst[SM_T + tn + 16 * m], bj[m]);
    }
  __syncthreads();
  if (tid < 2 * SM_T) {
    const int c = cnt[tid];
    if (c) {
      const long n = tid < SM_T ? i0 + tid : j0 + tid - SM_T;             // (c > 0: a member, so n < N)
      __hip_atomic_fetch_add(count + n, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_max(best + n, bst[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

bool dp_bad(const void* p, unsigned mask) { return !p || ((uintptr_t)p & mask); }
bool dp_bad_table(int N, int H, const float* t, int64_t ld) {
  return N < 1 || H < 1 || dp_bad(t, 3) || ld < H || (N > 1 && ld > (0x7fffffffffffL - H) / (N - 1));   // (N - 1) ld + H: an offset
}
bool dp_bad_threshold(float t) { return !(t > 0.f && t <= 1.f); }          // (NaN is neither)
inline int dp_blocks(int N) { return (int)(((int64_t)N + SM_T - 1) / SM_T); }
constexpr int DP_MAX_GRID_Y = 32768;                                       // row blocks per launch

}  // namespace

extern "C" int tcar_dupes_abi_version(void) { return TCAR_DUPES_ABI_VERSION; }

extern "C" int tcar_dup_rnorm(int N, int H, const float* content, int64_t ld_content, float* r, void* stream) {
  if (dp_bad_table(N, H, content, ld_content) || dp_bad(r, 3)) return TCAR_E_ARG;
  const dim3 grid((unsigned)(((int64_t)N + SM_NT / 8 - 1) / (SM_NT / 8))), block(SM_NT);
  TCAR_LAUNCH(dup_rnorm_kernel, grid, block, 0, (hipStream_t)stream, N, H, content, (long)ld_content, r);
  TCAR_CHECK_LAUNCH();
  return TCAR_OK;
}

extern "C" int tcar_dup_reset(int N, int32_t* count, uint64_t* best, void* stream) {
  if (N < 1 || dp_bad(count, 3) || dp_bad(best, 7)) return TCAR_E_ARG;
  const dim3 grid((unsigned)(((int64_t)N + SM_NT - 1) / SM_NT)), block(SM_NT);
  TCAR_LAUNCH(dup_reset_kernel, grid, block, 0, (hipStream_t)stream, N, count, reinterpret_cast<u64*>(best));
  TCAR_CHECK_LAUNCH();
  return TCAR_OK;
}

extern "C" int tcar_dup_tiles(int N, int H, const float* content, int64_t ld_content, const float* r, int b0, int b1, float t,
                              const int32_t* key, int lo, int hi, int32_t* count, uint64_t* best, void* stream) {
  if (dp_bad_table(N, H, content, ld_content) || dp_bad(r, 3) || dp_bad(count, 3) || dp_bad(best, 7)) return TCAR_E_ARG;
  if (b0 < 0 || b1 < b0 || b1 > dp_blocks(N) || dp_bad_threshold(t)) return TCAR_E_ARG;
  if (key ? ((uintptr_t)key & 3) != 0 : (lo != 0 || hi != 0)) return TCAR_E_ARG;
  if (b0 == b1) return TCAR_OK;
  const int vec = tcar_aligned16(content) && !(ld_content & 3);
  const int nb = dp_blocks(N);
  for (int y0 = b0; y0 < b1; y0 += DP_MAX_GRID_Y) {
    const int ny = b1 - y0 < DP_MAX_GRID_Y ? b1 - y0 : DP_MAX_GRID_Y;
    const dim3 grid((unsigned)(nb - y0), (unsigned)ny), block(SM_NT);
    TCAR_LAUNCH(dup_tile_kernel, grid, block, 0, (hipStream_t)stream, N, H, content, (long)ld_content, vec, r, y0, t, key, lo, hi, count,
                reinterpret_cast<u64*>(best));
    TCAR_CHECK_LAUNCH();
  }
  return TCAR_OK;
}

extern "C" int tcar_dup_finish(int N, const uint64_t* best, int32_t* partner, float* partner_sim, void* stream) {
  if (N < 1 || dp_bad(best, 7) || dp_bad(partner, 3) || dp_bad(partner_sim, 3)) return TCAR_E_ARG;
  const dim3 grid((unsigned)(((int64_t)N + SM_NT - 1) / SM_NT)), block(SM_NT);
  TCAR_LAUNCH(dup_finish_kernel, grid, block, 0, (hipStream_t)stream, N, reinterpret_cast<const u64*>(best), partner, partner_sim);
  TCAR_CHECK_LAUNCH();
  return TCAR_OK;
}

extern "C" int tcar_dupes_step(const tcar_ctx_t* c, const tcar_dupes_t* d, void* stream) {
  if (!c || !d || !c->E || d->stripe < 1) return TCAR_E_ARG;
  const int N = c->d.n_items, H = c->d.H, ldh = c->d.ldh;
  const int64_t ek = 2 * (int64_t)c->d.ldh + 5 * (int64_t)c->d.ldt;
  if (N < 1 || H < 1 || ldh < H) return TCAR_E_ARG;
  const float* content = c->E + ldh;
  // every argument is checked before the first launch: the four calls below repeat these tests and cannot fail on them
  if (dp_bad_table(N, H, content, ek) || dp_bad(d->r, 3) || dp_bad(d->count, 3) || dp_bad(d->best, 7) || dp_bad(d->partner, 3) ||
      dp_bad(d->partner_sim, 3) || dp_bad_threshold(d->t))
    return TCAR_E_ARG;
  if (d->key ? ((uintptr_t)d->key & 3) != 0 : (d->lo != 0 || d->hi != 0)) return TCAR_E_ARG;
  int rc = tcar_dup_rnorm(N, H, content, ek, d->r, stream);
  if (rc) return rc;
  if ((rc = tcar_dup_reset(N, d->count, d->best, stream))) return rc;
  const int nb = dp_blocks(N);
  for (int b0 = 0; b0 < nb;) {
    const int b1 = nb - b0 < d->stripe ? nb : b0 + d->stripe;
    if ((rc = tcar_dup_tiles(N, H, content, ek, d->r, b0, b1, d->t, d->key, d->lo, d->hi, d->count, d->best, stream))) return rc;
    b0 = b1;
  }
  return tcar_dup_finish(N, d->best, d->partner, d->partner_sim, stream);
}
