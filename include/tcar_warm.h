/* tcar_warm.h — warm start: the item rows of U COLD catalog rows (articles published into a live context, whose item row is an
 * untrained draw or the row of a retired article) from the trained item rows of their content neighbours, computed on the device and
 * installed in place.  The model scores a candidate as attout_ic . [item row | content] + attout_t . time: without this call half of
 * the item / content block of a new article is noise.  Three existing layers and one new kernel: the neighbour lists are those of
 * tcar_similar.h, the rows go in through tcar_catalog.h, and tcar_rows_blend sits between them.
 *
 * THE RULE.  For cold row u take its neighbour list (n_j, s_j), j = 0 .. k - 1, 1 <= k <= 64: exactly what tcar_similar_step returns
 * for the query "catalog id ids[u]" — content read from the columns of E in place, the list order of tcar_serve.h — with EVERY id the
 * call names excluded (cold rows do not donate to each other, and a row is not its own donor); the caller's exclusion lists and
 * windows apply on top.  Then, all in fp32:
 *   w_j        = s_j  where n_j >= 0 (and < N), s_j > 0 and s_j >= min_sim;  0 otherwise (a NaN s_j gives 0).  0 <= min_sim <= 1
 *   W          = sum_j w_j, added with j ascending from +0
 *   support[u] = #{j : w_j > 0},   wsum[u] = W
 *   row[c]     = acc_c / W, acc_c the fma chain acc = fmaf(w_j, x_{n_j}[c], acc) over the j with w_j > 0, j ascending, from +0; x_n is
 *                the item row E[n, 0:H], read in place and unclipped, as the scoring GEMM reads it.  The division is correctly rounded
 *   support[u] == 0:  row = +0 in every column and wsum[u] = +0 (a zero row adds nothing to a logit; a stale one adds noise)
 * A slot with w_j = 0 takes no part: its row is not read.  No sum depends on an arrival order and no float atomics are used, so the
 * result is the same bits on every run, for every U and for every `panel`.  Against exact arithmetic over the same (n_j, s_j):
 * |row[c] - exact[c]| <= (2 k + 2) 2^-24 max_j |x_{n_j}[c]| over the donors with w_j > 0 (k fmas, a k-term sum, one division).
 *
 * Contracts as in tcar_serve.h: TCAR_OK / TCAR_E_ARG / TCAR_E_LAUNCH, launch on `stream`, never synchronise, never allocate, argument
 * errors before anything is launched, no mutable global state.  U == 0 is TCAR_OK with nothing launched. */
#ifndef TCAR_WARM_H
#define TCAR_WARM_H

#include "tcar_catalog.h"
#include "tcar_similar.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TCAR_WARM_ABI_VERSION 1
int tcar_warm_abi_version(void);

/* The blend alone, over any table: out[u, :] = the row of the rule for the list (nbr[u, :], sim[u, :]).
 *   nbr      int32 [U, k] device, sim fp32 [U, k] device (dense, k <= 64): the lists.  A slot with nbr < 0 or nbr >= N is empty
 *   table    fp32, row n at table + n * ld_table (ld_table >= H), N rows; only the rows of donors with w_j > 0 are read, and of those
 *            only the columns < H
 *   out      fp32, row u at out + u * ld_out (ld_out >= H); must not overlap the rows of `table`
 *   support  int32 [U], wsum fp32 [U]
 * Where table and out are 16-byte aligned and ld_table % 4 == ld_out % 4 == 0, loads and stores are 16 bytes per lane and the pad
 * columns [H, ld_out) of every out row are written as +0; otherwise everything is scalar and only the columns < H of out are written.
 * One wave per row, four rows per 256-thread workgroup; rows >= U are not touched.
 * Argument errors: U < 0; k outside [1, 64]; N < 1; H < 1; a NULL or misaligned (4 bytes) pointer; ld < H; min_sim outside [0, 1]
 * (NaN included); out overlapping table. */
int tcar_rows_blend(int U, int k, int N, int H, const int32_t* nbr, const float* sim, float min_sim, const float* table,
                    int64_t ld_table, float* out, int64_t ld_out, int32_t* support, float* wsum, void* stream);

/* one warm start */
typedef struct {
  int32_t U;                        /* cold rows named by this call */
  const int32_t* ids;               /* [U] device, 0-based, each in [0, N), pairwise distinct (not checked here): the queries AND the rows written */
  float min_sim;                    /* in [0, 1] */
  float* xq;                        /* [U, ldh of the context] workspace of tcar_similar_t */
  float* rq;                        /* [U] workspace of tcar_similar_t */
  const tcar_serve_t* serve;        /* as tcar_similar_step takes it: k <= 64, panel, panel_buf [U, panel], state, state_bytes, excl [U, X],
                                       topk [U, k] and score [U, k] — both REQUIRED here: they are the donor lists the blend reads.  excl must
                                       name every id of `ids` in every row (the caller builds it; X >= U is checked, the contents are not) */
  const tcar_window_t* window;      /* one window per cold row, or NULL */
  float* rows;                      /* [U, ld_rows] staging, 16-byte aligned: receives the blended rows (columns >= H zero) */
  int64_t ld_rows;                  /* >= H, % 4 == 0 */
  int32_t* support;                 /* [U] */
  float* wsum;                      /* [U] */
  int32_t zero_moments;             /* as tcar_catalog_update_t: != 0 clears the Mi / Vi rows of the U items (a published call passes 1) */
} tcar_warm_t;

/* tcar_similar_step with Q = U queries by id -> tcar_rows_blend from the item block of E (ld = ek) into `rows` -> tcar_catalog_update
 * with `rows` as item: afterwards every buffer of the context holds, for the named rows, the bytes of a context built from tables
 * whose item rows are `rows` (tcar_catalog.h).  An empty score slot of the lists is not written by the finish: the caller zeroes
 * serve->score if it reads it.  The context covers the whole catalog (no shard).  Every argument error of the three calls is raised
 * before the first launch. */
int tcar_warm_step(const tcar_ctx_t* c, const tcar_warm_t* w, void* stream);

#ifdef __cplusplus
}
#endif
#endif
