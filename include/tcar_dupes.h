/* tcar_dupes.h — the duplicate audit: for EVERY item of the catalog, how many other items have content that is at least as similar
 * as a threshold, and which of them is the most similar.  One triangular pass over all pairs of rows of the frozen fp32 content table,
 * read in place (E[:, ldh : ldh + H] of a context): every cosine is computed once, no [N, N] or [Q, panel] block is written, and there
 * is no list of pairs — three numbers per item.
 *
 *   sim      THE similarity of the library, tcar_mmr.h / tcar_similar.h: sim(i, j) = (x_i . x_j) * (r_i * r_j), the dot in eight fma
 *            chains closed as there, r = 1 / sqrt(x . x) (0 for an all-zero row).  Bit for bit what tcar_sim_panel writes for the pair,
 *            and sim(i, j) == sim(j, i).
 *   t        the threshold, 0 < t <= 1.
 *   M        the member set: every item, or with a window (key != NULL) the items n with lo <= key[n] < hi (key: the int32 keys of
 *            tcar_window.h; lo >= hi is an empty set, not an error).
 *   count    int32 [N]: count[i] = the number of j in M, j != i, with sim(i, j) >= t; 0 for i outside M.
 *   partner  int32 [N]: the first such j in the list order of tcar_serve.h (sim descending, then item id descending); -1 where
 *            count[i] == 0.
 *   partner_sim  fp32 [N]: sim(i, partner[i]); +0 where there is no partner.
 * A NaN similarity (non-finite content) is never >= t; an all-zero row scores +0 against everything and is never flagged.
 *
 * All three are order-independent reductions — an integer sum, and the maximum of the unsigned 64-bit key
 * (float bits of sim) << 32 | id, which is monotone in the list order because sim >= t > 0 — so they are the same bits on every run
 * and for every partition of the row blocks into calls of tcar_dup_tiles.  No float is summed across pairs, nothing has a capacity.
 * A caller who wants ALL partners of a flagged row asks tcar_similar_step for them: the audit says where to look.
 *
 * Contracts as in tcar_similar.h: TCAR_OK / TCAR_E_ARG / TCAR_E_LAUNCH, launch on `stream`, never synchronise, never allocate, argument
 * errors before anything is launched, no mutable global state.  Every table pointer is 4-byte aligned (best: 8-byte); content, row n
 * at content + n * ld_content (ld_content >= H), need not be 16-byte aligned (the kernels then load scalars).  N >= 1, H >= 1,
 * (N - 1) * ld_content + H < 2^47 (the offset of the last float read; checked without overflow). */
#ifndef TCAR_DUPES_H
#define TCAR_DUPES_H

#include "tcar_similar.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TCAR_DUPES_ABI_VERSION 1
int tcar_dupes_abi_version(void);

/* r[n] = 1 / sqrt(x_n . x_n) for every row n < N of content, 0 for an all-zero row: the rq tcar_sim_queries writes for qid = n. */
int tcar_dup_rnorm(int N, int H, const float* content, int64_t ld_content, float* r, void* stream);

/* The state of an audit, zeroed: count int32 [N], best 64-bit [N] (the packed keys; 0 = no partner). */
int tcar_dup_reset(int N, int32_t* count, uint64_t* best, void* stream);

/* The row blocks [b0, b1) of 64 rows (block b: rows 64 b .. 64 b + 63; 0 <= b0 <= b1 <= ceil(N / 64)) against every column block >=
 * the row block: every pair (i, j), i < j, i in those rows, is met exactly once, and an admitted pair adds to BOTH of its items.  A
 * whole audit is any set of calls whose [b0, b1) partition [0, ceil(N / 64)), between one tcar_dup_reset and tcar_dup_finish.
 *   r        fp32 [N]: what tcar_dup_rnorm wrote for this table
 *   key      int32 [N] or NULL.  NULL: every item is a member, and lo == hi == 0 (a window without its keys is TCAR_E_ARG)
 * b0 == b1 with good arguments returns TCAR_OK and launches nothing. */
int tcar_dup_tiles(int N, int H, const float* content, int64_t ld_content, const float* r, int b0, int b1, float t, const int32_t* key,
                   int lo, int hi, int32_t* count, uint64_t* best, void* stream);

/* partner[n] and partner_sim[n] from best[n], n < N: (-1, +0) where best[n] == 0. */
int tcar_dup_finish(int N, const uint64_t* best, int32_t* partner, float* partner_sim, void* stream);

/* one audit */
typedef struct {
  float t;                          /* the threshold, 0 < t <= 1 */
  int stripe;                       /* row blocks per tcar_dup_tiles launch, >= 1: any value gives the same bits */
  const int32_t* key;               /* [N] or NULL (then lo == hi == 0) */
  int lo, hi;                       /* the members: lo <= key < hi */
  float* r;                         /* [N] workspace */
  int32_t* count;                   /* [N] */
  uint64_t* best;                   /* [N] workspace */
  int32_t* partner;                 /* [N] */
  float* partner_sim;               /* [N] */
} tcar_dupes_t;

/* One audit over the context's content table (E + ldh, ld = ek, H columns, N rows): tcar_dup_rnorm, tcar_dup_reset, tcar_dup_tiles per
 * stripe of d->stripe row blocks, tcar_dup_finish.  The context covers the whole catalog (no shard); of *c only d and E are read. */
int tcar_dupes_step(const tcar_ctx_t* c, const tcar_dupes_t* d, void* stream);

#ifdef __cplusplus
}
#endif
#endif
