/* tcar_similar.h — related items: for Q QUERY rows of content, the k catalog items whose content is most similar, streamed.  There is
 * no session and no model in this call: the score of item n for query q is the cosine of two rows of the frozen fp32 content table,
 * read in place (E[:, ldh : ldh + H] of a context), so a row replaced by tcar_catalog_update is found under its new content by the
 * next call; no derived table exists.  The catalog is scored in column panels and every panel is folded by the folds of
 * tcar_serve.h / tcar_window.h / tcar_quota.h, unchanged: no [Q, N] matrix exists at any time, and windows, exclusion lists and
 * per-category caps mean what they mean there.
 *
 *   sim      THE similarity of the library, tcar_mmr.h: sim(x, y) = (x . y) * (r_x * r_y), r = 1 / sqrt(x . x) with correctly rounded
 *            sqrt and division, r = 0 for an all-zero row.  All fp32.  Every dot, the two x . x included, is eight fma chains — chain j
 *            takes the columns c with c % 8 == j in ascending order, starting from +0; columns past H add nothing — closed as
 *            ((c0 + c1) + (c2 + c3)) + ((c4 + c5) + (c6 + c7)): the order of csrc/mmr.hip.  The bits of sim depend on the two rows and
 *            on H alone — not on Q, the query's place in the batch, the panel width or n0 —, so sim(i, j) == sim(j, i), a query given
 *            by id and the same row given as a vector score the same bits, and a related list agrees with what tcar_mmr_walk reports
 *            for the same pair.  An all-zero row scores +0 against every finite row; non-finite content gives NaN, which no fold
 *            admits.
 *   lists    the list order of tcar_serve.h: sim descending, then item id descending; -1 where fewer than k items are eligible.
 *
 * Contracts as in tcar_serve.h: TCAR_OK / TCAR_E_ARG / TCAR_E_LAUNCH, launch on `stream`, never synchronise, never allocate, argument
 * errors before anything is launched, no mutable global state. */
#ifndef TCAR_SIMILAR_H
#define TCAR_SIMILAR_H

#include "tcar_quota.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TCAR_SIMILAR_ABI_VERSION 1
int tcar_similar_abi_version(void);

/* The prologue: the query rows and their r.  Exactly ONE of qid and qrow is given (the other NULL):
 *   qid      int32 [Q] device: 0-based rows of the table.  An id outside [0, N) (-1 is the empty query) gives a zero row and rq = 0
 *   qrow     fp32 [Q, ld_qrow >= H] device: rows that are in no table (drafts); ld_qrow is ignored with qid
 *   content  fp32, row n at content + n * ld_content (ld_content >= H): pass E + ldh with ld_content = ek for a context's table.
 *            Read with qid only, and then only the rows qid names; may be NULL with qrow
 *   xq       fp32 [Q, ld_xq >= H]: receives the query rows (columns >= H are not written);  rq fp32 [Q]: receives their r
 * N >= 1, H >= 1, Q >= 0; Q == 0 with good arguments launches nothing. */
int tcar_sim_queries(int Q, int N, int H, const float* content, int64_t ld_content, const int32_t* qid, const float* qrow, int64_t ld_qrow,
                     float* xq, int64_t ld_xq, float* rq, void* stream);

/* panel[q, j] = sim(query q, item n0 + j) for q < Q, j < n: the shape the folds read — fp32, row q at panel + q * ld, ld % 4 == 0,
 * ld >= n, 16-byte aligned rows, n <= 49,152.  Columns >= n are not written.  Rows of content outside [n0, n0 + n) and columns >= H
 * of any row are not read.  Each item's r is computed in the kernel from the tile it loads anyway.  content and xq need not be
 * 16-byte aligned (4-byte aligned; the kernel then loads scalars).  H >= 1, n0 >= 0; Q == 0 or n == 0 with good arguments returns
 * TCAR_OK and launches nothing.  (xq, rq): what tcar_sim_queries wrote. */
int tcar_sim_panel(int Q, int n0, int n, int H, const float* content, int64_t ld_content, const float* xq, int64_t ld_xq, const float* rq,
                   float* panel, int64_t ld, void* stream);

/* the queries of one related-items step */
typedef struct {
  const int32_t* qid;               /* [Q] or NULL */
  const float* qrow;                /* [Q, ld_qrow] or NULL: exactly one of the two */
  int64_t ld_qrow;
  float* xq;                        /* [Q, ldh of the context] workspace: the query rows */
  float* rq;                        /* [Q] workspace */
} tcar_similar_t;

/* One related-items step over the context's content table (E + ldh, ld = ek, H columns, N rows): tcar_sim_queries once,
 * tcar_select_reset, then for every panel tcar_sim_panel into s->panel_buf -> the unlabelled tcar_select_panel_quota; tcar_select_finish
 * into (s->topk, s->score).  Of *s: k <= 64, panel, panel_buf [Q, panel], state, state_bytes, excl [Q, X], topk, score; its lab_score,
 * rank and ce are unused.  w / quota optional (NULL), as tcar_serve_step_quota takes them, one window per QUERY.  No session forward,
 * no time refresh, no batch.  The context covers the whole catalog (no shard).  The list of a query whose id is outside [0, N) is
 * the list of a zero row (every sim +0); the caller knows its ids. */
int tcar_similar_step(const tcar_ctx_t* c, int Q, const tcar_similar_t* q, const tcar_serve_t* s, const tcar_window_t* w,
                      const tcar_quota_t* quota, void* stream);

#ifdef __cplusplus
}
#endif
#endif
