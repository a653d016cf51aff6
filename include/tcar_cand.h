/* tcar_cand.h — candidate-list scoring on top of the C ABI of tcar_hip.h: every session b names C candidate items, cand[b, 0 .. C),
 * and only those catalog rows are read.  Two uses: re-ranking a retrieved list (the second stage of retrieve-then-rank) and
 * impression-based evaluation (AUC / MRR / nDCG@5 / nDCG@10 over an impression's candidates, or a label among sampled negatives).
 * No [B, N] score matrix exists and no panel is streamed: the cost follows B C, not N.
 *
 * A SLOT is one entry of a list.  A slot whose id lies outside [0, N) is EMPTY (-1 by convention): it reads no row and scores -inf.
 * tcar_cand_rank, which is given no N, takes a slot as empty iff its id is negative or its score is -inf — what tcar_cand_scores
 * wrote for every id outside the catalog.  Repeats of one id are allowed; each is a slot of its own.
 *
 * Order of a list (its non-empty slots): score descending, then item id descending — the list order of tcar_serve.h — then slot
 * ascending, which only repeats of one id reach.  It is a total order over the slots, so ranks are a permutation and every run gives
 * the same bits.
 *
 * Contracts as in tcar_serve.h: TCAR_OK / TCAR_E_ARG / TCAR_E_LAUNCH, launch on `stream`, never synchronise, never allocate, argument
 * errors before anything is launched. */
#ifndef TCAR_CAND_H
#define TCAR_CAND_H

#include "tcar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TCAR_CAND_ABI_VERSION 1
int tcar_cand_abi_version(void);

/* out[b, c] = attout[b] . E[cand[b, c]] over K columns (1 <= C <= 1024, K % 4 == 0), -inf for an empty slot.  Operands as the panel
 * GEMM of tcar_serve.h reads them: a_hi == NULL: the fp32 matrices att [B, ld_att] and E [N, ldE] (16-byte aligned, ld % 4 == 0,
 * ld >= K); else the KB32 planes of the B session rows (a_hi / a_lo, a_inner columns) and of the N catalog rows (e_hi / e_lo,
 * e_inner columns), inner % 32 == 0 and >= K; nsplit 1: hi hi only, nsplit 3: hi hi + hi lo + lo hi.  Columns >= K of a plane are
 * never read as scores.  cand: int32 [B, ld_cand >= C]; out: fp32 [B, ld_out >= C], columns >= C are never written.
 * The summation order of one dot depends on K and nsplit alone: the score of an item is the same bits in every slot, for every C, B
 * and whatever else the list holds. */
int tcar_cand_scores(int B, int C, int N, int K, const float* att, int64_t ld_att, const float* E, int64_t ldE, const void* a_hi,
                     const void* a_lo, int64_t a_inner, const void* e_hi, const void* e_lo, int64_t e_inner, int nsplit,
                     const int32_t* cand, int64_t ld_cand, float* out, int64_t ld_out, void* stream);

/* The list order of every session's slots and the impression metrics.  score fp32 [B, ld_score >= C], cand int32 [B, ld_cand >= C].
 *   rank_of [B, C] int32 or NULL: the 1-based rank of every slot, 0 for an empty one
 *   order   [B, C] int32 or NULL: order[b, r - 1] = the slot with rank r, -1 behind the last
 *   clicked [B, ld_clicked >= C] int32 0 / 1 or NULL (then counts and metrics must be NULL); over the non-empty slots:
 *   counts  [B, 3] int32 or NULL: (npos, nneg, auc2), auc2 = sum over (positive p, negative n) of 2 [s_p > s_n] + [s_p == s_n] — scores
 *           alone are compared, ties count half: ROC AUC = auc2 / (2 npos nneg), divided by the host
 *   metrics [B, 3] fp32 or NULL: (mrr, ndcg5, ndcg10); mrr = (sum over positives of 1 / rank) / npos, ndcg_k = sum over positives
 *           of rank <= k of 1 / log2(1 + rank), over the same sum for ranks 1 .. min(npos, k); all 0 when npos == 0.  The sums run
 *           in an order the code fixes. */
int tcar_cand_rank(int B, int C, const float* score, int64_t ld_score, const int32_t* cand, int64_t ld_cand, const int32_t* clicked,
                   int64_t ld_clicked, int32_t* rank_of, int32_t* order, int32_t* counts, float* metrics, void* stream);

/* One candidate-scoring step. */
typedef struct {
  int32_t C;                        /* slots per session, 1 .. 1024 */
  const int32_t* cand;              /* [B, ld_cand] 0-based item ids; outside [0, N): an empty slot */
  int64_t ld_cand;                  /* >= C; the row stride of cand AND of clicked */
  const int32_t* clicked;           /* [B, ld_cand] 0 / 1, or NULL (then counts and metrics are NULL) */
  float* score;                     /* [B, C] */
  int32_t* rank_of; int32_t* order; /* [B, C] each, or NULL */
  int32_t* counts; float* metrics;  /* [B, 3] each, or NULL */
} tcar_cand_t;

/* session forward (+ candidate-time refresh) exactly as tcar_serve_step runs it, then tcar_cand_scores from the context's operands
 * (fp32 or planes, by c->scoring) and, when any of rank_of / order / counts / metrics is asked for, tcar_cand_rank.  bt->label,
 * bt->neg and c->logits are neither needed nor touched.  The context covers the whole catalog (no shard). */
int tcar_cand_step(const tcar_ctx_t* c, const tcar_batch_t* bt, int refresh_time, const tcar_cand_t* d, void* stream);

#ifdef __cplusplus
}
#endif
#endif
