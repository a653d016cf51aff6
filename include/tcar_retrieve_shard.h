/* tcar_retrieve_shard.h — retrieve-then-rank (tcar_retrieve.h, tcar_cand.h) on a catalog cut into SHARDS, the way tcar_serve_shard.h
 * carries the streamed score-and-select there: every shard folds its own rows into a top-C state per session and scores the shortlist
 * slots whose rows it owns; S such states MERGE into the state of the whole catalog, and S score parts COMBINE into the whole list's.
 *
 * Both joins are exact.
 *   merge    a retrieve state is a sufficient statistic under the total list order (score descending, then item id descending), and
 *            the shards' item ids are disjoint: the C best of the union are the C best of the shards' C bests.  Entries are compared
 *            and copied, never recomputed; there is no float sum, so the result is the same bits for every shard order.
 *   combine  every slot's row lives on exactly one shard, and the summation order of a dot of tcar_cand_scores depends on K and nsplit
 *            alone: the owner's score is bit for bit what a whole-catalog engine computes from the same operands.  The combine copies
 *            the owner's bits — a NaN or a -0.0 survives as it is; there is no max and no sum over the parts.
 *
 * Contracts as in tcar_serve.h: TCAR_OK / TCAR_E_ARG / TCAR_E_LAUNCH, launch on `stream`, never synchronise, never allocate, argument
 * errors before anything is launched. */
#ifndef TCAR_RETRIEVE_SHARD_H
#define TCAR_RETRIEVE_SHARD_H

#include "tcar_retrieve.h"
#include "tcar_serve_shard.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TCAR_RETRIEVE_SHARD_ABI_VERSION 1
int tcar_retrieve_shard_abi_version(void);

/* S retrieve states of B sessions each -> one.  Addressing as tcar_select_merge: states = shard 0's state of session 0; shard s's
 * state of session b lies at states + s*stride_words + b*(2C + 4) (4-byte words; stride_words >= B*(2C + 4) where S > 1, anything
 * between two shards' rows is never read).  out [B, 2C + 4]: a state in the layout of tcar_retrieve.h; it overlaps no input.
 * 1 <= S <= 64, 1 <= C <= 1024.  All inputs were folded with the same C, exclusions and window, over disjoint items.
 * out holds the C best entries of the union in list order (-inf / -1 behind the last), `held` and the threshold words are what ONE
 * fold of the whole catalog would have left: tcar_retrieve_finish reads it unchanged and a further tcar_retrieve_panel may be folded
 * into it.  A shard that holds nothing, and one whose best entry does not beat the C-th entry held so far, costs one read. */
int tcar_retrieve_merge(int B, int C, int S, const void* states, int64_t stride_words, void* out, void* stream);

/* tcar_retrieve_panel with a liveness word per session: the workgroup of a session with live[b] < 0 returns at once and its state
 * stays as it was (as reset: an empty list).  live == NULL: tcar_retrieve_panel.  A padding session of a gathered batch has an
 * all-zero score row, which under "score, then id descending" admits EVERY item of a catalog streamed in ascending id — the
 * selector's worst case; it must cost nothing. */
int tcar_retrieve_panel_live(int B, int n0, int n, const float* panel, int64_t ld, int C, const int32_t* excl, int X, const int32_t* key,
                             const int32_t* lo, const int32_t* hi, void* state, const int32_t* live /* [B] or NULL */, void* stream);

/* The shard's side of a retrieval, after tcar_shard_serve_begin (label NULL: it rebuilds stale time planes and splits the gathered
 * attout rows).  sc, sh as tcar_shard_serve_fold takes them; Bq = world*cap gathered sessions.  Resets d->state [Bq, 2C + 4]
 * (d->state_bytes >= tcar_retrieve_state_bytes(Bq, C)) and folds every panel of the shard's rows into it: the evaluation form of the
 * logits GEMM in the COARSE precision of tcar_retrieve_step (the hi planes alone) into d->panel_buf [ceil-to-Bq rows, d->panel], then
 * tcar_retrieve_panel_live with GLOBAL item ids (sh->n0 + local); d->excl [Bq, X] and d->window (key over the WHOLE catalog) keep their
 * global meaning.  live [Bq] or NULL.  No finish: the shards' states are merged first; d->ids and d->scores are not used. */
int tcar_shard_retrieve_fold(const tcar_ctx_t* sc, const tcar_shard_t* sh, const tcar_retrieve_t* d, const int32_t* live, void* stream);

/* tcar_cand_scores for operands that cover the catalog rows [id0, id0 + N) only: a slot with id i reads local row i - id0 iff
 * (unsigned)(i - id0) < N, else it reads nothing and scores -inf.  id0 >= 0, id0 + N <= 2^31 - 1.  For an owned slot the score is the
 * bits tcar_cand_scores gives on the whole catalog's operands; id0 = 0 is tcar_cand_scores. */
int tcar_cand_scores_owned(int B, int C, int N, int K, const float* att, int64_t ld_att, const float* E, int64_t ldE, const void* a_hi,
                           const void* a_lo, int64_t a_inner, const void* e_hi, const void* e_lo, int64_t e_inner, int nsplit,
                           const int32_t* cand, int64_t ld_cand, float* out, int64_t ld_out, int id0, void* stream);

/* The shard's side of candidate scoring over the Bq = world*cap gathered sessions, after tcar_shard_serve_begin: part[b, c] = the exact
 * score (the precision of sc->scoring, split-bf16 only) of slot cand[b, c] where this shard owns the row, -inf elsewhere.
 * cand int32 [Bq, ld_cand >= C] GLOBAL ids; part fp32 [Bq, ld_part >= C]; 1 <= C <= 1024. */
int tcar_shard_cand_scores(const tcar_ctx_t* sc, const tcar_shard_t* sh, int C, const int32_t* cand, int64_t ld_cand, float* part,
                           int64_t ld_part, void* stream);

/* out[b, c] = parts[owner][b, c] with owner = cand[b, c] / rows_per_shard for ids in [0, N) whose owner is < S, -inf otherwise.
 * parts: shard s's [B, C] part (dense rows of C floats) at parts + s*stride (floats; stride >= B*C where S > 1); cand int32
 * [B, ld_cand >= C]; out fp32 [B, ld_out >= C], columns >= C are never written, it overlaps no input.  1 <= S <= 64,
 * 1 <= C <= 1024, rows_per_shard >= 1, N >= 1. */
int tcar_cand_combine(int B, int C, int S, int rows_per_shard, int N, const int32_t* cand, int64_t ld_cand, const float* parts,
                      int64_t stride, float* out, int64_t ld_out, void* stream);

/* The closing launch of a two-stage call, which tcar_retrieve_rerank_step runs itself and a sharded call runs behind the combine:
 * topk[b, j] = ids[b, order[b, j]] and score[b, j] = cand_score[b, order[b, j]] for the first k ranks of every list (ids, cand_score,
 * order [B, C]; order: tcar_cand_rank's); -1 / untouched behind a list's end.  1 <= k <= 64, k <= C; score may be NULL. */
int tcar_rerank_take(int B, int C, int k, const int32_t* ids, const float* cand_score, const int32_t* order, int32_t* topk, float* score,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif
