/* tcar_serve_shard.h — the streamed score-and-select of tcar_serve.h / tcar_window.h / tcar_quota.h on a catalog cut into SHARDS: every
 * shard folds its own rows into a select state per session, and S such states MERGE into the state of the whole catalog.
 *
 * The merge is exact.  A state is a sufficient statistic under the total list order (score descending, then item id descending):
 *   list    the k best of the union are among the k best of every part; capped: tcar_quota.h proves capped_k(A u B) =
 *           capped_k(capped_k(A) u B), and by symmetry capped_k(A u B) = capped_k(capped_k(A) u capped_k(B)) — the walk over the union
 *           of the parts' capped lists.  Scores are copied, never recomputed: topk and score are the bits a single state gives.
 *   count   strict-greater counts of disjoint parts add: rank is exact.
 *   softmax (max, sum exp) pairs combine as in the online fold, in ASCENDING SHARD ORDER, so the sum has one rounding order: the same
 *           bits on every run and on every rank; against a single state it differs by the rounding of a repartitioned sum.
 *
 * Contracts as in tcar_serve.h: TCAR_OK / TCAR_E_ARG / TCAR_E_LAUNCH, launch on `stream`, never synchronise, never allocate, argument
 * errors before anything is launched. */
#ifndef TCAR_SERVE_SHARD_H
#define TCAR_SERVE_SHARD_H

#include "tcar_quota.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TCAR_SERVE_SHARD_ABI_VERSION 1
int tcar_serve_shard_abi_version(void);

/* S states of B sessions each -> one.  states = shard 0's state of session 0; shard s's state of session b lies at
 * states + s*stride_words + b*(2k + 4) (4-byte words; stride_words >= B*(2k + 4) where S > 1, anything between two shards' rows is never
 * read).  out [B, 2k + 4]: a state in the layout of tcar_serve.h, read unchanged by tcar_select_finish; it overlaps no input.
 * 1 <= S <= 64, 1 <= k <= 64.  cat [N] with cap >= 1: the capped walk of tcar_quota.h over the S k input entries (cap >= k: the uncapped
 * merge, same bits); cat == NULL requires cap == 0.  All inputs were folded with the same k, exclusions, window, cat and cap.
 *   list   the k best of the input entries in list order (entries with index -1 do not exist); slots past the end hold -inf / -1
 *   count  the sum of the S counts
 *   (M, sum)  M = max_s m_s, sum = SUM over s ascending with m_s > -inf of sum_s * expf(m_s - M); a state that never folded a pooled
 *          column (m_s = -inf) adds nothing and produces no NaN; all of them empty: (-inf, 0) */
int tcar_select_merge(int B, int k, int S, const void* states, int64_t stride_words, void* out, const int32_t* cat, int cap, void* stream);

/* The shard's side of one evaluation / recommendation step (sharded.py: ShardExchange.serve), between the exchanges.  sc = the shard's
 * context (the `c` of tcar_shard_score: its candidate side covers rows [sh->n0, sh->n0 + sh->n_loc) of the catalog), sh = the shard
 * descriptor with att_all / ld_att = the Bq = world*cap gathered session rows and a16h / a16l = planes for ceil128(Bq) rows; of sh only
 * world, cap, n0, n_loc, att_all, ld_att, a16h and a16l are read.
 *
 * tcar_shard_serve_begin: rebuilds the shard's candidate-time planes where refresh_time says they are stale, splits att_all into the
 * attout planes, and — label [Bq] != NULL — writes lab_part [Bq]: attout[b] . E[label[b]] from the planes the panel GEMM reads (the
 * arithmetic of the unsharded step's label score, local row label[b] - n0) where this shard owns label[b], 0 where it does not;
 * label < 0 (a padding session) indexes nothing. */
int tcar_shard_serve_begin(const tcar_ctx_t* sc, const tcar_shard_t* sh, int refresh_time, const int32_t* label, float* lab_part,
                           void* stream);

/* tcar_shard_serve_fold: resets s->state [Bq, 2k + 4] and folds every panel of the shard's rows into it — the evaluation form of the
 * logits GEMM over the SHARD's planes into s->panel_buf [ceil-to-Bq rows, s->panel], then tcar_select_panel_quota with GLOBAL item ids
 * (n0 + local): label / lab_score [Bq] (both or neither; lab_score = the owners' label scores), s->excl [Bq, X], w->key / q->cat (full
 * length) keep their global meaning.  No finish: the states of all shards are merged first (tcar_select_merge).  s->topk, s->score,
 * s->rank, s->ce and s->lab_score are not used. */
int tcar_shard_serve_fold(const tcar_ctx_t* sc, const tcar_shard_t* sh, const int32_t* label, const float* lab_score,
                          const tcar_serve_t* s, const tcar_window_t* w, const tcar_quota_t* q, void* stream);

#ifdef __cplusplus
}
#endif
#endif
