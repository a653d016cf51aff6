/* tcar_retrieve.h — the FIRST stage of retrieve-then-rank on top of the C ABI of tcar_hip.h: a streamed top-C selector, 1 <= C <= 1024,
 * that keeps a shortlist of C (score, item) entries per session while the catalog's scores stream by in column panels, and the two
 * steps built on it: tcar_retrieve_step (a shortlist from COARSE scores) and tcar_retrieve_rerank_step (the shortlist re-scored
 * exactly by tcar_cand_scores of tcar_cand.h and cut to its k best).  No [B, N] score matrix exists at any time.
 *
 * Order of a list: the library's one list order (tcar_serve.h; key_gt of csrc/topk_rows.h): score descending, then item id descending.
 * +0.0 and -0.0 are EQUAL scores (the id decides), as every float comparison has it; the score a list reports keeps its own bits.
 * It is a TOTAL order over the items, and a fold keeps the exact C best of (state entries + panel columns) under it: the result is the
 * same bits for every partition of the catalog into panels and on every run, whatever order survivors land in LDS.  No float sum
 * exists in the selector, so there is no summation order to fix.
 *
 * Eligibility: an item in an exclusion list of its session, an item outside the session's window and an item whose score is NaN is
 * never admitted.  There is no label, no count and no softmax: retrieval has no rank and no cross entropy.
 *
 * Cost: an element is ADMITTED when it beats the session's current threshold (the C-th best so far; "nothing" until C entries are
 * held); admitted elements are appended to an LDS buffer that is pruned — sorted, cut to the best C, threshold raised — when it is
 * full and at the end of every panel.  For items in an order unrelated to their scores about C (1 + ln(n / C)) of n items are
 * admitted: a few prunes per panel.  A catalog sorted by ASCENDING score admits every item and prunes every C items or so: that
 * case is exact like every other, and slow.
 *
 * Contracts as in tcar_serve.h: TCAR_OK / TCAR_E_ARG / TCAR_E_LAUNCH, launch on `stream`, never synchronise, never allocate, argument
 * errors before anything is launched, no mutable global state. */
#ifndef TCAR_RETRIEVE_H
#define TCAR_RETRIEVE_H

#include "tcar_cand.h"
#include "tcar_window.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TCAR_RETRIEVE_ABI_VERSION 1
int tcar_retrieve_abi_version(void);

/* running per-session state, 2 C + 4 words: score[C] | id[C] (-1: empty), kept in list order | entries held | the admission threshold
 * (the sortable key of the C-th entry, two words; 0 = "nothing" while fewer than C are held) | pad.  -1 for a B or C out of range. */
int64_t tcar_retrieve_state_bytes(int B, int C);                     /* 1 <= C <= 1024 */
int tcar_retrieve_reset(int B, int C, void* state, void* stream);

/* fold the score columns [n0, n0 + n) of every session into the state.  panel, ld, n as tcar_select_panel takes them: fp32, row b at
 * panel + b*ld, column j = item n0 + j, n <= 49,152, ld % 4 == 0 and >= n, 16-byte aligned rows; columns >= n are never read as scores.
 * Every item is folded ONCE between a reset and a finish, with the same C, excl and window in every call.
 *   excl [B, X] or NULL        -> 0-based item ids (-1 = empty slot, repeats allowed) that never enter session b's list
 *   key [N], lo [B], hi [B]    -> all three or none (tcar_window.h): item n0 + j is eligible iff lo[b] <= key[n0 + j] < hi[b] */
int tcar_retrieve_panel(int B, int n0, int n, const float* panel, int64_t ld, int C, const int32_t* excl, int X, const int32_t* key,
                        const int32_t* lo, const int32_t* hi, void* state, void* stream);

/* ids [B, C] in list order, -1 behind the last eligible item; scores [B, C] or NULL: the folded fp32 score of each entry bit for bit,
 * -inf where ids is -1 — the empty slot of tcar_cand.h, so (ids, C) is a valid `cand` of tcar_cand_scores / tcar_cand_rank. */
int tcar_retrieve_finish(int B, int C, const void* state, int32_t* ids, float* scores, void* stream);

/* One retrieval step without the [B, N] logits. */
typedef struct {
  int32_t C, panel;                 /* C: 1 .. 1024; panel: columns per panel, % 128 == 0, <= 49,152 */
  float* panel_buf;                 /* [ceil-to-B rows, panel] fp32 */
  void* state; int64_t state_bytes; /* >= tcar_retrieve_state_bytes(B, C) */
  const int32_t* excl; int32_t X;   /* optional exclusion lists [B, X] */
  int32_t* ids; float* scores;      /* [B, C]; scores may be NULL */
  const tcar_window_t* window;      /* optional: every fold windowed (key [N] over the context's whole catalog); NULL: no window */
} tcar_retrieve_t;

/* session forward (+ candidate-time refresh) exactly as tcar_serve_step runs it, then for every panel: the evaluation form of the
 * logits GEMM in the COARSE precision into panel_buf -> tcar_retrieve_panel; tcar_retrieve_finish.  Coarse precision:
 *   c->scoring != 0 (any split-bf16 engine): the hi planes alone (nsplit = 1 over a16h / e16h) — one MFMA per product instead of
 *                   three, half of the plane bytes, about 2^-8 relative per operand; the lo planes are never read
 *   c->scoring == 0 (the fp32 engine): the fp32 GEMM — that engine has no cheaper operands, so its shortlist is exact in fp32
 * bt->label, bt->neg and c->logits are neither needed nor touched.  The context covers the whole catalog (no shard). */
int tcar_retrieve_step(const tcar_ctx_t* c, const tcar_batch_t* bt, int refresh_time, const tcar_retrieve_t* d, void* stream);

/* The second stage of the two-stage call: workspaces [B, C] and the list it returns. */
typedef struct {
  int32_t k;                        /* 1 .. 64 and <= C of the retrieve descriptor */
  float* cand_score;                /* [B, C]: the exact score of every shortlist slot (-inf for an empty one) */
  int32_t* rank_of; int32_t* order; /* [B, C] each: tcar_cand_rank's outputs over the shortlist */
  int32_t* topk; float* score;      /* [B, k]: the k best of the shortlist in list order; -1 / untouched behind the last; score may be NULL */
} tcar_rerank_t;

/* Two-stage recommendation with ONE session forward: tcar_retrieve_step, then tcar_cand_scores over the shortlist d->ids from the
 * context's own operands (the exact precision of c->scoring, as tcar_cand_step calls it), tcar_cand_rank for r->order, and the first
 * k slots of the order as (topk, score).  By construction the list is the top k, under the list order, of tcar_cand_scores over
 * the shortlist. */
int tcar_retrieve_rerank_step(const tcar_ctx_t* c, const tcar_batch_t* bt, int refresh_time, const tcar_retrieve_t* d,
                              const tcar_rerank_t* r, void* stream);

#ifdef __cplusplus
}
#endif
#endif
