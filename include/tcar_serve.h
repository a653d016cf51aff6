/* tcar_serve.h — streamed score-and-select on top of the C ABI of tcar_hip.h: the catalog is scored in column panels and every
 * panel is folded into a small per-session running state (top-k list, strict-greater count, online softmax).  No [B, N] score
 * matrix exists at any time; the label is optional (recommendation).  All functions return TCAR_OK / TCAR_E_ARG / TCAR_E_LAUNCH,
 * launch on `stream`, never synchronise and never allocate.  Argument errors are reported before anything is launched.
 *
 * Order of a list: score descending, then index descending — the total order of np.argsort(x)[::-1] and of tcar_rank_topk.  It is
 * a TOTAL order, so topk, score and rank are the same bits for every partition of the catalog into panels and on every run; ce is
 * an online sum whose rounding follows the partition. */
#ifndef TCAR_SERVE_H
#define TCAR_SERVE_H

#include "tcar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TCAR_SERVE_ABI_VERSION 1
int tcar_serve_abi_version(void);

/* running per-session state: k (score, index) entries kept sorted, strict-greater count, online (max, sum exp) */
int64_t tcar_select_state_bytes(int B, int k);                       /* k <= 64 */
int tcar_select_reset(int B, int k, void* state, void* stream);

/* fold the score columns [n0, n0 + n) of every session into the state.  panel: fp32, row b at panel + b*ld, column j = item n0 + j;
 * n <= 49,152 per call (the row slice is register resident), ld % 4 == 0, 16-byte aligned rows; columns >= n are never read as scores.
 * Every item is folded ONCE between a reset and a finish (the panels are disjoint), with the same k and the same excl in every call.
 *   lab_score [B] or NULL  -> count += #{j : n0 + j != label[b] and x > lab_score[b]};  label [B] or NULL (0-based; needed with lab_score)
 *   excl [B, X] or NULL    -> 0-based item ids (-1 = empty slot, repeats allowed) that must never enter session b's list;
 *                             exclusion affects the LIST only, never the count or the softmax sums */
int tcar_select_panel(int B, int n0, int n, const float* panel, int64_t ld, int k, const int32_t* label, const float* lab_score,
                      const int32_t* excl, int X, void* state, void* stream);

/* topk [B, k] (descending; -1 where fewer than k eligible items exist), score [B, k] or NULL (the fp32 score of each entry, bit for bit;
 * untouched where topk is -1), rank [B] or NULL (= 1 + count), ce [B] or NULL (= log-sum-exp over ALL folded columns - lab_score[b]) */
int tcar_select_finish(int B, int k, const void* state, const float* lab_score, int32_t* topk, float* score, int32_t* rank, float* ce,
                       void* stream);

/* One evaluation / recommendation step without the [B, N] logits. */
typedef struct {
  int32_t k, panel;                 /* panel: columns per panel, % 128 == 0, <= 49,152 */
  float* panel_buf;                 /* [ceil-to-B rows, panel] fp32 */
  void* state; int64_t state_bytes; /* >= tcar_select_state_bytes(B, k) */
  float* lab_score;                 /* [B] workspace (evaluation only) */
  const int32_t* excl; int32_t X;   /* optional exclusion lists [B, X] */
  int32_t* topk; float* score;      /* [B, k]; score may be NULL */
  int32_t* rank; float* ce;         /* [B]; written only when bt->label != NULL */
} tcar_serve_t;

/* session forward (+ candidate-time refresh), then for every panel: logits GEMM into panel_buf -> tcar_select_panel; tcar_select_finish.
 * bt->label == NULL: recommendation (no rank, no ce).  bt->neg / bt->K are ignored.  c->logits is neither read nor written.
 * The context covers the whole catalog (no shard).  lab_score[b] = attout[b] . E[label[b]] from the operands the panel GEMM reads. */
int tcar_serve_step(const tcar_ctx_t* c, const tcar_batch_t* bt, int refresh_time, const tcar_serve_t* s, void* stream);

#ifdef __cplusplus
}
#endif
#endif
