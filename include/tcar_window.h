/* tcar_window.h — publish-time windows for the streamed score-and-select of tcar_serve.h.  The catalog carries one int32 KEY per item
 * (key [N]; the trainer uses the publish time in minutes, the kernels only compare integers) and every session of a call a half-open
 * interval [lo[b], hi[b]).  Item n is in the POOL of session b iff
 *     lo[b] <= key[n] < hi[b],   or   the call is labelled (lab_score != NULL) and n == label[b].
 * For a session, items outside its pool do not exist: they never enter the list, are not counted in the rank and add nothing to the
 * softmax sums.  The label is always in the pool, so rank and ce stay defined.  Exclusion lists keep their meaning (the list only) and
 * apply on top of the window; where fewer than k pool items remain the list ends in -1.  lo[b] >= hi[b] is an empty pool, not an error.
 *
 * Contracts as in tcar_serve.h: TCAR_OK / TCAR_E_ARG / TCAR_E_LAUNCH, launch on `stream`, never synchronise, never allocate, argument
 * errors before anything is launched.  Calls that share a state (reset ... finish) use the same window.  topk, score and rank are
 * exact in the total order of tcar_serve.h restricted to the pool: the same bits for every partition into panels and on every run. */
#ifndef TCAR_WINDOW_H
#define TCAR_WINDOW_H

#include "tcar_serve.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TCAR_WINDOW_ABI_VERSION 1
int tcar_window_abi_version(void);

typedef struct {
  const int32_t* key;               /* [N] device: one key per catalog item, indexed by 0-based item id */
  const int32_t *lo, *hi;           /* [B] device: session b's pool is lo[b] <= key < hi[b] (+ its label) */
} tcar_window_t;

/* tcar_select_panel with a window: column j of the panel is item n0 + j, so the fold reads key[n0 + j] (n0 + n <= N; n0 need not be a
 * multiple of 4).  key == NULL (then lo and hi are NULL too): exactly tcar_select_panel.  key without lo or hi, or lo / hi without key:
 * TCAR_E_ARG, as every argument error of tcar_select_panel. */
int tcar_select_panel_window(int B, int n0, int n, const float* panel, int64_t ld, int k, const int32_t* label, const float* lab_score,
                             const int32_t* excl, int X, void* state, void* stream, const int32_t* key, const int32_t* lo, const int32_t* hi);

/* tcar_serve_step with every fold windowed by w (key [N] over the context's whole catalog).  w == NULL: tcar_serve_step. */
int tcar_serve_step_window(const tcar_ctx_t* c, const tcar_batch_t* bt, int refresh_time, const tcar_serve_t* s, const tcar_window_t* w,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif
