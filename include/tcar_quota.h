/* tcar_quota.h — per-category caps for the streamed score-and-select of tcar_serve.h / tcar_window.h.  Every catalog item n carries an
 * int32 CATEGORY cat[n] (the kernels only test categories for equality, so any int32 value is a code, negatives and INT32_MAX
 * included) and a call a CAP m >= 1: at most m items of any one category in a list.
 *
 * The list of session b is the result of a WALK: take its eligible items — in the pool of its window if there is one, and not
 * excluded — in the list order of tcar_serve.h (score descending, then item id descending); take an item iff fewer than m items of its
 * category have been taken; stop at k.  The list is what was taken, with -1 where the walk ends early.
 *   - Excluded and out-of-pool items do not exist for the walk and consume no quota.
 *   - The label is an ordinary item of the walk.
 *   - rank, ce and the softmax sums are not touched by the cap: they stay those of the whole pool (as exclusions leave them alone),
 *     and for a given partition they are the same bits as the uncapped call's.
 *   - m >= k is the uncapped call and runs the uncapped kernels: same bits, same cost.
 *   - All calls that share a state (reset ... finish) use the same cat and m, and the same excl and window as before.
 *
 * A fold is exact: with capped_k(S) the walk over a set S, capped_k(A u B) = capped_k(capped_k(A) u B).  An item y of A that the walk
 * over A did not take either has m better items of its category in A — they are still in A u B — or k items were taken before it, and
 * the number taken above y, sum over categories c of min(m, #items of c above y), only grows when items are added.  A dropped item never
 * comes back, so the running list of k (score, index) entries is a sufficient state (the category of an entry is re-read as
 * cat[index]), and topk and score are the same bits for every partition into panels and every panel order.  tcar_select_state_bytes,
 * tcar_select_reset and tcar_select_finish are those of tcar_serve.h, unchanged.
 *
 * Contracts as in tcar_serve.h: TCAR_OK / TCAR_E_ARG / TCAR_E_LAUNCH, launch on `stream`, never synchronise, never allocate, argument
 * errors before anything is launched. */
#ifndef TCAR_QUOTA_H
#define TCAR_QUOTA_H

#include "tcar_window.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TCAR_QUOTA_ABI_VERSION 1
int tcar_quota_abi_version(void);

typedef struct {
  const int32_t* cat;               /* [N] device: the category of every catalog item, indexed by 0-based item id */
  int32_t cap;                      /* m >= 1: at most m items of one category in a list */
} tcar_quota_t;

/* tcar_select_panel_window with a cap: column j of the panel is item n0 + j, and the fold reads cat[n0 + j] and cat[index] of the
 * state's entries (n0 + n <= N is the caller's promise, as for key).  cat == NULL (then cap == 0): exactly tcar_select_panel_window.
 * cat with cap < 1, or cap != 0 without cat: TCAR_E_ARG. */
int tcar_select_panel_quota(int B, int n0, int n, const float* panel, int64_t ld, int k, const int32_t* label, const float* lab_score,
                            const int32_t* excl, int X, void* state, void* stream, const int32_t* key, const int32_t* lo, const int32_t* hi,
                            const int32_t* cat, int cap);

/* tcar_serve_step_window with every fold capped by q (cat [N] over the context's whole catalog).  w == NULL: no window; q == NULL: no
 * cap (tcar_serve_step_window). */
int tcar_serve_step_quota(const tcar_ctx_t* c, const tcar_batch_t* bt, int refresh_time, const tcar_serve_t* s, const tcar_window_t* w,
                          const tcar_quota_t* q, void* stream);

#ifdef __cplusplus
}
#endif
#endif
