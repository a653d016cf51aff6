/* tcar_sections.h — one list PER CATEGORY from one pass over the catalog, on top of the streamed score-and-select of tcar_serve.h /
 * tcar_window.h.  A front page has sections (sport, politics, culture, ...), each with a list of its own.  Every catalog item n carries
 * an int32 CATEGORY cat[n] (tcar_quota.h: the kernels only test categories for equality, so any int32 value is a code, INT32_MIN and
 * INT32_MAX included) and a call names G SECTIONS, 1 <= G <= 16: G pairwise distinct category codes.
 *
 * List g of session b is the k best items, 1 <= k <= 64, in the library's one list order (tcar_serve.h; key_gt of csrc/topk_rows.h:
 * score descending, then item id descending) among the items n with
 *   - cat[n] == sections[g],
 *   - n inside the session's window, if the call has one (tcar_window.h: lo[b] <= key[n] < hi[b]),
 *   - n not in the session's exclusion list,
 *   - a score that is not NaN.
 * Where fewer than k such items exist the list ends in -1 and the scores behind the end are untouched; a code no item carries gives
 * a list of -1 throughout.  +0.0 and -0.0 are EQUAL scores (the id decides); the score a list reports keeps its own bits.
 * There is no label, no rank and no cross entropy: sections are a recommendation call.
 *
 * State: B G rows of the select state of tcar_serve.h (2 k + 4 words each), row b G + g.  tcar_select_state_bytes(B G, k),
 * tcar_select_reset(B G, k, ...) and tcar_select_finish(B G, k, state, NULL, topk, score, NULL, NULL, ...) serve it unchanged, and the
 * rows are what tcar_select_merge (tcar_serve_shard.h) merges.  The sectioned fold never writes the four tail words of a row (count,
 * max, sum, pad: they keep the reset's bits).
 *
 * A fold is exact: the list order is a total order over the items, the sections partition what they list (the codes are distinct,
 * an item has one category), and a state row is the exact k best of its section over everything folded so far — an item that is not
 * among the k best of a subset is not among the k best of a superset.  So lists and scores are the same bits for every partition of
 * the catalog into panels, for every panel order and on every run.  The fold holds no float sum.
 *
 * Cost: ONE launch per panel, one workgroup per session, the row slice read once; an element is ADMITTED when it beats the k-th
 * best of its section so far (tcar_retrieve.h's selector, segmented by section).  A catalog whose scores ascend with the item id
 * inside a section admits every item of it: exact like every other case, and slow.
 *
 * Contracts as in tcar_serve.h: TCAR_OK / TCAR_E_ARG / TCAR_E_LAUNCH, launch on `stream`, never synchronise, never allocate, argument
 * errors before anything is launched, no mutable global state. */
#ifndef TCAR_SECTIONS_H
#define TCAR_SECTIONS_H

#include "tcar_window.h"
#include "tcar_ragged.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TCAR_SECTIONS_ABI_VERSION 1
#define TCAR_MAX_SECTIONS 16
int tcar_sections_abi_version(void);

/* fold the score columns [n0, n0 + n) of every session into its G state rows.  panel, ld, n, n0, excl and key / lo / hi exactly as
 * tcar_select_panel_window takes them: fp32, row b at panel + b*ld, column j = item n0 + j, n <= 49,152, ld % 4 == 0 and >= n, 16-byte
 * aligned rows, columns >= n never read as scores; n0 need not be a multiple of 4 and no load leaves a slice.
 *   sections  HOST array of G codes, copied into the launch arguments (nothing on the device is read to validate it)
 *   cat       device [N]: the category of every item; the fold reads cat[n0 .. n0 + n) (n0 + n <= N is the caller's promise)
 *   state     B G rows, row b G + g; every item is folded ONCE between a reset and a finish, with the same k, G, sections, excl and
 *             window in every call
 * TCAR_E_ARG: G outside 1 .. 16, two equal codes, NULL sections or cat, and every argument error of tcar_select_panel_window.
 * B == 0 or n == 0 with good arguments: TCAR_OK, nothing is launched. */
int tcar_section_panel(int B, int n0, int n, const float* panel, int64_t ld, int k, int G, const int32_t* sections, const int32_t* cat,
                       const int32_t* excl, int X, const int32_t* key, const int32_t* lo, const int32_t* hi, void* state, void* stream);

/* One sectioned recommendation step without the [B, N] logits. */
typedef struct {
  int32_t k, G;                     /* k: 1 .. 64 entries per list; G: 1 .. 16 sections */
  int32_t sections[TCAR_MAX_SECTIONS];    /* the G codes, by value; pairwise distinct */
  const int32_t* cat;               /* [N] device: the category of every catalog item */
  int32_t panel;                    /* columns per panel, % 128 == 0, <= 49,152 */
  float* panel_buf;                 /* [ceil-to-B rows, panel] fp32 */
  void* state; int64_t state_bytes; /* >= tcar_select_state_bytes(B G, k) */
  const int32_t* excl; int32_t X;   /* optional exclusion lists [B, X] */
  int32_t* topk; float* score;      /* [B, G, k]; score may be NULL */
  const tcar_window_t* window;      /* optional: every fold windowed (key [N] over the context's whole catalog); NULL: no window */
  const tcar_serve_t* overall;      /* optional: ALSO the one list over all categories, from the same panels (below); NULL: none */
} tcar_sections_t;

/* session forward (+ candidate-time refresh) exactly as tcar_serve_step runs it, a reset of the state, then for every panel: ONE
 * logits GEMM (the scoring of c->scoring) into panel_buf -> tcar_section_panel; tcar_select_finish over the B G rows.  bt->label,
 * bt->neg and c->logits are neither needed nor touched.  The context covers the whole catalog (no shard).
 * overall != NULL: every panel is ALSO folded by tcar_select_panel_window, unlabelled, into overall->state and finished into
 * overall->topk / overall->score [B, overall->k] — the bits of tcar_serve_step_window with the same window and exclusions, at the cost
 * of one more fold per panel and no more GEMM.  Of *overall only k, state, state_bytes, topk and score are read: the panel, its
 * buffer, the exclusion lists and the window are this descriptor's. */
int tcar_sections_step(const tcar_ctx_t* c, const tcar_batch_t* bt, int refresh_time, const tcar_sections_t* s, void* stream);

/* tcar_sections_step on a ragged batch (tcar_ragged.h): the ragged head, then the same body.  NULL rg: TCAR_E_ARG. */
int tcar_sections_step_ragged(const tcar_ctx_t* c, const tcar_batch_t* bt, const tcar_ragged_t* rg, int refresh_time,
                              const tcar_sections_t* s, void* stream);

#ifdef __cplusplus
}
#endif
#endif
