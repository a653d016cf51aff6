/* tcar_catalog.h — in-place catalog updates on top of the C ABI of tcar_hip.h: U rows of a LIVE context's catalog take new item rows,
 * content rows, publish times, keys or categories, and everything the context derives from a catalog row follows in the same launch.
 * A context is otherwise frozen when it is built: without this layer a new or corrected article costs a re-upload of both [N, H]
 * tables, a re-split of all Npad x ek plane elements and a whole-catalog refresh of the candidate time block.
 *
 * Every derived quantity of catalog row n is a pure function of the row, its publish_time_MWDHM entry and the five time tables:
 *   the fp32 image      E[n, 0:H] = item row, E[n, ldh:ldh+H] = content row, the pad columns [H, ldh) of both blocks zero;
 *   the bf16 planes     (c->scoring != 0) the same columns of e16h / e16l at kb32_off(n, col, ek / 32), hi = bf16(x),
 *                       lo = bf16(x - float(hi)): the rounding of tcar_split_bf16;
 *   the time block      clip(table_k[mwdhm[n, k]]), k = 0 .. 4, at columns 2 ldh + k ldt — in E on an fp32 context, in the planes ALONE
 *                       on a plane context: the destinations of the refresh the steps run (tcar_cand_time_fwd_bf16), and its bits: the
 *                       clip scale comes from the same code in the same reduction order;
 *   the one-hot row     of tcar_time_onehot (ones at the five time rows and the eight anchor columns, zeros elsewhere).
 * kb32_off(row, k, inner / 32) does not depend on N.  So after tcar_catalog_update every buffer holds THE BYTES it would hold had it
 * been built from the final tables with tcar_split_bf16 / tcar_cand_time_fwd_bf16 / tcar_time_onehot — no tolerance.
 *
 * What a call writes, for every named row n = ids[u] and for nothing else: the columns above of the tables it is given, the
 * context's mwdhm[n, :], key_table[n], cat_table[n], the Mi / Vi rows (zero_moments) — a row that is not named keeps every byte, the
 * padding rows [N, Npad) stay zero.  An id outside [0, N) names no row and is skipped; ids that repeat race with each other (one of
 * the payloads wins per 16-byte piece), never out of bounds.
 *
 * One wave per row: a 256-thread workgroup takes four rows, the grid follows U.  A lane owns 8 consecutive columns, so every plane
 * store is one whole 16-byte piece of the KB32 layout and every E store a float4.  The clipped time rows a row names (at most five) are
 * clipped inside its wave; nothing depends on U but the grid.
 *
 * Contracts as in tcar_serve.h: TCAR_OK / TCAR_E_ARG / TCAR_E_LAUNCH, launch on `stream`, never synchronise, never allocate, argument
 * errors before anything is launched, no mutable global state.  U == 0 is TCAR_OK with nothing launched. */
#ifndef TCAR_CATALOG_H
#define TCAR_CATALOG_H

#include "tcar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TCAR_CATALOG_ABI_VERSION 1
int tcar_catalog_abi_version(void);

typedef struct {
  int32_t U;                       /* rows named by this call */
  const int32_t* ids;              /* [U] device, 0-based, each in [0, N) of the context's catalog, pairwise distinct (not checked here) */
  const float* item;               /* [U, ld_item] new item-table rows (16-byte aligned), or NULL: keep */
  int64_t ld_item;                 /* >= H, % 4 == 0 */
  const float* content;            /* [U, ld_content] new content rows (16-byte aligned), or NULL: keep */
  int64_t ld_content;              /* >= H, % 4 == 0 */
  const int32_t* mwdhm;            /* [U, 5] new publish_time_MWDHM rows -> the context's mwdhm[ids[u], :], or NULL: keep */
  int32_t refresh_time;            /* != 0: also rewrite the clipped time block of the U rows (from `mwdhm`, else from the context's table) */
  const int32_t* key;              /* [U] -> key_table[ids[u]] (both or neither) */
  int32_t* key_table;              /* [N] the item keys of tcar_window.h */
  const int32_t* cat;              /* [U] -> cat_table[ids[u]] (both or neither) */
  int32_t* cat_table;              /* [N] the category table of tcar_quota.h */
  int32_t zero_moments;            /* != 0: the Mi / Vi rows of the U items := 0 (a replaced row has no optimizer history) */
  void* onehot;                    /* the static one-hot plane of tcar_time_onehot, [ceil128(N), onehot_inner] bf16 (KB32), or NULL: not kept by
                                      this context; written where `mwdhm` is given */
  int64_t onehot_inner;            /* % 32 == 0, >= 160 (with onehot) */
} tcar_catalog_update_t;

/* Argument errors: NULL c or u; U < 0; ids NULL; none of item / content / mwdhm / key / cat; a table that is not 16-byte aligned, ld < H
 * or ld % 4 != 0; key without key_table or the reverse, likewise cat; refresh_time without u->mwdhm and c->mwdhm; onehot with a bad
 * onehot_inner — then those of the context: bad dims, E NULL, scoring != 0 without e16h / e16l, mwdhm given without c->mwdhm,
 * zero_moments without Mi / Vi, refresh_time without W.  c->mwdhm is written through (the context declares it const for the steps). */
int tcar_catalog_update(const tcar_ctx_t* c, const tcar_catalog_update_t* u, void* stream);

#ifdef __cplusplus
}
#endif
#endif
