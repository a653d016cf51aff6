/* tcar_catalog_shard.h — in-place catalog updates where the candidate side of the catalog is SHARDED: the ownership-aware form of
 * tcar_catalog_update (tcar_catalog.h).  A rank of the catalog-sharded engine holds E whole — the session-side gathers read any row —
 * and everything else it derives from a catalog row for its rows [n0, n0 + n_loc) only, at local row n - n0.  Every rank is handed
 * the SAME request (the U rows of the whole update); a rank writes, of each named row, what it holds of it.
 *
 * What the context and the descriptor carry here:
 *   c->d.n_items = N, c->E                 the WHOLE catalog's: [ceil128(N), ek] fp32
 *   c->e16h / e16l                         the SHARD's planes, [ceil128(n_loc), ek] bf16 (KB32): row n at kb32_off(n - n0, col, ek / 32)
 *   c->Mi / Vi, c->mwdhm                   the SHARD's: [n_loc, ldh] and [n_loc, 5], row n at n - n0
 *   u->onehot                              the SHARD's one-hot plane, [ceil128(n_loc), onehot_inner], row n at n - n0
 *   u->key_table, u->cat_table             whole [N] tables: every rank keeps them whole, the folds compare global ids
 *   mwdhm_all                              an optional whole [N, 5] publish-time table (the one a rank keeps for the materialised
 *                                          evaluation over the whole catalog), or NULL
 *
 * For every n = ids[u] in [0, N):
 *   on EVERY rank                          the item and content columns of E[n] (the pad columns [H, ldh) zero), key_table[n],
 *                                          cat_table[n], mwdhm_all[n, :]
 *   only where n0 <= n < n0 + n_loc        both planes of the item and content columns, the clipped time block in the planes
 *                                          (refresh_time), the one-hot row, the Mi / Vi rows (zero_moments), c->mwdhm[n - n0, :]
 *   nothing else                           a row that is not named, the padding rows of every buffer and every row of a shard-local
 *                                          buffer whose id another rank owns keep every byte
 * An id outside [0, N) names no row and is skipped.
 *
 * The same bytes as a rebuild: tcar_catalog_update IS this call with (n0, n_loc) = (0, N) and no mwdhm_all — one kernel body serves
 * both entry points, so the split rounding of the planes, the clip of the time rows with its reduction order and the one-hot rule
 * are shared code, and kb32_off depends on neither N nor n_loc.  After the call a rank's buffers hold THE BYTES they would hold had
 * the shard been built from the final tables with tcar_split_bf16 / tcar_cand_time_fwd_bf16 / tcar_time_onehot over its rows.
 *
 * Plane contexts only (c->scoring != 0): the sharded step has no fp32 scoring mode, and an engine that holds the whole catalog
 * uses tcar_catalog_update.  Ownership is decided per wave (one wave per row); the workgroup barrier of the time-block hand-over
 * is reached by every wave, owner or not.
 *
 * Contracts as in tcar_catalog.h: TCAR_OK / TCAR_E_ARG / TCAR_E_LAUNCH, launch on `stream`, never synchronise, never allocate,
 * argument errors before anything is launched, no mutable global state.  U == 0 is TCAR_OK with nothing launched. */
#ifndef TCAR_CATALOG_SHARD_H
#define TCAR_CATALOG_SHARD_H

#include "tcar_catalog.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TCAR_CATALOG_SHARD_ABI_VERSION 1
int tcar_catalog_shard_abi_version(void);

/* Argument errors: those of tcar_catalog_update, and: c->scoring == 0; n0 < 0; n_loc <= 0; n0 + n_loc > N. */
int tcar_catalog_update_owned(const tcar_ctx_t* c, const tcar_catalog_update_t* u, int32_t n0, int32_t n_loc, int32_t* mwdhm_all,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif
