/* tcar_ragged.h — ragged batches on top of the C ABI of tcar_hip.h: B sessions of MIXED lengths in one serving call.  The
 * rectangular entry points take one length T per call, so a request batch of every length costs one call — and one stream of the
 * whole catalog — per length.  Of the session forward only two kernels know T: the gather (t = row % T picks the position row) and the
 * attention pool (one wave owns one session, row = b * T + t).  Their ragged forms read the position of a row and the first row of a
 * session from a descriptor instead; the projections, the click-query MLP and the output transforms are per-row or per-session
 * problems, and everything behind attout (panel GEMM, folds, candidate gather) is per-session already.
 *
 * A ragged call passes a tcar_batch_t with
 *   B sessions, T = the longest length (1 .. 40), K = 0, neg = NULL;
 *   seq / pub[5] / gap as flat [R] arrays: session b occupies the rows [off[b], off[b + 1]);
 *   cw / ch / label as [B]
 * and a tcar_ragged_t.  The activations of tcar_ctx_t must cover R rows (x_icp, x_pt, x_act, pre1, pre2: [R, .]; alpha: [3, R]) and B
 * sessions; proj_slabs is used when it holds the slabs of R rows.
 *
 * The library cannot read device arrays without a synchronise, so the kernels are safe on bad contents.  They enforce:
 *   * the length of session b is off[b + 1] - off[b] clamped into 0 .. 40, and then cut so that off[b] + length <= R; a session whose
 *     off[b] is outside [0, R) has length 0 (its pooled row is zero, its alpha rows are not written);
 *   * no row index >= R (or < 0) is read or written;
 *   * pos[row] is clamped into 0 .. 39 (the position table has 40 rows); item and time ids are clamped as the rectangular gather
 *     clamps them.
 * A descriptor that overlaps sessions or leaves rows unowned gives finite garbage in those sessions, never a fault.
 *
 * Uniform lengths: a ragged call whose sessions all have the length T (off[b] = b T, pos[row] = row % T, R = B T) runs the launches of
 * the rectangular call — same grids, same problems, same form rules, which depend on the row count alone — and every wave runs the
 * same operations on the same rows in the same order: attout and every output carry the bits of the rectangular call.
 *
 * No backward kernel has a ragged form: training stays rectangular.
 *
 * Contracts as in tcar_serve.h: TCAR_OK / TCAR_E_ARG / TCAR_E_LAUNCH, launch on `stream`, never synchronise, never allocate, argument
 * errors before anything is launched, no mutable global state.  Argument errors of every entry point below: NULL rg, rg->off or
 * rg->pos; R < B or R > 40 B; T outside 1 .. 40 — beside those of its rectangular twin. */
#ifndef TCAR_RAGGED_H
#define TCAR_RAGGED_H

#include "tcar_serve.h"
#include "tcar_quota.h"
#include "tcar_retrieve.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TCAR_RAGGED_ABI_VERSION 1
int tcar_ragged_abi_version(void);

typedef struct {
  int32_t R;            /* session rows in all = sum of the lengths; B <= R <= 40 B */
  const int32_t* off;   /* device [B + 1]: first row of session b; off[0] = 0, off[B] = R, 1 <= off[b+1] - off[b] <= 40 */
  const int32_t* pos;   /* device [R]: position of a row inside its session, row - off[session] */
} tcar_ragged_t;

/* ---- op level, beside the rectangular entry points of tcar_hip.h ---- */

/* tcar_gather_clip_fwd over the R rows of a ragged batch: x_icp [R, ic], x_pt [R, pt], x_act [R, ldt], click_t [B, ct]; the position
 * row of a row is pos[row] in place of row % T.  The launch form follows the row count R as the rectangular call's follows B T
 * (latency form / throughput form: the same bits). */
int tcar_gather_clip_fwd_ragged(const tcar_dims_t* d, const tcar_tables_t* tab, const tcar_batch_t* bt, const tcar_ragged_t* rg,
                                float* x_icp, float* x_pt, float* x_act, float* click_t, void* stream);

/* tcar_attn_pool_fwd / tcar_attn_pool_fwd_slabs with `rg` in place of T: the wave of session b reads off[b] and its length and walks
 * its own rows; pooled [B, ek]; alpha [3, R] (plane p of session b at alpha + p R + off[b]); slab_stride >= R ldh. */
int tcar_attn_pool_fwd_ragged(const tcar_dims_t* d, int B, const tcar_ragged_t* rg, const float* x_icp, const float* x_pt,
                              const float* pre1, const float* pre2, const float* q, const float* w_res1, const float* w_res2,
                              float* pooled, float* alpha, void* stream);
int tcar_attn_pool_fwd_slabs_ragged(const tcar_dims_t* d, int B, const tcar_ragged_t* rg, const float* x_icp, const float* x_pt,
                                    const float* pre1_slabs, int n1, const float* pre2_slabs, int n2, int64_t slab_stride, float* pre1,
                                    float* pre2, const float* q, const float* w_res1, const float* w_res2, float* pooled, float* alpha,
                                    void* stream);

/* ---- steps: the ragged head, then the body the rectangular twin runs ---- */

/* The head of a forward pass: the candidate-time refresh where it is due (refresh_time != 0), then the session forward of the ragged
 * batch; leaves c->attout [B, ek] and its bf16 planes (split-bf16 contexts). */
int tcar_ragged_forward(const tcar_ctx_t* c, const tcar_batch_t* bt, const tcar_ragged_t* rg, int refresh_time, void* stream);

/* tcar_serve_step_quota (w / q NULL: the unwindowed / uncapped step), tcar_cand_step, tcar_retrieve_step and
 * tcar_retrieve_rerank_step on a ragged batch */
int tcar_serve_step_ragged(const tcar_ctx_t* c, const tcar_batch_t* bt, const tcar_ragged_t* rg, int refresh_time, const tcar_serve_t* s,
                           const tcar_window_t* w, const tcar_quota_t* q, void* stream);
int tcar_cand_step_ragged(const tcar_ctx_t* c, const tcar_batch_t* bt, const tcar_ragged_t* rg, int refresh_time, const tcar_cand_t* d,
                          void* stream);
int tcar_retrieve_step_ragged(const tcar_ctx_t* c, const tcar_batch_t* bt, const tcar_ragged_t* rg, int refresh_time,
                              const tcar_retrieve_t* d, void* stream);
int tcar_retrieve_rerank_step_ragged(const tcar_ctx_t* c, const tcar_batch_t* bt, const tcar_ragged_t* rg, int refresh_time,
                                     const tcar_retrieve_t* d, const tcar_rerank_t* r, void* stream);

#ifdef __cplusplus
}
#endif
#endif
