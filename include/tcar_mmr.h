/* tcar_mmr.h — diversity re-ranking on top of the two-stage call of tcar_retrieve.h: the k best of a shortlist are taken by a greedy
 * walk that charges every remaining slot for its CONTENT similarity to what is already listed (maximal marginal relevance, MMR).
 * Similarity is the cosine of two rows of the frozen fp32 content table, read in place (E[:, ldh : ldh + H] of a context), so a row
 * replaced by tcar_catalog_update is diversified against its new content by the next call; no derived table exists.
 *
 * The rule.  A session has C slots (ids, exact scores s, the `order` of tcar_cand_rank) and the call a penalty mu >= 0, finite, in
 * SCORE units: a verbatim duplicate of something already listed loses mu logits.  With the textbook weight lambda of
 * lambda * s - (1 - lambda) * max sim, mu = (1 - lambda) / lambda.  Scores are NOT min-max normalised per session: that would make
 * the meaning of lambda depend on the worst member of the shortlist.
 *   pool     the first P = min(eligible slots, TCAR_MMR_MAX_POOL) eligible slots of `order`; a slot is eligible iff tcar_cand_rank
 *            takes it as non-empty (id >= 0, score != -inf), its score is not NaN and its id lies in [0, N) (tcar_cand_scores has
 *            written -inf for every other id).  Nothing outside the pool can enter the list.
 *   sim      sim(i, j) = (x_i . x_j) * (r_i * r_j), x_n the H fp32 content columns of row n, r_n = 1 / sqrt(x_n . x_n) with
 *            correctly rounded sqrt and division, r_n = 0 for an all-zero row.  All fp32.  One dot is four fma chains — the columns
 *            c % 8 in {0,1,2,3} + 4 h of HALF h (h = 0, 1) form chains 0 .. 3 of that half, each over its columns in ascending order
 *            —, per half (c0 + c1) + (c2 + c3), then half 0 + half 1: the order depends on H alone, so the similarity of two items
 *            is the same bits in every session, slot, B, C and run, and sim(i, j) == sim(j, i).
 *   walk     m_c = 0 for every pool slot; for t = 0 .. k - 1 pick the pool slot not yet taken that is largest under (v_c descending,
 *            then item id descending, then slot ascending), v_c = s_c - mu * m_c as two separately rounded fp32 operations (multiply,
 *            then subtract; no fma); then m_c = max(m_c, sim(c, pick)) for every remaining slot.  m_c never falls below 0:
 *            similarity never rewards.  +0.0 and -0.0 are equal values.  A repeated id is a slot of its own and a perfect
 *            duplicate of its twin.
 *   outputs  topk [B, k]: item ids, -1 once the pool is used up; out_score [B, k]: the exact score of each pick bit for bit,
 *            untouched behind the last pick; msim [B, k] or NULL: m of each pick at the moment it was taken (0 for the first),
 *            untouched behind the last pick.
 *   mu = 0   v_c = s_c, so the walk takes the first k eligible slots of `order`: the list of tcar_rerank_take.
 *
 * Contracts as in tcar_cand.h: TCAR_OK / TCAR_E_ARG / TCAR_E_LAUNCH, launch on `stream`, never synchronise, never allocate, argument
 * errors before anything is launched, no mutable global state. */
#ifndef TCAR_MMR_H
#define TCAR_MMR_H

#include "tcar_retrieve.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TCAR_MMR_ABI_VERSION 1
#define TCAR_MMR_MAX_POOL 256
int tcar_mmr_abi_version(void);

/* One launch, one workgroup per session.  1 <= C <= 1024, 1 <= k <= 64, k <= C, N >= 1, H >= 1, mu >= 0 and finite.
 *   content  fp32, row n at content + n * ld_content (ld_content >= H): pass E + ldh with ld_content = ek for a context's table
 *   cand     int32 [B, ld_cand >= C]; score fp32 [B, ld_score >= C]; order int32 [B, C] of tcar_cand_rank
 *   topk     int32 [B, k]; out_score fp32 [B, k] or NULL; msim fp32 [B, k] or NULL
 * For H <= 256 the pool's rows are gathered ONCE, into registers; the rounds read nothing but LDS. */
int tcar_mmr_walk(int B, int C, int k, float mu, int N, int H, const float* content, int64_t ld_content, const int32_t* cand,
                  int64_t ld_cand, const float* score, int64_t ld_score, const int32_t* order, int32_t* topk, float* out_score,
                  float* msim, void* stream);

/* The diversified close of the two-stage call. */
typedef struct {
  float mu;                         /* the penalty, >= 0 and finite */
  float* msim;                      /* [B, k] or NULL */
} tcar_mmr_t;

/* tcar_retrieve_rerank_step with tcar_mmr_walk over the context's content table in place of its closing take: the retrieval step,
 * tcar_cand_scores, tcar_cand_rank for r->order, then the walk into (r->topk, r->score, m->msim).  One session forward. */
int tcar_mmr_rerank_step(const tcar_ctx_t* c, const tcar_batch_t* bt, int refresh_time, const tcar_retrieve_t* d, const tcar_rerank_t* r,
                         const tcar_mmr_t* m, void* stream);
/* ... for a ragged batch: `ragged` is the tcar_ragged_t of include/tcar_ragged.h, as a plain pointer; NULL is an argument error */
int tcar_mmr_rerank_step_ragged(const tcar_ctx_t* c, const tcar_batch_t* bt, const void* ragged, int refresh_time, const tcar_retrieve_t* d,
                                const tcar_rerank_t* r, const tcar_mmr_t* m, void* stream);

#ifdef __cplusplus
}
#endif
#endif
