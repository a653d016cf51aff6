// Softmax cross entropy from the logits GEMM's softmax epilogue (tcar_gemm_bf16_ce, gemm_bf16.hip) for gfx950: the "finish" family.
// The epilogue left, per session row and column group g, (m_g, s_g) = (group maximum, sum of exp(x - m_g)), the plane
// e[b, n] = bf16(exp(x - m_g(n))) and the label's score.  Combine: M = max_g m_g, S = sum_g s_g exp(m_g - M),
// lse = M + log S, ce = lse - x_label (model_combine.py:145); rescale: plane = softmax - onehot, the gradient of the SUM of the
// per-session losses (model_combine.py:147,156).  The kernels here are front ends: the folds, the label rule, the rounding of a
// piece and the anchored row tail live ONCE in ce_rows.h.
#include <type_traits>
#include "ce_rows.h"

namespace {

// ---- grouped form, two launches: combine (one wave per row), then rescale ----------------------------------------------------------
__global__ __launch_bounds__(256) void ce_combine_kernel(int B, int ngroups, const float* __restrict__ stats,
                                                         const float* __restrict__ lab_logit, float* __restrict__ rowstat,
                                                         float* __restrict__ ce) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float2 ms = ce_row_max_sumexp(reinterpret_cast<const float2*>(stats) + (long)b * ngroups, ngroups, lane);
  if (lane == 0) {
    rowstat[2 * b] = ms.x;
    rowstat[2 * b + 1] = 1.0f / ms.y;
    ce[b] = ms.x + logf(ms.y) - lab_logit[b];
  }
}
// Rescale in place (ce_rescale_piece); rows [B, ceil128(B)) are zeroed (they are k-rows of dE).
// One thread per 16-byte piece position (row, q) of CE_KPT consecutive 32-column blocks: a wave instruction moves 1 KB of
// CONTIGUOUS plane (16 rows x 64 bytes) and the CE_KPT loads of a thread are independent (round 4: one thread per 64-byte row
// read its four pieces with four instructions of 64-byte lane stride — 26 us for the 94 MB of the Globo plane).
constexpr int CE_KPT = 4;
template <int GW>
__device__ __forceinline__ void ce_rescale_body(int B, int N, int in32, int ngroups, const float* __restrict__ stats,
                                                const float* __restrict__ rowstat, const int32_t* __restrict__ label,
                                                __bf16* __restrict__ plane, long nunits, int lab_off, int lab_window, bool wt) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nunits) return;
  const int q = (int)(i & 3), r = (int)((i >> 2) & 127);
  const long chunk = i >> 9;
  const int nch = (in32 + CE_KPT - 1) / CE_KPT;
  const long rb = chunk / nch;
  const int kb0 = (int)(chunk - rb * nch) * CE_KPT;
  const long row = rb * 128 + r;
  uint4* p = reinterpret_cast<uint4*>(plane + (rb * in32 + kb0) * 4096 + r * 32 + q * 8);      // block kb0 + j: p + 512 j
  if (row >= B) {
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int j = 0; j < CE_KPT; ++j)
      if (kb0 + j < in32) ce_store16(p + 512 * j, z, wt);
    return;
  }
  uint4 v[CE_KPT];
#pragma unroll
  for (int j = 0; j < CE_KPT; ++j)
    if (kb0 + j < in32) v[j] = p[512 * j];
  const float2 rs = *reinterpret_cast<const float2*>(rowstat + 2 * row);
  const int labc = ce_label_col(label[row], lab_off, N, lab_window);
  const int piece = q ^ ((r >> 2) & 3);                           // storage position q holds logical piece q ^ sw
  const float* strow = stats + row * ngroups * 2;
#pragma unroll
  for (int j = 0; j < CE_KPT; ++j) {
    if (kb0 + j >= in32) break;
    ce_store16(p + 512 * j, ce_rescale_piece<GW>(v[j], rs, strow, ngroups, N, (kb0 + j) * 32, labc, piece), wt);
  }
}
template <int GW>
__global__ __launch_bounds__(256) void ce_rescale_kernel(int B, int N, int in32, int ngroups, const float* __restrict__ stats,
                                                         const float* __restrict__ rowstat, const int32_t* __restrict__ label,
                                                         __bf16* __restrict__ plane, long nunits, int lab_off, int lab_window,
                                                         const TcarSignal sig) {
  ce_rescale_body<GW>(B, N, in32, ngroups, stats, rowstat, label, plane, nunits, lab_off, lab_window, sig.cnt != nullptr);
  tcar_signal_done(sig);        // (the body is a function: its early returns end up here)
}

// ---- ANCHORED form (round 6): the plane holds exp(x - anchor[b]) with ONE reference per row — subtracted INSIDE the logits GEMM's
// contraction (anchor columns of its one-hot K segment: embed.hip; tcar_gemm_bf16_ce_o with TcarOpt::anchored), so that the GEMM's
// epilogue neither computes group maxima nor loads anything —, a row's softmax is plane / S_b with S_b = the sum of its group sums, and
// NO pass over the [B, N] plane follows the logits GEMM: this launch (one wave per session row) folds the row's group sums in a fixed
// order — ce = log S_b - (x_label - anchor), the label's accumulator as the GEMM leaves it in lab_logit — and prepares the two
// consumers, which scale PER ROW (ce_anchor_row_tail):
//   * the label's -1 goes INTO the plane as v = bf16(e_l - S_b).  Rounded like that it carries the one-hot — the LARGEST term of a
//     row's gradient while the softmax is flat — with up to 2^-8 relative error (measured: 1.6e-3 instead of 1e-4 norm-wise on the
//     time-side gradients against the fp64 oracle), so the residual d = (e_l - S_b) - v is kept in fp32;
//   * dX is linear in the plane's rows: its slab reduce multiplies by scale2[b].x = 1 / S_b and adds scale2[b].y = d / S_b times the
//     label's candidate row in fp32 (TcarRowFix) — softmax part scaled exactly, one-hot part exact;
//   * dE contracts over b, so the scale rides on attout's rows: aps[b, :] = bf16((ap_hi + ap_lo)[b, :] / S') with S' = e_l - v; the
//     rounding of v becomes a common factor S_b / S' = 1 +- 2^-8 on the row's softmax part.
// 94 MB of plane traffic and ~23 us of the step's critical chain become 0.6 MB and one small launch.  The anchor is the label's
// score up to rounding (embed.hip: attout_finish_kernel), hence S_b >= ~1 (no underflow for any logits); the GEMM clamps its
// exponent at 2^100 (a logit > 69 nats above the anchor saturates): nothing overflows.
__global__ __launch_bounds__(256) void ce_anchor_fold_kernel(int B, int N, int in32, int ngroups, const float* __restrict__ stats,
                                                             const float* __restrict__ lab_logit, const int32_t* __restrict__ label,
                                                             float* __restrict__ rowstat, float* __restrict__ ce,
                                                             float* __restrict__ scale2, __bf16* __restrict__ plane,
                                                             const __bf16* __restrict__ ap_hi, const __bf16* __restrict__ ap_lo,
                                                             __bf16* __restrict__ aps, int ap_cols, int ap_in32) {
  const int lane = threadIdx.x & 63;
  const long b = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ce_anchor_pad_row(b, B, aps, ap_cols, ap_in32, lane)) return;
  // (.x: the sum of the plane's ROUNDED entries — the gradient's scale, consistent with what the GEMMs contract; .y: the sum of the
  //  exponentials themselves — the loss)
  const int lab = clampi(label[b], 0, N - 1);
  const float xl = lab_logit[b];
  const float2 s = ce_row_sums(reinterpret_cast<const float2*>(stats) + b * ngroups, ngroups, lane);
  ce_anchor_row_tail(b, lab, s.x, 1.0f / s.x, scale2, plane, in32, ap_hi, ap_lo, aps, ap_cols, ap_in32, lane);
  // (the wave's stores come AFTER its loads: a store between two dependent loads makes the second wait for the store's acknowledge too)
  if (lane == 0) {
    if (rowstat) { rowstat[2 * b] = 0.f; rowstat[2 * b + 1] = 1.0f / s.y; }           // (reference of the exponentials: the anchor = 0 here)
    ce[b] = logf(s.y) - xl;
  }
}
// ... for the catalog-sharded step: the row sums crossed the ranks (rowstat[b].x = the sum over the shards of their planes' rounded
// entries, from tcar_softmax_combine_anchored), the label lives in ONE shard (window: label - lab_off inside [0, N) or no label
// entry here), and a padding session (label < 0, lse = +inf) gets an exactly zero gradient row: scale 0 on both consumers
__global__ __launch_bounds__(256) void ce_anchor_apply_kernel(int B, int N, int in32, const float* __restrict__ rowstat,
                                                              const int32_t* __restrict__ label, int lab_off,
                                                              float* __restrict__ scale2, __bf16* __restrict__ plane,
                                                              const __bf16* __restrict__ ap_hi, const __bf16* __restrict__ ap_lo,
                                                              __bf16* __restrict__ aps, int ap_cols, int ap_in32) {
  const int lane = threadIdx.x & 63;
  const long b = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ce_anchor_pad_row(b, B, aps, ap_cols, ap_in32, lane)) return;
  const int lraw = label[b];
  const bool live = lraw >= 0;
  const float s = live ? rowstat[2 * b] : 0.f;    // (anchored convention: the sum over the shards of the planes' ROUNDED entries)
  ce_anchor_row_tail(b, live ? ce_label_col(lraw, lab_off, N, 1) : CE_NO_LABEL, s, live ? 1.0f / s : 0.f, scale2, plane, in32, ap_hi,
                     ap_lo, aps, ap_cols, ap_in32, lane);
}

// ---- grouped form, ONE launch (round 5; TCAR_CE_FOLD): ce_combine + ce_rescale.  A workgroup owns 16 session rows x one slice of
// the plane's column blocks.  It folds ITS rows' (max, sum) pairs itself — ngroups * 8 bytes per row out of L2, ce_combine_kernel's
// fold, so lse / ce / the scale come out in the same bits — and then streams its slice: a wave instruction is one 128 x 32 block's
// 16 rows x 64 bytes = 1 KB contiguous (lane = (row, 16-byte piece)), CE_FKPT independent loads in flight per wave, issued BEFORE
// the fold (they do not depend on it).  Slice 0 also writes rowstat and ce.  The launch saves the combine kernel (7.6 us) and its
// boundary on the step's critical chain; the pairs are re-read once per slice.
constexpr int CE_FKPT = 8;
template <int GW>
__global__ __launch_bounds__(256) void ce_fold_rescale_kernel(int B, int N, int in32, int ngroups, const float* __restrict__ stats,
                                                              const float* __restrict__ lab_logit, const int32_t* __restrict__ label,
                                                              float* __restrict__ rowstat, float* __restrict__ ce,
                                                              __bf16* __restrict__ plane, int nslice, int lab_off, int lab_window,
                                                              const TcarSignal sig) {
  __shared__ float sM[16], sR[16];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int rg = blockIdx.x / nslice, sl = blockIdx.x - rg * nslice;
  const int row0 = rg * 16;                                    // 16 rows of one 128-row block (16 divides 128)
  const int per = (in32 + nslice - 1) / nslice;
  const int kb_lo = sl * per, kb_hi = min(in32, kb_lo + per);
  const bool wt = sig.cnt != nullptr;
  const int r = (row0 & 127) + (lane >> 2), q = lane & 3;
  const long row = row0 + (lane >> 2);
  // block kb of this wave's 16 rows: 16 bytes per lane, 1 KB per wave instruction
  uint4* p0 = reinterpret_cast<uint4*>(plane + ((long)(row0 >> 7) * in32) * 4096 + r * 32 + q * 8);
  const int kb_first = kb_lo + wv;                             // wave w takes blocks kb_lo + w, + 4, ...
  if (row0 >= B) {                                             // pad rows of the last 128-row block: zero (they are k-rows of dE)
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    for (int kb = kb_first; kb < kb_hi; kb += 4) ce_store16(p0 + 512L * kb, z, wt);
    tcar_signal_done(sig);
    return;
  }
  uint4 v[CE_FKPT];
#pragma unroll
  for (int j = 0; j < CE_FKPT; ++j) {
    const int kb = kb_first + 4 * j;
    if (kb < kb_hi) v[j] = p0[512L * kb];
  }
  // ---- fold: wave w takes rows row0 + 4 w .. + 3
  const float2* st2 = reinterpret_cast<const float2*>(stats);
  auto put_row = [&](int i, float2 ms) {                       // (M, S) of the wave's i-th row
    const int b = row0 + 4 * wv + i;
    if (lane == 0 && b < B) {
      const float inv = 1.0f / ms.y;
      sM[4 * wv + i] = ms.x;
      sR[4 * wv + i] = inv;
      if (sl == 0) {
        if (rowstat) { rowstat[2 * b] = ms.x; rowstat[2 * b + 1] = inv; }
        ce[b] = ms.x + logf(ms.y) - lab_logit[b];
      }
    }
  };
  if (ngroups <= 64 * CE_NG) {
    // every pair of the wave's four rows is LOADED before the first use: one L2 round trip per workgroup (the first version walked
    // two dependent loops per row — 64 serial round trips, 46 us for the launch)
    float2 pr[4][CE_NG];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      ce_load_pairs(pr[i], st2 + (long)min(row0 + 4 * wv + i, B - 1) * ngroups, ngroups, lane, make_float2(-INFINITY, 0.f));
#pragma unroll
    for (int i = 0; i < 4; ++i) put_row(i, ce_fold_max_sumexp(CE_NG, [&](int j) { return pr[i][j]; }));
  } else {
#pragma unroll 1
    for (int i = 0; i < 4; ++i) {
      const int b = row0 + 4 * wv + i;
      if (b >= B) break;
      put_row(i, ce_row_max_sumexp(st2 + (long)b * ngroups, ngroups, lane));
    }
  }
  __syncthreads();
  const bool live = row < B;
  const float2 rs = live ? make_float2(sM[lane >> 2], sR[lane >> 2]) : make_float2(0.f, 0.f);
  const int labc = live ? ce_label_col(label[row], lab_off, N, lab_window) : CE_NO_LABEL;
  const int piece = q ^ ((r >> 2) & 3);                         // storage position q holds logical piece q ^ sw
  const float* strow = stats + (live ? row : 0) * ngroups * 2;
  const int ng_row = live ? ngroups : 0;                        // (a pad row of a live 16-row group reads no statistic and is zeroed)
  for (int kb0 = kb_first; kb0 < kb_hi; kb0 += 4 * CE_FKPT) {
    if (kb0 != kb_first) {                                     // (the first trip's loads were issued ahead of the fold)
#pragma unroll
      for (int j = 0; j < CE_FKPT; ++j) {
        const int kb = kb0 + 4 * j;
        if (kb < kb_hi) v[j] = p0[512L * kb];
      }
    }
#pragma unroll
    for (int j = 0; j < CE_FKPT; ++j) {
      const int kb = kb0 + 4 * j;
      if (kb >= kb_hi) continue;
      const uint4 y = ce_rescale_piece<GW>(v[j], rs, strow, ng_row, N, kb * 32, labc, piece);
      ce_store16(p0 + 512L * kb, live ? y : make_uint4(0u, 0u, 0u, 0u), wt);
    }
  }
  tcar_signal_done(sig);
}

// Catalog-sharded step: the shard's (max, sum exp, label score) per session from the epilogue's per-group pairs — the row of the
// statistics all-gather (shard.hip: softmax_combine); anchored != 0: (sum of the plane's rounded entries, sum of the exponentials,
// label's accumulator).  One wave per row.
__global__ __launch_bounds__(256) void ce_shard_stats_kernel(int B, int ngroups, const float* __restrict__ stats,
                                                             const float* __restrict__ lab_logit, const int32_t* __restrict__ label,
                                                             int n0, int n_loc, float* __restrict__ out3, int anchored) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float2* st = reinterpret_cast<const float2*>(stats) + (long)b * ngroups;
  const float2 folded = anchored ? ce_row_sums(st, ngroups, lane) : ce_row_max_sumexp(st, ngroups, lane);
  if (lane == 0) {     // the label's score: 0 unless the label lies in [n0, n0 + n_loc)
    out3[3L * b] = folded.x;
    out3[3L * b + 1] = folded.y;
    out3[3L * b + 2] = ce_label_col(label[b], n0, n_loc, 1) != CE_NO_LABEL ? lab_logit[b] : 0.f;
  }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------
// the one place where the group width of the logits layout (64 or 96 columns) becomes a template argument: launch(constant<GW>)
template <class F>
void ce_by_group_width(int group_width, F launch) {
  if (group_width == 96) launch(std::integral_constant<int, 96>{});
  else launch(std::integral_constant<int, 64>{});
}
// the argument terms the launchers share.  The plane: [ceil128(B), inner] in KB32 layout, N live columns, one label per row ...
bool ce_plane_ok(int N, const int32_t* label, const void* dl_hi, int64_t inner) {
  return N > 0 && label && dl_hi && !(inner & 31) && inner >= N;
}
// ... with the epilogue's pairs [B, ngroups] of group_width columns each, and the row statistics as float2
bool ce_grouped_ok(int N, int group_width, int ngroups, const float* stats, const float* rowstat, const int32_t* label,
                   const void* dl_hi, int64_t inner) {
  return ce_plane_ok(N, label, dl_hi, inner) && stats && ngroups > 0 && (group_width == 64 || group_width == 96) &&
         (long)ngroups * group_width >= N && !((uintptr_t)rowstat & 7);
}
// ... the packed attout planes of the dE GEMM [B, ap_cols] (inner dimension ap_inner, KB32) and the per-row scales as float2
bool ce_attout_ok(const void* ap_hi, const void* ap_lo, const void* aps_hi, int ap_cols, int64_t ap_inner, const float* scale2) {
  return ap_hi && ap_lo && aps_hi && ap_cols > 0 && !(ap_cols & 3) && !(ap_inner & 31) && ap_inner >= ap_cols && scale2 &&
         !((uintptr_t)scale2 & 7);
}

}  // namespace

// second half of tcar_ce_finish on its own (catalog-sharded step: the row statistics come from the statistics exchange):
// plane[b, n] = e[b, n] * exp(m_g - rowstat[b].x) * rowstat[b].y - [n == label[b] - lab_off]; lab_window != 0: a label outside
// [lab_off, lab_off + N) belongs to another shard and nothing is subtracted
// (flag-capable: with a completion flag the rescale stores the plane write-through — what the flag's consumer, the dE GEMM on the aux
//  stream, reads)
int tcar_ce_rescale_o(int B, int N, int group_width, int ngroups, const float* stats, const float* rowstat, const int32_t* label,
                      int lab_off, int lab_window, void* dl_hi, int64_t inner, void* stream, TcarOpt* o) {
  if (B <= 0) return TCAR_OK;
  if (!ce_grouped_ok(N, group_width, ngroups, stats, rowstat, label, dl_hi, inner) || !rowstat) return TCAR_E_ARG;
  const int in32 = (int)(inner >> 5);
  const long nunits = (((long)B + 127) >> 7) * ((in32 + CE_KPT - 1) / CE_KPT) * 512;
  const unsigned grid = (unsigned)((nunits + 255) / 256);
  const TcarSignal sig = tcar_sig(o);
  ce_by_group_width(group_width, [&](auto gw) {
    TCAR_LAUNCH(ce_rescale_kernel<decltype(gw)::value>, dim3(grid), dim3(256), 0, (hipStream_t)stream, B, N, in32, ngroups, stats, rowstat, label,
                (__bf16*)dl_hi, nunits, lab_off, lab_window, sig);
  });
  TCAR_CHECK_LAUNCH();
  return TCAR_OK;
}
extern "C" int tcar_ce_rescale(int B, int N, int group_width, int ngroups, const float* stats, const float* rowstat,
                               const int32_t* label, int lab_off, int lab_window, void* dl_hi, int64_t inner, void* stream) {
  return tcar_ce_rescale_o(B, N, group_width, ngroups, stats, rowstat, label, lab_off, lab_window, dl_hi, inner, stream, nullptr);
}

int tcar_ce_finish_o(int B, int N, int group_width, int ngroups, const float* stats, const float* lab_logit, const int32_t* label,
                     float* rowstat, float* ce, void* dl_hi, int64_t inner, void* stream, TcarOpt* o) {
  if (B <= 0) return TCAR_OK;
  if (!ce_grouped_ok(N, group_width, ngroups, stats, rowstat, label, dl_hi, inner) || !lab_logit || !rowstat || !ce) return TCAR_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  // TCAR_CE_FOLD = w > 0 (default 1024): ONE launch of about w workgroups, each folding its own 16 rows' pairs (ce_fold_rescale_kernel);
  // 0: the combine launch + the rescale launch (same bits either way)
  // (every slice re-reads its rows' pairs: fine while the [B, ngroups, 2] statistics sit in the L2s — 2 MB at the Globo shape —, a
  //  multiple of the plane's own traffic beyond; a 10 M-item catalog keeps the two launches)
  const int fold = tcar_tn(o).ce_fold;
  if (fold > 0 && (int64_t)B * ngroups * 8 <= (8LL << 20)) {
    const int in32 = (int)(inner >> 5);
    const int rgroups = (((B + 127) >> 7) << 7) / 16;
    int nslice = fold / rgroups;
    if (nslice > in32 / 4) nslice = in32 / 4;
    if (nslice < 1) nslice = 1;
    const TcarSignal sig = tcar_sig(o);
    ce_by_group_width(group_width, [&](auto gw) {
      TCAR_LAUNCH(ce_fold_rescale_kernel<decltype(gw)::value>, dim3(rgroups * nslice), dim3(256), 0, st, B, N, in32, ngroups, stats, lab_logit, label,
                  rowstat, ce, (__bf16*)dl_hi, nslice, 0, 0, sig);
    });
    TCAR_CHECK_LAUNCH();
    return TCAR_OK;
  }
  TCAR_LAUNCH(ce_combine_kernel, dim3((B + 3) / 4), dim3(256), 0, st, B, ngroups, stats, lab_logit, rowstat, ce);
  TCAR_CHECK_LAUNCH();
  return tcar_ce_rescale_o(B, N, group_width, ngroups, stats, rowstat, label, 0, 0, dl_hi, inner, stream, o);
}
extern "C" int tcar_ce_finish(int B, int N, int group_width, int ngroups, const float* stats, const float* lab_logit,
                              const int32_t* label, float* rowstat, float* ce, void* dl_hi, int64_t inner, void* stream) {
  return tcar_ce_finish_o(B, N, group_width, ngroups, stats, lab_logit, label, rowstat, ce, dl_hi, inner, stream, nullptr);
}

// anchored form of tcar_ce_finish (see ce_anchor_fold_kernel); any B (planes of ceil128(B) rows; the fold zeroes the scaled attout rows
// [B, ceil32(B)), the k-rows of dE beyond the batch)
int tcar_ce_anchor_fold_o(int B, int N, int group_width, int ngroups, const float* stats, const float* lab_logit, const int32_t* label,
                          float* rowstat, float* ce, float* scale2, void* dl_hi, int64_t inner, const void* ap_hi, const void* ap_lo,
                          void* aps_hi, int ap_cols, int64_t ap_inner, void* stream, TcarOpt* o) {
  (void)o;
  if (B <= 0) return TCAR_OK;
  if (!ce_grouped_ok(N, group_width, ngroups, stats, rowstat, label, dl_hi, inner) || !lab_logit || !ce || ((uintptr_t)stats & 7) ||
      !ce_attout_ok(ap_hi, ap_lo, aps_hi, ap_cols, ap_inner, scale2))
    return TCAR_E_ARG;
  TCAR_LAUNCH(ce_anchor_fold_kernel, dim3((((B + 31) & ~31) + 3) / 4), dim3(256), 0, (hipStream_t)stream, B, N, (int)(inner >> 5), ngroups, stats, lab_logit,
              label, rowstat, ce, scale2, (__bf16*)dl_hi, (const __bf16*)ap_hi, (const __bf16*)ap_lo, (__bf16*)aps_hi, ap_cols,
              (int)(ap_inner >> 5));
  TCAR_CHECK_LAUNCH();
  return TCAR_OK;
}
extern "C" int tcar_ce_anchor_fold(int B, int N, int group_width, int ngroups, const float* stats, const float* lab_logit,
                                   const int32_t* label, float* rowstat, float* ce, float* scale2, void* dl_hi, int64_t inner,
                                   const void* ap_hi, const void* ap_lo, void* aps_hi, int ap_cols, int64_t ap_inner, void* stream) {
  return tcar_ce_anchor_fold_o(B, N, group_width, ngroups, stats, lab_logit, label, rowstat, ce, scale2, dl_hi, inner, ap_hi, ap_lo,
                               aps_hi, ap_cols, ap_inner, stream, nullptr);
}

int tcar_ce_anchor_apply_o(int B, int N, const float* rowstat, const int32_t* label, int lab_off, void* dl_hi, int64_t inner,
                           const void* ap_hi, const void* ap_lo, void* aps_hi, int ap_cols, int64_t ap_inner, float* scale2, void* stream) {
  if (B <= 0) return TCAR_OK;
  if (!ce_plane_ok(N, label, dl_hi, inner) || !rowstat || !ce_attout_ok(ap_hi, ap_lo, aps_hi, ap_cols, ap_inner, scale2)) return TCAR_E_ARG;
  TCAR_LAUNCH(ce_anchor_apply_kernel, dim3((((B + 31) & ~31) + 3) / 4), dim3(256), 0, (hipStream_t)stream, B, N, (int)(inner >> 5), rowstat, label, lab_off,
              scale2, (__bf16*)dl_hi, (const __bf16*)ap_hi, (const __bf16*)ap_lo, (__bf16*)aps_hi, ap_cols, (int)(ap_inner >> 5));
  TCAR_CHECK_LAUNCH();
  return TCAR_OK;
}

// the epilogue's per-group pairs -> out3[b] of this shard's columns (tcar_softmax_stats without the logits), to be combined by
// tcar_softmax_combine / tcar_softmax_combine_anchored
int tcar_ce_shard_stats_a(int B, int ngroups, const float* stats, const float* lab_logit, const int32_t* label, int n0, int n_loc,
                          float* out3, int anchored, void* stream) {
  if (B <= 0) return TCAR_OK;
  if (ngroups <= 0 || !stats || !lab_logit || !label || !out3 || ((uintptr_t)stats & 7)) return TCAR_E_ARG;
  TCAR_LAUNCH(ce_shard_stats_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, B, ngroups, stats, lab_logit, label, n0,
              n_loc, out3, anchored);
  TCAR_CHECK_LAUNCH();
  return TCAR_OK;
}
