// Warm start (include/tcar_warm.h): the item row of a cold catalog row as the cosine-weighted mean of the item rows of its content
// neighbours.  tcar_rows_blend is the one new kernel; tcar_warm_step runs tcar_similar_step -> tcar_rows_blend -> tcar_catalog_update.
//
// Shape: a gather of up to 64 whole rows per destination, nothing to reuse between destinations, so it is bound by the latency of the
// row reads.  One wave owns one destination row, a 256-thread workgroup four, the grid follows U (the shape of catalog_update_kernel).
// A lane owns 4 consecutive columns: one 16-byte load per donor and lane, and a wave pass covers 256 columns (H = 250 at ld 256: one
// pass).  Lane j decodes slot j of the list once (k <= 64 = one wave); the live slots are a 64-bit ballot that every pass walks from
// its lowest bit up, so the fma chain runs j ascending and an empty slot costs nothing; index and weight of a slot reach the wave as
// scalars (readlane by a wave-uniform lane).  The loads of WB_DEPTH = 8 donors are issued before the first fma waits for one; the
// chain of W rides in the same loop.  Plain vector loads and stores only, no LDS, no atomics.
#include "tcar_common.h"
#include "../../include/tcar_warm.h"

namespace {

constexpr int WB_DEPTH = 8;                 // donor rows in flight per lane: 8 float4 = 32 VGPRs

struct BlendArgs {
  int U, k, N, H;
  const int32_t* nbr; const float* sim; float min_sim;
  const float* table; long ldt;
  float* out; long ldo;
  int32_t* support; float* wsum;
};

// MODE 0: scalar loads and stores (any alignment, any ld).  MODE 1: 16-byte loads and stores, H % 4 == 0.  MODE 2: 16-byte loads and
// stores, H % 4 != 0: the H % 4 columns behind the last whole float4 of a table row are read as scalars BESIDE the float4s — lane i of
// the wave keeps the chain of column (H & ~3) + i — and reach the lane that stores them by a shuffle, so no column >= H of the table is
// read and no load sits under a lane-divergent branch: every load of a batch is unconditional (a lane without a live column reads
// columns the wave reads anyway and drops them), which is what lets all of them be in flight at once.
template <int MODE>
__global__ __launch_bounds__(256) void rows_blend_kernel(const BlendArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long u = (long)blockIdx.x * 4 + wave;
  if (u >= a.U) return;                                   // (per wave; no barrier follows)
  int n = -1;
  float s = 0.f;
  if (lane < a.k) {
    n = a.nbr[u * a.k + lane];
    s = a.sim[u * a.k + lane];
  }
  const float w = n >= 0 && n < a.N && s > 0.f && s >= a.min_sim ? s : 0.f;       // (a NaN s fails s > 0)
  const unsigned long long live = __ballot(w > 0.f);
  const int S = __popcll(live);
  const int H = a.H, H4 = H & ~3, rem = H - H4;
  const long width = MODE ? a.ldo : H;                    // the columns of out this call writes
  const int tcol = H4 + (lane < rem ? lane : rem - 1);    // MODE 2: the tail column this lane reads (lanes >= rem: the last one again)
  float* const orow = a.out + u * a.ldo;

  float W = 0.f;
  for (long c0 = 0; c0 < width; c0 += 256) {
    const long c = c0 + lane * 4;
    const bool full = c + 4 <= H;
    const long cc = full ? c : 0;                         // MODE 1, 2: H >= 4, so columns 0 .. 3 exist
    const long k0 = c < H ? c : H - 1, k1 = c + 1 < H ? c + 1 : H - 1, k2 = c + 2 < H ? c + 2 : H - 1, k3 = c + 3 < H ? c + 3 : H - 1;
    float4 acc = zero4();
    float tacc = 0.f;
    W = 0.f;                                              // (every pass adds the same chain: the same bits)
    unsigned long long m = live;
    int j = 0;
    for (int t = 0; t < S; t += WB_DEPTH) {
      float4 v[WB_DEPTH];
      float tl[WB_DEPTH], wj[WB_DEPTH];
#pragma unroll
      for (int i = 0; i < WB_DEPTH; ++i) {                // the loads of eight donors; past the last live slot: its row again, weight 0
        const bool on = m != 0ull;
        j = on ? __ffsll((long long)m) - 1 : j;
        m &= m - 1;                                       // (0 stays 0)
        const float* row = a.table + (long)__builtin_amdgcn_readlane(n, j) * a.ldt;
        wj[i] = on ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), j)) : 0.f;
        v[i] = MODE ? ld4(row + cc) : make_float4(row[k0], row[k1], row[k2], row[k3]);
        tl[i] = MODE == 2 ? row[tcol] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < WB_DEPTH; ++i) {                // j ascending; a pad (wave-uniform) leaves every chain as it is
        const bool on = wj[i] > 0.f;
        acc.x = on ? fmaf(wj[i], v[i].x, acc.x) : acc.x;
        acc.y = on ? fmaf(wj[i], v[i].y, acc.y) : acc.y;
        acc.z = on ? fmaf(wj[i], v[i].z, acc.z) : acc.z;
        acc.w = on ? fmaf(wj[i], v[i].w, acc.w) : acc.w;
        if (MODE == 2) tacc = on ? fmaf(wj[i], tl[i], tacc) : tacc;
        W += wj[i];                                       // (a pad adds +0 to W > 0)
      }
    }
    float4 r = S ? make_float4(acc.x / W, acc.y / W, acc.z / W, acc.w / W) : zero4();
    if (MODE == 2) {                                      // the lane that owns columns H4 .. H4 + 3 takes the tail chains of lanes 0 .. 2
      const float tr = S ? tacc / W : 0.f;
      const float e0 = __shfl(tr, 0), e1 = __shfl(tr, 1), e2 = __shfl(tr, 2);
      if (c == H4) r = make_float4(e0, e1, e2, 0.f);      // (columns >= H are masked below)
    }
    if (MODE) {
      if (c < width) st4(orow + c, make_float4(c < H ? r.x : 0.f, c + 1 < H ? r.y : 0.f, c + 2 < H ? r.z : 0.f, c + 3 < H ? r.w : 0.f));
    } else {
      if (c < H) orow[c] = r.x;
      if (c + 1 < H) orow[c + 1] = r.y;
      if (c + 2 < H) orow[c + 2] = r.z;
      if (c + 3 < H) orow[c + 3] = r.w;
    }
  }
  if (lane == 0) {
    a.support[u] = S;
    a.wsum[u] = W;                                        // (+0 where S == 0: width >= 1, so a pass ran)
  }
}

bool bad4(const void* p) { return !p || ((uintptr_t)p & 3); }
bool bad_min_sim(float x) { return !(x >= 0.f && x <= 1.f); }

// everything tcar_rows_blend checks; launch == false: the checks alone
int rows_blend(int U, int k, int N, int H, const int32_t* nbr, const float* sim, float min_sim, const float* table, int64_t ld_table,
               float* out, int64_t ld_out, int32_t* support, float* wsum, void* stream, bool launch) {
  if (U < 0 || k < 1 || k > 64 || N < 1 || H < 1 || bad_min_sim(min_sim)) return TCAR_E_ARG;
  if (bad4(nbr) || bad4(sim) || bad4(table) || bad4(out) || bad4(support) || bad4(wsum)) return TCAR_E_ARG;
  if (ld_table < H || ld_out < H || ld_table > 0x7fffffffL || ld_out > 0x7fffffffL) return TCAR_E_ARG;
  const int vec = H >= 4 && tcar_aligned16(table) && tcar_aligned16(out) && !(ld_table & 3) && !(ld_out & 3);
  if (U > 0) {                                            // out may not overlap the rows of table
    const uintptr_t t0 = (uintptr_t)table, t1 = t0 + 4 * ((uintptr_t)(N - 1) * (uintptr_t)ld_table + (uintptr_t)H);
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + 4 * ((uintptr_t)(U - 1) * (uintptr_t)ld_out + (uintptr_t)(vec ? ld_out : H));
    if (o0 < t1 && t0 < o1) return TCAR_E_ARG;
  }
  if (U == 0 || !launch) return TCAR_OK;
  BlendArgs a{};
  a.U = U; a.k = k; a.N = N; a.H = H;
  a.nbr = nbr; a.sim = sim; a.min_sim = min_sim;
  a.table = table; a.ldt = (long)ld_table; a.out = out; a.ldo = (long)ld_out;
  a.support = support; a.wsum = wsum;
  const dim3 grid((unsigned)(((long)U + 3) / 4)), block(256);
  if (!vec) TCAR_LAUNCH(rows_blend_kernel<0>, grid, block, 0, (hipStream_t)stream, a);
  else if (!(H & 3)) TCAR_LAUNCH(rows_blend_kernel<1>, grid, block, 0, (hipStream_t)stream, a);
  else TCAR_LAUNCH(rows_blend_kernel<2>, grid, block, 0, (hipStream_t)stream, a);
  TCAR_CHECK_LAUNCH();
  return TCAR_OK;
}

}  // namespace

extern "C" int tcar_warm_abi_version(void) { return TCAR_WARM_ABI_VERSION; }

extern "C" int tcar_rows_blend(int U, int k, int N, int H, const int32_t* nbr, const float* sim, float min_sim, const float* table,
                               int64_t ld_table, float* out, int64_t ld_out, int32_t* support, float* wsum, void* stream) {
  return rows_blend(U, k, N, H, nbr, sim, min_sim, table, ld_table, out, ld_out, support, wsum, stream, true);
}

extern "C" int tcar_warm_step(const tcar_ctx_t* c, const tcar_warm_t* w, void* stream) {
  if (!c || !w || w->U < 0 || !w->serve) return TCAR_E_ARG;
  const tcar_serve_t* s = w->serve;
  const tcar_dims_t& d = c->d;
  const int U = w->U;
  // ---- every argument error of the three calls, before the first launch
  // the lists (tcar_similar_step)
  if (bad4(w->ids) || bad4(w->xq) || bad4(w->rq) || !s->topk || !s->score || !s->state) return TCAR_E_ARG;
  if (s->k < 1 || s->k > SEL_MAX_K || s->panel <= 0 || (s->panel & 127) || s->panel > SEL_MAX_N) return TCAR_E_ARG;
  if (!s->panel_buf || !tcar_aligned16(s->panel_buf) || !s->excl || s->X < U || s->X < 1) return TCAR_E_ARG;      // (excl names every id)
  if (s->state_bytes < tcar_select_state_bytes(U, s->k)) return TCAR_E_ARG;
  if (w->window && (!w->window->key || !w->window->lo || !w->window->hi)) return TCAR_E_ARG;
  // the context (tcar_catalog_update with item rows)
  if (d.n_items <= 0 || d.H <= 0 || d.Ht <= 0 || d.ldh < d.H || d.ldt < d.Ht || (d.ldh & 63) || d.ldh > 512 ||
      (d.ldt != 64 && d.ldt != 128 && d.ldt != 256))
    return TCAR_E_ARG;
  if (!c->E || !tcar_aligned16(c->E)) return TCAR_E_ARG;
  if (c->scoring && (!c->e16h || !c->e16l || !tcar_aligned16(c->e16h) || !tcar_aligned16(c->e16l))) return TCAR_E_ARG;
  if (w->zero_moments && (!c->Mi || !c->Vi || !tcar_aligned16(c->Mi) || !tcar_aligned16(c->Vi))) return TCAR_E_ARG;
  if (!w->rows || !tcar_aligned16(w->rows) || w->ld_rows < d.H || (w->ld_rows & 3)) return TCAR_E_ARG;
  // the blend
  const int64_t ek = 2 * (int64_t)d.ldh + 5 * (int64_t)d.ldt;
  if (const int rc = rows_blend(U, s->k, d.n_items, d.H, s->topk, s->score, w->min_sim, c->E, ek, w->rows, w->ld_rows, w->support, w->wsum,
                                stream, false))
    return rc;
  if (U == 0) return TCAR_OK;

  tcar_similar_t q{};
  q.qid = w->ids; q.xq = w->xq; q.rq = w->rq;
  if (const int rc = tcar_similar_step(c, U, &q, s, w->window, nullptr, stream)) return rc;
  if (const int rc = rows_blend(U, s->k, d.n_items, d.H, s->topk, s->score, w->min_sim, c->E, ek, w->rows, w->ld_rows, w->support, w->wsum,
                                stream, true))
    return rc;
  tcar_catalog_update_t up{};
  up.U = U; up.ids = w->ids; up.item = w->rows; up.ld_item = w->ld_rows; up.zero_moments = w->zero_moments;
  return tcar_catalog_update(c, &up, stream);
}
