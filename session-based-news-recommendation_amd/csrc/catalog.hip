// In-place catalog updates (include/tcar_catalog.h): U named rows of a live context take new item rows, content rows, publish times,
// keys or categories, and every quantity the context derives from a catalog row is rewritten in the same launch — the fp32 image in E,
// the hi / lo bf16 planes in the KB32 layout, the clipped candidate time block, the one-hot row, the Adam moments.
//
// Shape: a scatter of whole rows.  One wave owns one row, a 256-thread workgroup four rows, the grid follows U.  A lane owns 8
// consecutive columns: two float4 stores into E and ONE 16-byte piece per plane (kb32_off with k % 8 == 0 addresses a whole piece), so a
// wave pass writes 64 pieces of 16 bytes per plane and 2 KB of E.  Plain vector stores only.
//
// The clipped time rows: a catalog row names five of the 139 table rows.  They are clipped on the fly inside the row's wave — an
// aligned group of ldt / 4 lanes per table row, clip_time_piece of tcar_common.h, the code and the reduction order of
// cand_time_fwd_kernel — and pass through 5 ldt floats of LDS per wave to change owner from 4 columns per lane to 8.  Staging all
// 139 rows per workgroup, as the whole-catalog refresh does, would read and clip 139 rows for four catalog rows: 28 times the five a
// wave needs, at every U (the grid follows U, so the share per workgroup never grows).
//
// Ownership (include/tcar_catalog_shard.h): the kernel takes the rows [n0, n0 + nl) a context OWNS.  E, the key and category tables and
// the optional whole publish-time table are indexed by the catalog row n and written for every named row; the planes, the context's
// publish times, the one-hot plane and the moments are the owner's, indexed by n - n0 and written only where n is owned.
// tcar_catalog_update is the owned form with (0, N): ONE kernel body, so both give the bytes of a rebuild by the same code.
#include "tcar_common.h"
#include "tcar_bf16_layout.h"
#include "../../include/tcar_catalog_shard.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_c;

namespace {

struct CatArgs {
  int U, N, H, ldh, ldt, planes, refresh;
  int n0, nl;                          // the rows this context owns: [n0, n0 + nl) of [0, N)
  const int32_t* ids;
  const float* item; long ld_item;
  const float* content; long ld_content;
  const int32_t* mw_new; int32_t* mw_tab;   // mw_tab: the owner's table, [nl, 5]
  int32_t* mw_all;                     // the whole [N, 5] table a rank may keep beside it, or null
  const float* tab[5];
  float* E; __bf16* eh; __bf16* el;
  const int32_t* key; int32_t* key_table;
  const int32_t* cat; int32_t* cat_table;
  float* Mi; float* Vi;
  __bf16* oh; int oh_in32;
};

// 8 consecutive fp32 values -> one 16-byte piece of each plane: hi = bf16(x), lo = bf16(x - float(hi)), as split_bf16_kernel rounds
__device__ __forceinline__ void store_planes8(__bf16* eh, __bf16* el, long o, const float4 a, const float4 b) {
  const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  bf16x8_c h, l;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    h[j] = (__bf16)v[j];
    l[j] = (__bf16)(v[j] - (float)h[j]);
  }
  *reinterpret_cast<bf16x8_c*>(eh + o) = h;
  *reinterpret_cast<bf16x8_c*>(el + o) = l;
}
// columns [w, w + 4) of a source row of H live columns (w % 4 == 0, the row 16-byte aligned and at least ceil4(H) floats long);
// columns >= H read as zero: the pad columns of E and of the planes stay zero
__device__ __forceinline__ float4 ld4_live(const float* row, int w, int H) {
  if (w >= H) return zero4();
  float4 t = ld4(row + w);
  if (w + 1 >= H) t.y = 0.f;
  if (w + 2 >= H) t.z = 0.f;
  if (w + 3 >= H) t.w = 0.f;
  return t;
}

__global__ __launch_bounds__(256) void catalog_update_kernel(const CatArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];   // [4 waves][5 ldt]: the clipped time rows of each wave's catalog row
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ldh = a.ldh, ldt = a.ldt, ic = 2 * ldh, pt = 5 * ldt, ek = ic + pt, in32 = ek >> 5;
  const long u = (long)blockIdx.x * 4 + wave;
  const int n = u < a.U ? a.ids[u] : -1;
  const bool live = n >= 0 && n < a.N;            // (an id outside the catalog names no row: nothing is read or written for it)
  const bool own = live && n >= a.n0 && n - a.n0 < a.nl;      // (per wave: the planes, publish times, one-hot row and moments are the owner's)
  const int r = own ? n - a.n0 : 0;               // the row in the owner's buffers
  float* const Erow = a.E + (long)(live ? n : 0) * ek;

  // item | content rows -> E and the planes
  if (live && (a.item || a.content)) {
    for (int c = lane * 8; c < ic; c += 512) {
      const bool second = c >= ldh;
      const float* src = second ? a.content : a.item;
      if (!src) continue;
      const int w = second ? c - ldh : c;
      const float* row = src + u * (second ? a.ld_content : a.ld_item);
      const float4 t0 = ld4_live(row, w, a.H), t1 = ld4_live(row, w + 4, a.H);
      st4(Erow + c, t0);
      st4(Erow + c + 4, t1);
      if (a.planes && own) store_planes8(a.eh, a.el, kb32_off(r, c, in32), t0, t1);
    }
  }

  // the row's publish time: the new entry where the call brings one (and then the context's table follows), else the table's
  int id[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int raw = !own ? 0 : a.mw_new ? a.mw_new[u * 5 + k] : a.mw_tab ? a.mw_tab[(long)r * 5 + k] : 0;
    id[k] = clampi(raw, 0, time_vocab(k) - 1);
  }
  if (live && a.mw_new && lane < 5) {
    const int32_t v = a.mw_new[u * 5 + lane];
    if (own) a.mw_tab[(long)r * 5 + lane] = v;
    if (a.mw_all) a.mw_all[(long)n * 5 + lane] = v;
  }

  // clipped time block: clip the five table rows in groups of ldt / 4 lanes, hand them over through LDS, store 8 columns per lane —
  // into E on an fp32 context, into the planes alone on a plane context (the destinations of tcar_cand_time_fwd_bf16 in step.hip)
  if (a.refresh) {                                // (uniform over the grid: every thread reaches the barrier, a wave that owns nothing too)
    float* const my = lds + wave * pt;
    const int sub = ldt >> 2, gpw = 64 / sub;
    const int grp = lane / sub, lin = lane - grp * sub;
    for (int k0 = 0; k0 < 5; k0 += gpw) {
      const int k = k0 + grp;
      const bool valid = own && k < 5;
      const int kk = k < 5 ? k : 0;
      const float4 x = valid ? ld4(pick5(a.tab, kk) + (long)pick5(id, kk) * ldt + lin * 4) : zero4();
      const float4 y = clip_time_piece(x, sub);
      if (valid) st4(my + kk * ldt + lin * 4, y);
    }
    __syncthreads();
    if (own) {                                    // (an fp32 context owns the whole catalog: r == n, Erow is row n)
      for (int c = lane * 8; c < pt; c += 512) {
        const float4 t0 = ld4(my + c), t1 = ld4(my + c + 4);
        if (a.planes) store_planes8(a.eh, a.el, kb32_off(r, ic + c, in32), t0, t1);
        else {
          st4(Erow + ic + c, t0);
          st4(Erow + ic + c + 4, t1);
        }
      }
    }
  }
  if (!live) return;
  if (lane == 0) {                                // the whole tables every rank keeps
    if (a.key) a.key_table[n] = a.key[u];
    if (a.cat) a.cat_table[n] = a.cat[u];
  }
  if (!own) return;

  // the one-hot row of tcar_time_onehot: ones at the five time rows and at the anchor columns 139 .. 146, zeros elsewhere
  if (a.oh && a.mw_new) {
    for (int c = lane * 8; c < 160; c += 512) {
      bf16x8_c o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int col = c + j;
        bool one = col >= 139 && col < 139 + TCAR_ANCHOR_COLS;
#pragma unroll
        for (int k = 0; k < 5; ++k) one = one || col == time_rowoff(k) + id[k];
        o[j] = (__bf16)(one ? 1.0f : 0.0f);
      }
      *reinterpret_cast<bf16x8_c*>(a.oh + kb32_off(r, c, a.oh_in32)) = o;
    }
  }
  // a replaced row has no optimizer history
  if (a.Mi) {
    for (int c = lane * 4; c < ldh; c += 256) {
      st4(a.Mi + (long)r * ldh + c, zero4());
      st4(a.Vi + (long)r * ldh + c, zero4());
    }
  }
}

// the context's dimensions as every launcher of the core checks them (embed.hip: check_dims)
bool bad_dims(const tcar_dims_t& d) {
  return d.n_items <= 0 || d.H <= 0 || d.Ht <= 0 || d.ldh < d.H || d.ldt < d.Ht || (d.ldh & 63) || d.ldh > 512 ||
         (d.ldt != 64 && d.ldt != 128 && d.ldt != 256);
}
bool bad_table(const float* p, int64_t ld, int H) { return p && (!tcar_aligned16(p) || ld < H || (ld & 3)); }

// both entry points: the rows [n0, n0 + n_loc) of the context's catalog are owned (sharded: the shard-local layout of
// tcar_catalog_shard.h; whole: (0, N), where it is the layout of tcar_catalog.h)
int update_rows(const tcar_ctx_t* c, const tcar_catalog_update_t* u, bool sharded, int32_t n0, int32_t n_loc, int32_t* mwdhm_all,
                void* stream) {
  if (!c || !u || u->U < 0) return TCAR_E_ARG;
  if (u->U == 0) return TCAR_OK;
  // the descriptor
  if (!u->ids) return TCAR_E_ARG;
  if (!u->item && !u->content && !u->mwdhm && !u->key && !u->cat) return TCAR_E_ARG;
  if (bad_table(u->item, u->ld_item, c->d.H) || bad_table(u->content, u->ld_content, c->d.H)) return TCAR_E_ARG;
  if (!u->key != !u->key_table || !u->cat != !u->cat_table) return TCAR_E_ARG;
  if (u->refresh_time && !u->mwdhm && !c->mwdhm) return TCAR_E_ARG;
  if (u->onehot && ((u->onehot_inner & 31) || u->onehot_inner < 160 || !tcar_aligned16(u->onehot))) return TCAR_E_ARG;
  // the context
  if (bad_dims(c->d) || !c->E || !tcar_aligned16(c->E)) return TCAR_E_ARG;
  if (c->scoring && (!c->e16h || !c->e16l || !tcar_aligned16(c->e16h) || !tcar_aligned16(c->e16l))) return TCAR_E_ARG;
  if (u->mwdhm && !c->mwdhm) return TCAR_E_ARG;
  if (u->zero_moments && (!c->Mi || !c->Vi || !tcar_aligned16(c->Mi) || !tcar_aligned16(c->Vi))) return TCAR_E_ARG;
  if (u->refresh_time && (!c->W || !tcar_aligned16(c->W))) return TCAR_E_ARG;
  // the shard
  if (sharded && (!c->scoring || n0 < 0 || n_loc <= 0 || (long)n0 + n_loc > c->d.n_items)) return TCAR_E_ARG;
  if (!sharded) { n0 = 0; n_loc = c->d.n_items; }

  CatArgs a{};
  a.n0 = n0; a.nl = n_loc; a.mw_all = mwdhm_all;
  a.U = u->U; a.N = c->d.n_items; a.H = c->d.H; a.ldh = c->d.ldh; a.ldt = c->d.ldt;
  a.planes = c->scoring != 0; a.refresh = u->refresh_time != 0;
  a.ids = u->ids;
  a.item = u->item; a.ld_item = (long)u->ld_item;
  a.content = u->content; a.ld_content = (long)u->ld_content;
  a.mw_new = u->mwdhm; a.mw_tab = const_cast<int32_t*>(c->mwdhm);
  for (int k = 0; k < 5; ++k) {
    a.tab[k] = a.refresh ? c->W + c->off[TCAR_V_MONTH + k] : nullptr;
    if (a.refresh && (c->off[TCAR_V_MONTH + k] & 3)) return TCAR_E_ARG;      // (the table rows are read as float4)
  }
  a.E = c->E; a.eh = (__bf16*)c->e16h; a.el = (__bf16*)c->e16l;
  a.key = u->key; a.key_table = u->key_table; a.cat = u->cat; a.cat_table = u->cat_table;
  if (u->zero_moments) { a.Mi = c->Mi; a.Vi = c->Vi; }
  a.oh = (__bf16*)u->onehot; a.oh_in32 = (int)(u->onehot_inner >> 5);
  const size_t lds = a.refresh ? (size_t)4 * 5 * a.ldt * sizeof(float) : 0;      // at most 20 KB (ldt = 256)
  const unsigned grid = (unsigned)(((long)u->U + 3) / 4);
  TCAR_LAUNCH(catalog_update_kernel, dim3(grid), dim3(256), lds, (hipStream_t)stream, a);
  TCAR_CHECK_LAUNCH();
  return TCAR_OK;
}

}  // namespace

extern "C" int tcar_catalog_abi_version(void) { return TCAR_CATALOG_ABI_VERSION; }
extern "C" int tcar_catalog_shard_abi_version(void) { return TCAR_CATALOG_SHARD_ABI_VERSION; }

extern "C" int tcar_catalog_update(const tcar_ctx_t* c, const tcar_catalog_update_t* u, void* stream) {
  return update_rows(c, u, false, 0, 0, nullptr, stream);
}

extern "C" int tcar_catalog_update_owned(const tcar_ctx_t* c, const tcar_catalog_update_t* u, int32_t n0, int32_t n_loc,
                                         int32_t* mwdhm_all, void* stream) {
  return update_rows(c, u, true, n0, n_loc, mwdhm_all, stream);
}
