"""The Python-sequenced op-level step: one C call per kernel of include/tcar_hip.h, fp32 scoring only.

The product path is the C++ step driver (engine.py); this is the same step with every launch visible from Python — the call order
of INTEGRATION.md, the non-native branches of `TcarEngine` (`eng.native = False`) and `dp.DPEngine`.  A mixin of `TcarEngine`: it
reads the engine's state, tables and workspace and owns none of its own.
"""
from __future__ import annotations

import ctypes as C

from . import _lib
from ._lib import Batch, GemmDesc, Segments, check


class OpLevelStep:
    def gemm(self, layout, M, N, K, A, lda, Bm, ldb, Cm, ldc, bias=None, act=0, beta=0, splitk=1):
        check(self.lib.tcar_gemm_f32(layout, M, N, K, A, lda, Bm, ldb, Cm, ldc, bias, act, beta, splitk,
                                     self._stream()), "tcar_gemm_f32")

    @staticmethod
    def desc(M, N, segs, Cm, ldc, bias=None, act=0, beta=0, splitk=1, atomic=0) -> GemmDesc:
        """One problem of a grouped GEMM; segs = [(A, lda, B, ldb, K), ...] accumulate into one C."""
        d = GemmDesc()
        d.nseg = len(segs)
        for i, (A, lda, Bm, ldb, K) in enumerate(segs):
            d.A[i], d.lda[i], d.B[i], d.ldb[i], d.K[i] = A.value, lda, Bm.value, ldb, K
        d.C, d.ldc, d.bias = Cm.value, ldc, (bias.value if bias is not None else None)
        d.M, d.N, d.act, d.beta, d.splitk, d.atomic = M, N, act, beta, splitk, atomic
        return d

    def ggemm(self, layout, descs):
        arr = (GemmDesc * len(descs))(*descs)
        check(self.lib.tcar_gemm_f32_grouped(layout, len(descs), arr, self._stream()), "tcar_gemm_f32_grouped")

    def rows_blend(self, nbr, sim, table, min_sim: float = 0.0):
        """tcar_rows_blend (include/tcar_warm.h) on its own: for U neighbour lists (nbr int32 [U, k], sim f32 [U, k], k <= 64; a
        slot < 0 or >= N is empty) the cosine-weighted mean of the named rows of `table` (f32 [N, H], any row stride) ->
        (rows f32 [U, H], support int32 [U], wsum f32 [U]), new device tensors.  Op-level: it allocates its results."""
        import torch
        U, k = (int(x) for x in nbr.shape)
        N, H = (int(x) for x in table.shape)
        ldo = (H + 3) // 4 * 4
        out = torch.empty(U, ldo, dtype=torch.float32, device=table.device)
        support = torch.empty(U, dtype=torch.int32, device=table.device)
        wsum = torch.empty(U, dtype=torch.float32, device=table.device)
        nbr, sim = nbr.contiguous(), sim.contiguous()
        check(self.lib.tcar_rows_blend(U, k, N, H, nbr.data_ptr(), sim.data_ptr(), float(min_sim), table.data_ptr(), int(table.stride(0)),
                                       out.data_ptr(), ldo, support.data_ptr(), wsum.data_ptr(), self._stream()), "tcar_rows_blend")
        return out[:, :H], support, wsum

    # --------------------------------------------------------------------------------------------- forward
    def forward(self, bt: Batch):
        """model_combine.py:52-138 up to the full-catalog logits (Python-sequenced op-level path, fp32 scoring only;
        the bf16 scoring modes are sequenced by the C++ step driver)."""
        if self.scoring_code:
            raise _lib.TcarError("the Python-sequenced op-level path supports scoring='f32' only")
        g, lib, st = self.geo, self.lib, self._stream()
        B, T = bt.B, bt.T
        BT = B * T
        self._ensure_work(B, T)
        p = self._p
        if self._time_dirty:
            check(lib.tcar_cand_time_fwd(C.byref(self.dims), C.byref(self._time_ptrs()), p(self.mwdhm), p(self.E), st),
                  "tcar_cand_time_fwd")
            self._time_dirty = False
        tab = self._tables()
        check(lib.tcar_gather_clip_fwd(C.byref(self.dims), C.byref(tab), C.byref(bt), p(self.x_icp), p(self.x_pt),
                                       p(self.x_act), p(self.click_t), st), "tcar_gather_clip_fwd")
        # one grouped launch:  pre1 = X_ic W_in + X_c W_c + X_act W_int (modules.py:126-131),
        # pre2 = X_pt W'_in + X_c W'_c (modules.py:94-96), q1 = relu(click_t Wq1 + b) (modules.py:138)
        D = self.desc
        x_c = p(self.x_icp, g.ldh)
        self.ggemm(0, [
            D(BT, g.ldh, [(p(self.x_icp), g.ic, self._w("m_win"), g.ldh, g.ic), (x_c, g.ic, self._w("m_wc"), g.ldh, g.ldh),
                          (p(self.x_act), g.ldt, self._w("m_wint"), g.ldh, g.ldt)], p(self.pre1), g.ldh),
            D(BT, g.ldh, [(p(self.x_pt), g.pt, self._w("s_win"), g.ldh, g.pt), (x_c, g.ic, self._w("s_wc"), g.ldh, g.ldh)],
              p(self.pre2), g.ldh),
            D(B, g.ldh, [(p(self.click_t), g.ct, self._w("q1_w"), g.ldh, g.ct)], p(self.q1), g.ldh,
              bias=self._w("q1_b"), act=1)])
        # q = tanh(q1 Wq2 + b)                           (modules.py:139)
        self.ggemm(0, [D(B, g.ic, [(p(self.q1), g.ldh, self._w("q2_w"), g.ic, g.ldh)], p(self.q), g.ic,
                         bias=self._w("q2_b"), act=2)])
        check(lib.tcar_attn_pool_fwd(C.byref(self.dims), B, T, p(self.x_icp), p(self.x_pt), p(self.pre1), p(self.pre2),
                                     p(self.q), self._w("m_wres"), self._w("s_wres"), p(self.pooled), p(self.alpha),
                                     st), "tcar_attn_pool_fwd")
        # attout = [tanh(pooled_ic W_o + b) | tanh(pooled_t W'_o + b)]   (model_combine.py:119,127,132)
        self.ggemm(0, [
            D(B, g.ic, [(p(self.pooled), g.ek, self._w("o_w"), g.ic, g.ic)], p(self.attout), g.ek,
              bias=self._w("o_b"), act=2),
            D(B, g.pt, [(p(self.pooled, g.ic), g.ek, self._w("ot_w"), g.pt, g.pt)], p(self.attout, g.ic), g.ek,
              bias=self._w("ot_b"), act=2)])
        # logits = attout E^T                              (model_combine.py:138)
        self.gemm(1, B, g.N, g.ek, p(self.attout), g.ek, p(self.E), g.ek, p(self.logits), g.Npad)

    # -------------------------------------------------------------------------------------------- backward
    def backward(self, bt: Batch):
        """Loss (model_combine.py:142-147) and the gradient of its SUM w.r.t. all 23 variables."""
        self.backward_local(bt)
        lib, st, p = self.lib, self._stream(), self._p
        # clip norm of the dense item block BEFORE the sparse rows are scattered in
        self._sqnorm_item()
        tab, gr = self._tables(), self._grads()
        check(lib.tcar_gather_clip_bwd(C.byref(self.dims), C.byref(tab), C.byref(bt), p(self.dx_icp), p(self.dx_pt),
                                       p(self.dx_act), p(self.dclick), C.byref(gr), st), "tcar_gather_clip_bwd")
        self._cand_time_bwd()
        self._sqnorm_dense()

    def _sqnorm_item(self):
        g = self.geo
        one = Segments()
        one.nseg = 1
        one.off[0], one.len[0], one.slot[0] = 0, g.N * g.ldh, self.slot_item
        check(self.lib.tcar_sqnorm(self._p(self.Gi), C.byref(one), self._p(self.sqn_dense), self._stream()), "tcar_sqnorm")

    def _cand_time_bwd(self):
        gr = self._grads()
        check(self.lib.tcar_cand_time_bwd_indexed(C.byref(self.dims), C.byref(self._time_ptrs()), self._p(self.inv_n),
                                                  self._p(self.inv_off), self._p(self.d_et), int(self.scoring_code != 0),
                                                  self._p(self.ct_ws), C.byref(gr), self._stream()),
              "tcar_cand_time_bwd_indexed")

    def _sqnorm_dense(self):
        check(self.lib.tcar_sqnorm(self._p(self.G), C.byref(self.segs_dense), self._p(self.sqn_dense), self._stream()),
              "tcar_sqnorm")

    def backward_local(self, bt: Batch):
        """Everything of the backward pass that needs no other rank: loss, dlogits, dE, input / weight gradients."""
        g, lib, st = self.geo, self.lib, self._stream()
        B, T, K = bt.B, bt.T, bt.K
        BT = B * T
        p = self._p
        self.Gx.zero_()               # tables, bias, weight gradients and norm pieces are accumulated with atomics
        self.sqn_dense.zero_()
        check(lib.tcar_softmax_ce(B, g.N, p(self.logits), g.Npad, C.c_void_p(bt.label), p(self.ce), st), "tcar_softmax_ce")
        # d attout = dlogits E  (contraction over the catalog: split-K slabs + reduce)
        S = lib.tcar_gemm_splitk_effective(g.Npad, self.splitk)
        self.gemm(0, B, g.ek, g.Npad, p(self.logits), g.Npad, p(self.E), g.ek, p(self.slabs), g.ek, splitk=self.splitk)
        check(lib.tcar_splitk_reduce(p(self.slabs), S, B, g.ek, g.ek, p(self.dattout), st), "tcar_splitk_reduce")
        # dE = dlogits^T attout: item columns -> Gi, time columns -> d_et (content is frozen); one launch, both
        # problems stream the same dlogits tiles
        D = self.desc
        self.ggemm(2, [
            D(g.N, g.ldh, [(p(self.logits), g.Npad, p(self.attout), g.ek, B)], p(self.Gi), g.ldh),
            D(g.N, g.pt, [(p(self.logits), g.Npad, p(self.attout, g.ic), g.ek, B)], p(self.d_et), g.pt)])
        if K:
            check(lib.tcar_neg_term(C.byref(self.dims), B, K, p(self.E), C.c_void_p(bt.neg), p(self.attout),
                                    self.neg_weight, p(self.neg_fb), p(self.dattout), p(self.Gi), p(self.ce), p(self.loss),
                                    st), "tcar_neg_term")
        else:
            self.neg_fb[:B].zero_()
        # output transforms (linear_2d + tanh) backward
        check(lib.tcar_dact_colsum(B, g.ic, g.ek, p(self.attout), p(self.dattout), self._g("o_b"), 2, st), "dact")
        check(lib.tcar_dact_colsum(B, g.pt, g.ek, p(self.attout, g.ic), p(self.dattout, g.ic), self._g("ot_b"), 2, st), "dact")
        self.ggemm(1, [
            D(B, g.ic, [(p(self.dattout), g.ek, self._w("o_w"), g.ic, g.ic)], p(self.dpooled), g.ek),
            D(B, g.pt, [(p(self.dattout, g.ic), g.ek, self._w("ot_w"), g.pt, g.pt)], p(self.dpooled, g.ic), g.ek)])
        check(lib.tcar_attn_pool_bwd(C.byref(self.dims), B, T, p(self.x_icp), p(self.x_pt), p(self.pre1), p(self.pre2),
                                     p(self.q), self._w("m_wres"), self._w("s_wres"), p(self.alpha), p(self.dpooled),
                                     p(self.dx_icp), p(self.dx_pt), p(self.dq), p(self.dpre1), p(self.dpre2),
                                     self._g("m_wres"), self._g("s_wres"), st), "tcar_attn_pool_bwd")
        # query MLP backward (modules.py:138-139)
        check(lib.tcar_dact_colsum(B, g.ic, g.ic, p(self.q), p(self.dq), self._g("q2_b"), 2, st), "dact")
        self.ggemm(1, [D(B, g.ldh, [(p(self.dq), g.ic, self._w("q2_w"), g.ic, g.ic)], p(self.dq1), g.ldh)])
        check(lib.tcar_dact_colsum(B, g.ldh, g.ldh, p(self.q1), p(self.dq1), self._g("q1_b"), 1, st), "dact")
        # input gradients: click query rows and the projections (only the ITEM half of dX_ic is needed: content
        # is frozen)
        self.ggemm(1, [
            D(B, g.ct, [(p(self.dq1), g.ldh, self._w("q1_w"), g.ldh, g.ldh)], p(self.dclick), g.ct),
            D(BT, g.ldh, [(p(self.dpre1), g.ldh, self._w("m_win"), g.ldh, g.ldh)], p(self.dx_icp), g.ic, beta=1),
            D(BT, g.ldt, [(p(self.dpre1), g.ldh, self._w("m_wint"), g.ldh, g.ldh)], p(self.dx_act), g.ldt),
            D(BT, g.pt, [(p(self.dpre2), g.ldh, self._w("s_win"), g.ldh, g.ldh)], p(self.dx_pt), g.pt, beta=1)])
        # all nine weight gradients (x^T dy, K = batch rows) in one launch, split-K with fp32 atomics into the
        # zeroed gradient arena
        kb = max(1, min(16, (B + 1023) // 1024))
        kr = max(1, min(16, (BT + 1023) // 1024))
        x_c = p(self.x_icp, g.ldh)
        W = lambda M, N, A, lda, Bm, ldb, K, name, ks: D(M, N, [(A, lda, Bm, ldb, K)], self._g(name), N, splitk=max(ks, 2),
                                                          atomic=1)
        self.ggemm(2, [
            W(g.ic, g.ic, p(self.pooled), g.ek, p(self.dattout), g.ek, B, "o_w", kb),
            W(g.pt, g.pt, p(self.pooled, g.ic), g.ek, p(self.dattout, g.ic), g.ek, B, "ot_w", kb),
            W(g.ldh, g.ic, p(self.q1), g.ldh, p(self.dq), g.ic, B, "q2_w", kb),
            W(g.ct, g.ldh, p(self.click_t), g.ct, p(self.dq1), g.ldh, B, "q1_w", kb),
            W(g.ic, g.ldh, p(self.x_icp), g.ic, p(self.dpre1), g.ldh, BT, "m_win", kr),
            W(g.ldh, g.ldh, x_c, g.ic, p(self.dpre1), g.ldh, BT, "m_wc", kr),
            W(g.ldt, g.ldh, p(self.x_act), g.ldt, p(self.dpre1), g.ldh, BT, "m_wint", kr),
            W(g.pt, g.ldh, p(self.x_pt), g.pt, p(self.dpre2), g.ldh, BT, "s_win", kr),
            W(g.ldh, g.ldh, x_c, g.ic, p(self.dpre2), g.ldh, BT, "s_wc", kr)])

    # ---------------------------------------------------------------------------------------------- update
    def update(self):
        """model_combine.py:157-163: per-variable clip_by_norm(max_grad) + TF-1 Adam."""
        g, lib, st, p = self.geo, self.lib, self._stream(), self._p
        lr_t = self._lr_t()
        clip = float(self.max_grad) if self.max_grad else 0.0
        check(lib.tcar_clip_adam(p(self.W), p(self.G), p(self.M), p(self.V), C.byref(self.segs_all), p(self.sqn_dense),
                                 p(self.sqn_pieces), p(self.use_dense), clip, lr_t, self.b1, self.b2, self.eps, st),
              "tcar_clip_adam")
        check(lib.tcar_clip_adam_2d(p(self.E), g.ek, p(self.Gi), p(self.Mi), p(self.Vi), g.N, g.ldh, self.slot_item,
                                    p(self.sqn_dense), p(self.sqn_pieces), p(self.use_dense), clip, lr_t, self.b1,
                                    self.b2, self.eps, st), "tcar_clip_adam_2d")
        self._after_update()
