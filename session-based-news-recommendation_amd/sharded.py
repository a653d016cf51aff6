"""Catalog-sharded data-parallel TCAR step ("catalog-sharded scoring"): one process per GPU,
torch.distributed ("nccl" = RCCL over xGMI).  No reference equivalent — the reference is single process.

The replica exchange of dp.py moves the dense item-table gradient and the candidate-time block of dE through an all-reduce
(106 MB per step and rank at the Globo size).  Here rank r OWNS the catalog rows [n0_r, n0_r + S) of the candidate side —
their bf16 planes, their gradient, their Adam moments — and scores them against the sessions of EVERY rank:

  session forward (local B sessions)   gather, projections, pools, output transforms           -> attout [B, ek]
  all-gather   ONE packed row per session: [attout | label | negative-term coefficient | negatives]    -> [W*B, ld]
  scoring      logits = attout_all . E_shard^T  [W*B, S];  per-shard softmax statistics
  all-gather   (max, sum exp, label logit) per session and shard -> lse, cross entropy          (3 floats per session)
  gradients    dlogits planes;  dE_shard = dlogits^T attout_all (item block | time block) STAYS LOCAL;
               dX_partial = dlogits . E_shard [W*B, ek]
  reduce-scatter dX_partial over the ranks                                                     -> dattout of the local sessions
  session backward (local)            ... -> (id, row) item-row gradients of the local sessions
  all-gather   packed [row | id] item-row gradients; every owner keeps the rows of its shard
  all-reduce   arena gradients + IndexedSlices norm pieces (+ the shards' dense item norms)     (5 MB)
  update       clip + Adam: arena on every rank (identical inputs, dense norms summed in a fixed order: identical bits,
               no broadcast), item rows by their owner
  all-gather   the updated item rows [S, ldh] -> every rank's E (the session-side gathers of the next step read any row)

Per step and rank at W = 8, B = 512, N = 46,033: ~14 MB attout + ~14 MB dX + ~9 MB rows + 5 MB arena + 47 MB item rows
received, against 2 x 106 MB through the replica all-reduce; the candidate-side memory (planes, gradient, moments: 0.5 GB
at this size, 130 GB at 10 M items) divides by W.  The clip semantics of DESIGN.md S5 hold exactly: the dense item norm is
the sum of the shards' norms of (scoring + densified negative part), taken BEFORE the gathered rows are scattered in.
Six collectives per step (eleven before the exchange buffers were packed): at ~20-40 us of latency each over RCCL they,
not the bytes, are what a step waits for at this catalog size.

Sequenced from C++ between the exchanges (csrc/step.hip: tcar_step_session_forward / tcar_shard_score / tcar_shard_backward /
tcar_shard_finish / tcar_step_session_backward), the collectives in between from here; split-bf16 scoring modes only.

Evaluation: `eval_step` scores the local sessions against the whole catalog on the fp32 GEMM ([B, Npad] logits on every rank).
`eval_step_streamed` / `recommend` (ShardExchange.serve, include/tcar_serve_shard.h) use the shard instead:

  session forward (local B sessions)                                                            -> attout [B, ek]
  all-gather   ONE packed row per session: [attout | label | - | window lo | window hi | exclusion ids]   -> [W*cap, ld]
  label scores attout_all . E_shard[label] where this shard owns the label, 0 elsewhere (evaluation only)
  all-gather   the shards' label scores; every session takes its label owner's entry             (1 float per session and shard)
  fold         the shard's split-bf16 planes in column panels, global item ids -> one select state per gathered session
  all-gather   the select states [W*cap, 2k + 4]; rank r merges the W states of its own sessions (tcar_select_merge), finishes

The merge is exact: top-k, scores and rank are the bits of the unsharded streamed call, the cross entropy differs by the rounding of a
sum whose order is fixed.  No [., Npad] buffer exists on any rank.

Retrieve-then-rank over the shards: `shard_retrieve` / `shard_recommend_two_stage` / `shard_score_candidates` (ShardExchange.retrieve /
.candidates, include/tcar_retrieve_shard.h).  Collectives under names of their own — the single-engine names keep refusing:

  all-gather   the packed session rows of the streamed selection; the label slot is the live marker (-1: a padding session)
  fold         the shard's HI planes alone in column panels, global item ids -> one top-C state per gathered LIVE session
  all-to-all   the states [W*cap, 2C + 4]: rank r receives rows [r cap, (r + 1) cap) of every shard's; tcar_retrieve_merge, finish
  all-gather   the shortlists [cap, C]                                              (two-stage only)
  gather       the exact score of every slot whose row this shard owns, -inf elsewhere
  all-to-all   the parts [W*cap, C]; every slot takes its OWNER's bits (tcar_cand_combine), list order, the first k

Both joins are exact: no float sum in the merge, a copy of the owner's word in the combine.  The all-to-all moves a W-th of what an
all-gather would (W = 8, cap = 512, C = 1,024: 8.4 MB into every rank instead of 67 MB).  Which path it took — RCCL's ncclAllToAll on the
step's stream, all_to_all_single of a process group, or all-gather + slice where a backend has neither (the documented fallback, not a
failure) — is `exchange_info()["all_to_all"]`.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib, dp
from ._lib import Batch, Dims, check
from .engine import CandResult, Switches, TcarEngine, _ru
from .workspace import BF16, F32, I32, ScoreForm, Spec, scoring_specs


def shard_rows(n_items: int, world: int):
    """rows per shard (a multiple of 128: the bf16 planes are blocked in 128-row units); the last shard may be short"""
    return _ru((n_items + world - 1) // world, 128)


class ShardExchange(dp.Collectives):
    """The collective schedule of the catalog-sharded step, independent of where the local pieces come from (the engine binds
    them to the HIP entry points; tests/test_sharded_gloo.py drives the SAME schedule over gloo on CPU tensors with fp64
    torch pieces).  Every rank — also one whose shard of the batch is empty — issues the same six collectives in the same
    order with buffers of the same shape:

      1 all-gather      packed session rows [cap, ld_head]                    -> [W * cap, ld_head]
      2 all-gather      softmax statistics of the shard [W * cap, 3]          -> [W, W * cap, 3]
      3 reduce-scatter  dX partial [W * cap, ek]  (all-reduce + slice where the backend has no reduce-scatter)
      4 all-gather      packed item-row gradients [cap * T, ldr]              -> [W * cap * T, ldr]
      5 all-reduce      arena gradients + norm pieces
      6 all-gather      updated item rows of the shard [S, ldh]               -> [W, S, ldh]   (update steps only)

    Collective 6 is issued asynchronously: nothing of the step that follows needs the other shards' rows before its session
    gathers, so `wait_rows()` is called at the top of the next step (and by every other reader of the item table)."""

    def step(self, pieces, cap: int, update: bool) -> None:
        """one training step; `pieces` supplies the local compute between the exchanges:
             begin() -> head [cap, ld]             score(head_all [W*cap, ld]) -> stats [W*cap, 3]
             backward(stats_all [W, W*cap, 3]) -> dx_full [W*cap, ek]         (dE of the shard stays inside)
             finish()                                                          (negative rows, shard norm, candidate-time grads)
             session_backward(dx_rows [cap, ek]) -> rows [cap*T, ldr]
             scatter(all_rows [W*cap*T, ldr])     arena() -> flat tensor      norms()
             update() -> (stage [W, S, ldh], install) or None"""
        self.order = []
        self.wait_rows()
        head = pieces.begin()
        head_all = self.all_gather(head, "attout+labels+negatives").view(self.world * cap, -1)
        stats = pieces.score(head_all)
        stats_all = self.all_gather(stats, "softmax_stats")
        dx_full = pieces.backward(stats_all)
        pieces.finish()
        dx_rows = self.reduce_scatter_rows(dx_full, cap, "dX")
        rows = pieces.session_backward(dx_rows)
        all_rows = self.all_gather(rows, "rows+ids").view(-1, rows.shape[-1])
        pieces.scatter(all_rows)
        self.all_reduce(pieces.arena(), "arena")
        pieces.norms()
        if update:
            out = pieces.update()
            if out is not None:
                self.share_rows(*out)

    def serve(self, pieces, cap: int, labelled: bool):
        """one evaluation (labelled) or recommendation step of the streamed score-and-select (include/tcar_serve_shard.h): every
        rank folds ITS shard of the catalog for the sessions of EVERY rank, and the per-shard select states merge exactly.  Every
        rank, also one without sessions, issues the same collectives in the same order with buffers of the same shape:

          1 all-gather  packed session rows [cap, ld]: [attout | label | - | window lo | window hi | X exclusion ids | pad], ints as bits
          2 all-gather  the shards' label scores [W * cap] (labelled only; each session takes its label OWNER's entry)
          3 all-gather  the shards' select states [W * cap, 2k + 4]; rank r merges rows [r cap, (r + 1) cap) of the W states

        `pieces` supplies the local compute:
             begin() -> rows [cap, ld]                     prepare(rows_all [W*cap, ld]) -> label-score parts [W*cap] (or None)
             label_scores(parts_all [W, W*cap])            fold() -> state [W*cap, 2k+4]
             finish(states [W, W*cap, 2k+4]) -> the result of the local sessions (returned)"""
        self.order = []
        self.wait_rows()
        head = pieces.begin()
        head_all = self.all_gather(head, "serve_rows").view(self.world * cap, -1)
        parts = pieces.prepare(head_all)
        if labelled:
            pieces.label_scores(self.all_gather(parts, "serve_label_scores"))
        state = pieces.fold()
        return pieces.finish(self.all_gather(state, "serve_states"))

    def retrieve(self, pieces, cap: int, rerank: bool):
        """one retrieval (a shortlist of C items from coarse scores) or, with `rerank`, one two-stage recommendation
        (include/tcar_retrieve_shard.h): every rank folds ITS shard into a top-C state per session of EVERY rank, the states merge
        exactly; then every rank scores the shortlist slots whose rows it owns and the owners' bits combine.  A rank needs only its
        own sessions' slice of every shard's result, so results travel by all-to-all (Collectives.all_to_all_rows), a W-th of an
        all-gather.  Every rank, also one without sessions, issues the same collectives in the same order with buffers of the same shape:

          1 all-gather  serve_rows: the packed session rows of `serve` [cap, ld]; the label slot carries the live marker (-1: padding)
          2 all-to-all  retrieve_states [W * cap, 2C + 4] -> [W, cap, 2C + 4]; tcar_retrieve_merge, tcar_retrieve_finish
          3 all-gather  retrieve_shortlists int32 [cap, C]                            (rerank only)
          4 all-to-all  cand_parts fp32 [W * cap, C] -> [W, cap, C]; tcar_cand_combine, tcar_cand_rank, tcar_rerank_take   (rerank only)

        `pieces` supplies the local compute:
             begin() -> rows [cap, ld]          prepare(rows_all [W*cap, ld])          fold() -> state [W*cap, 2C+4]
             merge(states [W, cap, 2C+4]) -> shortlist ids [cap, C]                   shortlist() -> the result of a retrieval
             scores(lists [W*cap, C]) -> parts [W*cap, C]                             rerank(parts [W, cap, C]) -> the two-stage result"""
        self.order = []
        self.wait_rows()
        head = pieces.begin()
        head_all = self.all_gather(head, "serve_rows").view(self.world * cap, -1)
        pieces.prepare(head_all)
        state = pieces.fold()
        ids = pieces.merge(self.all_to_all_rows(state, cap, "retrieve_states"))
        if not rerank:
            return pieces.shortlist()
        lists = self.all_gather(ids, "retrieve_shortlists").view(self.world * cap, -1)
        part = pieces.scores(lists)
        return pieces.rerank(self.all_to_all_rows(part, cap, "cand_parts"))

    def candidates(self, pieces, cap: int):
        """one candidate-scoring step: every session names C items, every rank scores the slots whose rows it owns for the sessions of
        EVERY rank, and each session's list takes every slot from its owner.  The same collectives on every rank:

          1 all-gather  serve_rows (no exclusions, no window)
          2 all-gather  cand_lists int32 [cap, C]
          3 all-to-all  cand_parts fp32 [W * cap, C] -> [W, cap, C]; tcar_cand_combine, tcar_cand_rank (with `clicked`)

        `pieces`: begin(), prepare(rows_all), lists() -> [cap, C], scores(lists [W*cap, C]) -> parts, rank(parts [W, cap, C]) -> result"""
        self.order = []
        self.wait_rows()
        head = pieces.begin()
        pieces.prepare(self.all_gather(head, "serve_rows").view(self.world * cap, -1))
        lists = self.all_gather(pieces.lists(), "cand_lists").view(self.world * cap, -1)
        part = pieces.scores(lists)
        return pieces.rank(self.all_to_all_rows(part, cap, "cand_parts"))


class _Pieces:
    """The local compute between the exchanges of ShardExchange.step, bound to the C entry points of csrc/step.hip.  ONE object per
    engine, re-armed per step (a class statement and eight closures per step were host time the step cannot hide behind)."""

    def __init__(self, eng):
        self.eng = eng

    def arm(self, bt, cap, K, nr, ldr, refresh, lr_pending, ctx, sctx, sh):
        e = self.eng
        self.bt, self.cap, self.K, self.nr, self.ldr, self.refresh, self.lr_pending = bt, cap, K, nr, ldr, refresh, lr_pending
        self.ctx, self.sctx, self.sh, self.st = ctx, sctx, sh, e._stream()
        self.B = bt.B if bt is not None else 0
        self.Bq = e.world * cap
        self.has_neg = K > 0

    # zero the arena, session forward, ONE packed row per session: [attout (ek) | label | coefficient of the negative
    # term | K negatives | pad], ints as bits, row stride ld_head (tcar_shard_begin packs, tcar_shard_score unpacks)
    def begin(self):
        e, bt = self.eng, self.bt
        head = e.head_loc[:self.cap]
        check(e.lib.tcar_shard_begin(C.byref(self.ctx), C.byref(bt) if bt is not None else None, self.cap, e._kcap, e._p(head),
                                     e.ld_head, self.refresh, e.nl, self.lr_pending, self.st), "tcar_shard_begin")
        return head

    # scoring of the shard against every session + softmax statistics of the shard
    def score(self, head_all):
        e, sh = self.eng, self.sh
        sh.att_all, sh.ld_att, sh.head_K = head_all.data_ptr(), e.ld_head, (self.K if self.has_neg else 0)
        self._head_all = head_all
        tk = e._tick3(0)
        check(e.lib.tcar_shard_score(C.byref(self.sctx), C.byref(sh), self.refresh, self.st), "tcar_shard_score")
        e._tock3(tk)
        if self.refresh:        # (the one-hot schedule issues no refresh: the planes stay dirty for the next op-level reader)
            e._time_dirty = False
        return e.s_stats[:self.Bq]

    # lse, dlogits planes, dE of the shard (aux stream, stays here), dX partial (goes home)
    def backward(self, stats_all):
        e = self.eng
        self._stats_all = stats_all
        tk = e._tick3(1)
        check(e.lib.tcar_shard_backward(C.byref(self.sctx), C.byref(self.sh), e._p(stats_all), self.st), "tcar_shard_backward")
        e._tock3(tk)
        return e.s_dx[:self.Bq]

    # negative rows, shard norm, candidate-time backward: on the aux stream behind dE, beside the dX exchange and the
    # session backward (tcar_shard_join orders the main stream behind them)
    def finish(self):
        e = self.eng
        check(e.lib.tcar_shard_finish(C.byref(self.sctx), C.byref(self.sh), self.K if self.has_neg else 0,
                                      e._p(e.s_neg) if self.has_neg else None, e._p(e.s_coef) if self.has_neg else None, self.st),
              "tcar_shard_finish")

    # session backward (local) -> packed rows [row (ldh) | id | pad]
    def session_backward(self, dx_rows):
        e, bt = self.eng, self.bt
        rows = e._rows_buf[:self.nr]
        if bt is not None:
            if not dx_rows.is_contiguous():
                dx_rows = dx_rows.contiguous()
            ce_rows = e.s_ce[e.dp_rank * self.cap:e.dp_rank * self.cap + self.B]
            check(e.lib.tcar_step_session_backward(C.byref(self.ctx), C.byref(bt), e._p(dx_rows), e._p(rows), self.ldr, self.nr,
                                                   e._p(ce_rows), self.st), "tcar_step_session_backward")
        else:
            rows.zero_()                    # an empty rank contributes padding rows only (id 0, zero payload)
        return rows

    # ids are 1-based: the rows of this shard become 1 .. nl, the rest (and the id-0 padding) fall out
    def scatter(self, all_rows):
        e = self.eng
        check(e.lib.tcar_shard_join(C.byref(self.ctx), self.st), "tcar_shard_join")
        check(e.lib.tcar_scatter_add_rows_packed(C.byref(e.dims_cand), e._p(all_rows), self.ldr, all_rows.shape[0], e.n0, e._p(e.Gi),
                                                 self.st), "tcar_scatter_add_rows_packed")

    # arena gradients + norm pieces incl. the shards' dense item norms
    def arena(self):
        return self.eng.Gx

    # dense-weight norms, summed in a fixed order (one workgroup per variable): identical gradients give identical
    # norms on every rank, the replicas stay bit-identical without a broadcast
    def norms(self):
        check(self.eng.lib.tcar_step_dense_norms(C.byref(self.ctx), self.st), "tcar_step_dense_norms")

    def update(self):
        self.eng.poll_fork_errors()              # a fork of this step that has already timed out: raise BEFORE the variables move
        return self.eng._update_local()


class _ServePieces:
    """The local compute between the exchanges of ShardExchange.serve, bound to the C entry points of include/tcar_serve_shard.h.  ONE
    object per engine, re-armed per call.  Each piece can be called on its own (tests play the collectives by hand)."""

    def __init__(self, eng):
        self.eng = eng

    def arm(self, bt, cap, k, panel, labelled, meta, X, windowed, quota):
        e = self.eng
        self.bt, self.cap, self.k, self.panel, self.labelled = bt, cap, k, panel, labelled
        self.meta, self.X, self.K, self.windowed, self.quota = meta, X, 2 + X, windowed, quota
        self.B = bt.B if bt is not None else 0
        self.Bq = e.world * cap
        self.rw = 2 * k + 4                       # words of a state row (tcar_select_state_bytes)
        self.ld = _ru(e.geo.ek + 2 + self.K, 4)
        self.st = e._stream()
        self.refresh = int(e._time_dirty)
        sh = _lib.Shard()
        sh.world, sh.cap, sh.n0, sh.n_loc = e.world, cap, e.n0, e.nl
        sh.a16h, sh.a16l = e.sv_a16h.data_ptr(), e.sv_a16l.data_ptr()
        self.sh, self.sctx = sh, e._serve_ctx()

    # session forward of the local sessions, ONE packed row per session: [attout (ek) | label | unused | lo | hi | X exclusion ids |
    # pad] in the slots of the training step's rows (tcar_shard_pack_head: label, coefficient, "negatives"); rows past the local
    # batch are padding sessions: label -1, an empty window, no exclusions
    def begin(self):
        e, bt, B = self.eng, self.bt, self.B
        head = e.sv_head[:self.cap]
        if bt is not None:
            check(e.lib.tcar_step_session_forward(C.byref(e._ctx()), C.byref(bt), self.st), "tcar_step_session_forward")
        check(e.lib.tcar_shard_pack_head(B, self.cap, e.geo.ek, self.K, self.K, e._p(e.attout) if B else None,
                                         C.c_void_p(bt.label) if B else None, None, e._p(self.meta) if B else None, e._p(head),
                                         self.ld, self.st), "tcar_shard_pack_head")
        return head

    # the gathered rows: their ints back into arrays, the attout planes, the label scores this shard owns (0 elsewhere)
    def prepare(self, head_all):
        e, Bq = self.eng, self.Bq
        self._head_all = head_all
        self.sh.att_all, self.sh.ld_att = head_all.data_ptr(), self.ld
        check(e.lib.tcar_shard_unpack_head(Bq, e.geo.ek, self.K, e._p(head_all), self.ld, e._p(e.sv_lab), e._p(e.sv_coef),
                                           e._p(e.sv_meta), self.st), "tcar_shard_unpack_head")
        if self.windowed:
            e.sv_lohi[:, :Bq].copy_(e.sv_meta[:Bq, :2].t())
        if self.X:
            e.sv_excl[:Bq].copy_(e.sv_meta[:Bq, 2:])
        lab = self.labelled
        check(e.lib.tcar_shard_serve_begin(C.byref(self.sctx), C.byref(self.sh), self.refresh, e._p(e.sv_lab) if lab else None,
                                           e._p(e.sv_lab_part) if lab else None, self.st), "tcar_shard_serve_begin")
        if self.refresh:
            e._time_dirty = False
        return e.sv_lab_part[:Bq] if lab else None

    # every session takes the label score of its label's owner (label // shard rows), on the device
    def label_scores(self, parts_all):
        e, Bq = self.eng, self.Bq
        if parts_all.shape[0] == 1:
            e.sv_lab_score[:Bq].copy_(parts_all[0])
            return
        owner = torch.div(e.sv_lab[:Bq].clamp(min=0), e.S, rounding_mode="floor").clamp(max=parts_all.shape[0] - 1).long()
        e.sv_lab_score[:Bq].copy_(parts_all.gather(0, owner[None, :])[0])

    # the shard's rows, panel by panel, into one state per session of every rank
    def fold(self):
        e, Bq, lab = self.eng, self.Bq, self.labelled
        s = e._serve_desc(self.k, self.panel, e.sv_panel, e.sv_state, e.sv_excl if self.X else None, self.X)
        w = e._window_desc(e._item_keys, e.sv_lohi) if self.windowed else None
        q = self.quota
        check(e.lib.tcar_shard_serve_fold(C.byref(self.sctx), C.byref(self.sh), e._p(e.sv_lab) if lab else None,
                                          e._p(e.sv_lab_score) if lab else None, C.byref(s), C.byref(w) if w is not None else None,
                                          C.byref(q) if q is not None else None, self.st), "tcar_shard_serve_fold")
        return e.sv_state[:Bq]

    # the W states of the local sessions' rows -> one (tcar_select_merge), finished
    def finish(self, states):
        e, cap, k, B, lab = self.eng, self.cap, self.k, self.B, self.labelled
        W = states.shape[0]
        if not states.is_contiguous():
            states = states.contiguous()
        self._states = states
        r0 = e.dp_rank * cap
        q = self.quota
        check(e.lib.tcar_select_merge(cap, k, W, e._p(states, r0 * self.rw), self.Bq * self.rw, e._p(e.sv_merged),
                                      C.c_void_p(q.cat) if q is not None else None, q.cap if q is not None else 0, self.st),
              "tcar_select_merge")
        ls = e._p(e.sv_lab_score, r0) if lab else None
        check(e.lib.tcar_select_finish(cap, k, e._p(e.sv_merged), ls, e._p(e.sel_topk), e._p(e.sel_score), e._p(e.sel_rank) if lab else None,
                                       e._p(e.sel_ce) if lab else None, self.st), "tcar_select_finish")
        return e.sel_rank[:B], e.sel_topk[:B], e.sel_ce[:B], e.sel_score[:B]


class _OwnedScores(_ServePieces):
    """What the pieces of ShardExchange.retrieve and .candidates share on top of begin / prepare of `_ServePieces` (unlabelled: the
    label slot of a packed row is the live marker): the shard's exact scores of the slots it owns, and the combine of the parts."""

    # lists [W*cap, C] GLOBAL ids of the sessions of every rank -> parts [W*cap, C]: the owner's exact score, -inf elsewhere
    def scores(self, lists):
        e, C_ = self.eng, self.C
        if not lists.is_contiguous():
            lists = lists.contiguous()
        self._lists = lists
        check(e.lib.tcar_shard_cand_scores(C.byref(self.sctx), C.byref(self.sh), C_, e._p(lists), C_, e._p(e.rs_part), C_, self.st),
              "tcar_shard_cand_scores")
        return e.rs_part[:self.Bq]

    # parts [W, cap, C] of the local sessions' lists `cand` [cap, C] -> out [cap, C]: every slot takes its owner's bits
    def _combine(self, parts, cand, out):
        e, cap, C_ = self.eng, self.cap, self.C
        if not parts.is_contiguous():
            parts = parts.contiguous()
        self._parts = parts
        check(e.lib.tcar_cand_combine(cap, C_, parts.shape[0], e.S, e.geo.N, e._p(cand), C_, e._p(parts), cap * C_, e._p(out), C_,
                                      self.st), "tcar_cand_combine")


class _RetrievePieces(_OwnedScores):
    """The local compute between the exchanges of ShardExchange.retrieve, bound to the C entry points of
    include/tcar_retrieve_shard.h.  ONE object per engine, re-armed per call; each piece can be called on its own."""

    def arm(self, bt, cap, C_, k, panel, meta, X, windowed):
        super().arm(bt, cap, k or 1, panel, False, meta, X, windowed, None)
        self.C, self.k, self.rw = C_, k, 2 * C_ + 4

    # the shard's rows, panel by panel in the coarse precision, into one top-C state per session of every rank; padding sessions
    # (label slot -1) cost nothing
    def fold(self):
        e, Bq = self.eng, self.Bq
        d = _lib.Retrieve()
        d.C, d.panel, d.panel_buf = self.C, self.panel, e.sv_panel.data_ptr()
        d.state, d.state_bytes = e.rs_state.data_ptr(), e.rs_state.numel() * 4
        if self.X:
            d.excl, d.X = e.sv_excl.data_ptr(), self.X
        w = e._window_desc(e._item_keys, e.sv_lohi) if self.windowed else None
        if w is not None:
            d.window = C.addressof(w)                # (w stays alive until the call has returned)
        check(e.lib.tcar_shard_retrieve_fold(C.byref(self.sctx), C.byref(self.sh), C.byref(d), e._p(e.sv_lab), self.st),
              "tcar_shard_retrieve_fold")
        return e.rs_state[:Bq]

    # the W states of the local sessions' rows -> one (tcar_retrieve_merge), finished: the shortlist [cap, C]
    def merge(self, states):
        e, cap, C_ = self.eng, self.cap, self.C
        if not states.is_contiguous():
            states = states.contiguous()
        self._states = states
        check(e.lib.tcar_retrieve_merge(cap, C_, states.shape[0], e._p(states), cap * self.rw, e._p(e.rs_merged), self.st),
              "tcar_retrieve_merge")
        check(e.lib.tcar_retrieve_finish(cap, C_, e._p(e.rs_merged), e._p(e.rs_ids), e._p(e.rs_scores), self.st), "tcar_retrieve_finish")
        return e.rs_ids[:cap]

    def shortlist(self):
        e = self.eng
        return e.rs_ids[:self.B], e.rs_scores[:self.B]

    # the exact scores of the shortlist from their owners, its list order, the first k of it
    def rerank(self, parts):
        e, cap, C_, k = self.eng, self.cap, self.C, self.k
        self._combine(parts, e.rs_ids, e.rs_exact)
        check(e.lib.tcar_cand_rank(cap, C_, e._p(e.rs_exact), C_, e._p(e.rs_ids), C_, None, 0, e._p(e.rs_rank[0]), e._p(e.rs_rank[1]),
                                   None, None, self.st), "tcar_cand_rank")
        check(e.lib.tcar_rerank_take(cap, C_, k, e._p(e.rs_ids), e._p(e.rs_exact), e._p(e.rs_rank[1]), e._p(e.rs_topk),
                                     e._p(e.rs_topscore), self.st), "tcar_rerank_take")
        return e.rs_topk[:self.B], e.rs_topscore[:self.B]


class _CandPieces(_OwnedScores):
    """The local compute between the exchanges of ShardExchange.candidates.  ONE object per engine, re-armed per call."""

    def arm(self, bt, cap, C_, meta, clicked):
        super().arm(bt, cap, 1, 128, False, meta, 0, False, None)
        self.C, self.clicked = C_, clicked

    # the local sessions' lists [cap, C]: -1 (empty slots) in the rows past the local batch
    def lists(self):
        return self.eng.cs_in[0, :self.cap]

    def rank(self, parts):
        e, cap, C_, B, clk = self.eng, self.cap, self.C, self.B, self.clicked
        cand = e.cs_in[0]
        self._combine(parts, cand, e.cs_score)
        check(e.lib.tcar_cand_rank(cap, C_, e._p(e.cs_score), C_, e._p(cand), C_, e._p(e.cs_in[1]) if clk else None, C_ if clk else 0,
                                   e._p(e.cs_rank[0]), e._p(e.cs_rank[1]), e._p(e.cs_counts) if clk else None,
                                   e._p(e.cs_metrics) if clk else None, self.st), "tcar_cand_rank")
        return CandResult(e.cs_score[:B], e.cs_rank[0, :B], e.cs_rank[1, :B], e.cs_counts[:B] if clk else None,
                          e.cs_metrics[:B] if clk else None)


class ShardedEngine(TcarEngine):
    def __init__(self, params, content_emb, mwdhm, lr=1e-3, max_grad=150.0, neg_weight=0.01, device="cuda:0", group=None,
                 scoring="bf16x3", world: Optional[int] = None, rank: Optional[int] = None,
                 force_collectives: Optional[bool] = None, direct_rccl: Optional[bool] = None, **kw):
        if scoring == "f32":
            raise ValueError("the catalog-sharded step runs the split-bf16 scoring modes (use mode='replica' for f32)")
        self.group = group
        # the collective schedule; its layer (dp.Collectives) decides world, rank (TCAR_SIM_WORLD included) and how collectives run
        self.xch = ShardExchange(group, world, rank, sim=None, force=force_collectives, direct=direct_rccl)
        self.world, self.dp_rank = self.xch.world, self.xch.rank
        self._mwdhm_full = np.asarray(mwdhm)
        N = content_emb.shape[0] - 1
        self.S = shard_rows(N, self.world)
        n0 = min(N, self.dp_rank * self.S)
        nl = max(0, min(N, n0 + self.S) - n0)
        if nl <= 0:
            self.xch.close()
            raise ValueError("more ranks than 128-row catalog blocks")
        # dX of a shard contracts over N / W catalog rows for W * B sessions: W times more output tiles and a W times shorter
        # K than the single-rank GEMM, so the split that fills the chip (and the slab bytes it writes) shrinks with W
        sw = Switches.read()
        if "splitk" not in kw and not sw.splitk:
            kw["splitk"] = max(2, -(-36 // self.world))
        if self.xch.collective:
            self.priority_stream = False          # (TcarEngine.priority_stream: no priority stream beside live collectives)
        super().__init__(params, content_emb, mwdhm, lr=lr, max_grad=max_grad, neg_weight=neg_weight, device=device,
                         scoring=scoring, shard=(n0, nl), switches=sw, **kw)
        self.n0, self.nl = n0, nl
        self.n_local_items = nl
        self.backend = self.xch.backend
        if self.xch.collective and self.tune is None and not sw.shard_all_flags:
            # Flag forks whose PRODUCER sits behind a collective: the gather behind the item-row all-gather of the
            # previous update (FK_GATHER), the slab reduce and the input-gradient launch behind the dX reduce-scatter (FK_REDUCE,
            # FK_INGRAD).  A peer whose host stalls holds those producers back for as long as it likes, and a poll gives up after
            # 1 s — so these three fork through events whenever collectives are live; the others depend on local work only.
            mask = int(_lib.tuning().flag_fork) & ~((1 << 3) | (1 << 4) | (1 << 6))
            self.set_tuning(TCAR_FLAG_FORK=mask)
        self.cap, self._kcap, self._rows_cap = 0, 0, 0
        self.score_form = self._score_form()
        self.onehot = self.score_form.fused_ce
        self._stage = torch.zeros(self.world, self.S, self.geo.ldh, dtype=torch.float32, device=self.dev)
        self.bytes_moved = self.xch.bytes_moved

    # ------------------------------------------------------------------------------------------ collectives
    close = dp.DPEngine.close          # synchronise, then destroy the direct RCCL communicator (idempotent)
    RETRIEVE_COLLECTIVES = ("serve_rows", "retrieve_states", "retrieve_shortlists", "cand_parts")
    CAND_COLLECTIVES = ("serve_rows", "cand_lists", "cand_parts")

    def exchange_info(self) -> Dict[str, object]:
        g = self.geo
        return {"mode": "sharded", "world": self.world, "shard_rows": self.S,
                "collectives": ("none" if not self.xch.collective else
                                "RCCL C API on the step's stream (rccl.py)" if self.xch.direct is not None else
                                "torch.distributed process group (%s)" % self.xch.backend),
                "bytes_per_step": dict(self.bytes_moved),
                "ms_per_collective": self.xch.collective_ms(),      # filled by the event-instrumented pass (enable_native_timing)
                "item_rows_allgather_bytes": 4 * self.world * self.S * g.ldh,
                "replica_mode_allreduce_bytes": 4 * (g.N * (g.ldh + g.pt) + self.arena_n + _lib.NSLOT),
                "collectives_per_step": 6,
                "serve_collectives": ("serve_rows", "serve_label_scores", "serve_states"),        # ShardExchange.serve (labelled: all three)
                "serve_bytes": {n: self.bytes_moved.get(n, 0) for n in ("serve_rows", "serve_label_scores", "serve_states")},
                # ShardExchange.retrieve (a retrieval alone: the first two) and .candidates; bytes per rank SENT of an all-to-all
                "retrieve_collectives": self.RETRIEVE_COLLECTIVES, "cand_collectives": self.CAND_COLLECTIVES,
                "retrieve_bytes": {n: self.bytes_moved.get(n, 0) for n in self.RETRIEVE_COLLECTIVES},
                "cand_bytes": {n: self.bytes_moved.get(n, 0) for n in self.CAND_COLLECTIVES},
                # how all_to_all_rows ran: "all-to-all (RCCL C API)", "all-to-all (<backend>)", or, on a backend without one (the
                # documented fallback, not a failure), "all-gather + slice (<backend>)"; "none" until the first exchange
                "all_to_all": self.xch.all_to_all_path,
                "note": "all-gather [attout | label | negatives | coefficient] rows, all-gather softmax stats, reduce-scatter dX, "
                        "all-gather [row | id] item-row gradients, all-reduce arena, all-gather updated item rows; the dense item "
                        "gradient and the candidate-time block stay local"}

    # -------------------------------------------------------------------------------------------- workspace
    s_logits = None          # (the one-hot schedule keeps no fp32 logits of the shard)

    def _score_form(self) -> ScoreForm:
        """switches + geometry + scoring mode -> the form of the shard pieces (nothing else derives it): the benchmarked single-GPU
        schedule on the shard (tcar_hip.h: tcar_shard_score) — softmax epilogue + both one-hot forms, no fp32 logits — or all of it
        materialised; the anchored softmax form on top of the former"""
        sw = self.sw
        oh = (self.scoring_code == 3 and self.scoring_bwd == 1 and self.geo.ldt == 64
              and not (sw.shard_materialised or sw.no_onehot or sw.no_onehot_bwd))
        return ScoreForm(planes=True, logits=not oh, fused_ce=oh, onehot_fwd=oh, onehot_bwd=oh, anchored=oh and not sw.no_ce_anchor)

    def _score_specs(self) -> List[Spec]:
        """the scoring family of the shard: the world * cap session rows of the exchange against the n_loc candidate rows, under
        `s_` names (the row scales of the anchored form: tcar_shard_t.scale2)"""
        return scoring_specs(self.geo, self.world * self.cap, self.nl, self.splitk, self.score_form,
                             lambda f: "s_scale2" if f == "ce_rowscale" else "s_" + f, self._fill_onehot)

    def _ensure_score(self, cap: int, K: int):
        if cap > self.cap or K > self._kcap:
            g = self.geo
            self.cap, self._kcap = max(cap, self.cap), max(K, self._kcap, 1)
            cap, kc, Bq = self.cap, self._kcap, self.world * self.cap
            self.ld_head = _ru(g.ek + 2 + kc, 4)
            self.ws.ensure([Spec("head_loc", (cap, self.ld_head), F32, 0),        # [attout | label | neg coefficient | negatives | pad]
                            Spec("s_lab", (Bq,), I32, -1), Spec("s_neg", (Bq, kc), I32, -1), Spec("s_coef", (Bq,), F32, 0),   # unpacked by tcar_shard_score
                            Spec("s_stats", (Bq, 3), F32), Spec("s_lse", (Bq,), F32), Spec("s_ce", (Bq,), F32), Spec("s_dx", (Bq, g.ek), F32)]
                           + self._score_specs())

    # two composite spans instead of the three GEMMs of the fused step: the C++ pieces between the exchanges
    TIMED_KERNELS = ("shard_score", "shard_backward")

    # ------------------------------------------------------------- timing of the scoring pieces (bench.py)
    def enable_native_timing(self, n: int):
        self._tm = {"n": n, "ev": [[], [], []]}
        self.xch.timing = True

    def _tick3(self, kind):
        tm = getattr(self, "_tm", None)
        if tm is None or len(tm["ev"][kind]) >= tm["n"]:
            return None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(torch.cuda.current_stream(self.dev))
        tm["ev"][kind].append((e0, e1))
        return e1

    def _tock3(self, e1):
        if e1 is not None:
            e1.record(torch.cuda.current_stream(self.dev))

    def native_timing_ms(self, kind: int = 0):
        tm = getattr(self, "_tm", None)
        return [a.elapsed_time(b) for a, b in tm["ev"][kind]] if tm else []

    # ----------------------------------------------------------------------------------------------- step
    def _step(self, bt: Optional[Batch], cap: int, K: int, update: bool, T: int, lr_pending: float = -1.0):
        """one training step; bt = None: a rank whose shard of the global batch is empty still joins every collective (T is
        the step's input length: the row buffers of the exchanges have the same shape on every rank).  The collectives are
        ShardExchange.step; the pieces between them are the C entry points of csrc/step.hip (`_Pieces`).  lr_pending >= 0 (one
        rank): the previous step's update is owed and rides in tcar_shard_begin as the split update of the single-GPU step.
        A rank that exchanges nothing (one rank, no live collectives) makes ONE call: tcar_shard_step_local sequences the same
        pieces in C++ (round 6: the Python sequencing was ~0.2 ms of host time per step).  With live collectives the step stays
        sequenced here; one C call that is handed the communicator is left for later."""
        g = self.geo
        B = bt.B if bt is not None else 0
        cap = max(cap, B, 1)
        if self._index_stale:                      # (shard_update_items changed a publish time of an owned row)
            self._build_time_index()
        self.xch.wait_rows()                       # the previous update's rows, before anything reads the item table
        self._ensure_work(max(B, 1), T)
        self._ensure_score(cap, K)
        nr = cap * T
        ldr = g.ldh + 4
        if self._rows_cap < nr:
            self.ws.get(Spec("_rows_buf", (nr, ldr), F32, 0))
            self._rows_cap = nr
        # (the one-hot schedule reads the shard's time planes nowhere; eval_step rebuilds the fp32 time columns itself)
        refresh = 0 if self.onehot else int(self._time_dirty)
        ctx, sctx = self._ctx(), self._shard_ctx()
        sh = self._shard_desc(cap)
        if (bt is not None and not self.xch.collective and self.world == 1 and getattr(self, "_tm", None) is None
                and not self.sw.shard_py_step):
            sh.att_all, sh.ld_att, sh.head_K = self.head_loc.data_ptr(), self.ld_head, K
            lr_u = -1.0
            if update:
                self.poll_fork_errors()
                lr_u = self._lr_t()
            check(self.lib.tcar_shard_step_local(C.byref(ctx), C.byref(sctx), C.byref(sh), C.byref(bt), self._kcap,
                                                 C.c_void_p(self.head_loc.data_ptr()), self.ld_head, refresh, lr_pending,
                                                 C.c_void_p(self._rows_buf.data_ptr()), ldr, nr, C.byref(self.dims_cand), lr_u,
                                                 self._stream()), "tcar_shard_step_local")
            if refresh:
                self._time_dirty = False
            if update:
                self._after_update()
            return
        pc = getattr(self, "_pieces", None)
        if pc is None:
            pc = self._pieces = _Pieces(self)
        pc.arm(bt, cap, K, nr, ldr, refresh, lr_pending, ctx, sctx, sh)
        self.xch.step(pc, cap, update)

    # tcar_shard_t pointer fields <- attribute, beside those of the scoring family
    SHARD_OWN = (("stats", "s_stats"), ("lse", "s_lse"), ("ce", "s_ce"), ("dx", "s_dx"), ("lab_all", "s_lab"), ("neg_all", "s_neg"),
                 ("coef_all", "s_coef"))
    SHARD_FAMILY = ("logits", "a16h", "a16l", "ap16h", "ap16l", "dl16h", "dl16l", "slabs", "aps16h")
    # fields of the shard's tcar_ctx_t that take the shard's own buffers of the one-hot schedule
    SCTX_FAMILY = ("ce_ws", "ce_geo", "oh16", "p16h", "p16l", "tclip", "dP", "qz")

    def _shard_desc(self, cap: int) -> "_lib.Shard":
        key = (cap, self.ws.version)
        if getattr(self, "_sh_key", None) != key:
            sh = _lib.Shard()
            sh.world, sh.cap, sh.n0, sh.n_loc = self.world, cap, self.n0, self.nl
            for f, a in self.SHARD_OWN:
                setattr(sh, f, getattr(self, a).data_ptr())
            self.ws.bind(sh, self._score_specs(), only=self.SHARD_FAMILY)
            if self.score_form.anchored:
                sh.scale2, sh.n_total = self.s_scale2.data_ptr(), self.geo.N
            self._sh, self._sh_key = sh, key
        return self._sh

    def shard_form(self, cap: int) -> Dict[str, bool]:
        """the form the C++ shard pieces take at a capacity of `cap` sessions per rank (tcar_shard_form: their own predicates)"""
        self._ensure_score(cap, self._kcap)
        out = (C.c_int32 * 2)()
        check(self.lib.tcar_shard_form(C.byref(self._shard_ctx()), C.byref(self._shard_desc(cap)), out), "tcar_shard_form")
        return {"onehot": bool(out[0]), "ce_anchored": bool(out[1])}

    def _shard_ctx(self):
        """tcar_ctx_t whose candidate side is this rank's shard (tcar_step_update: arena + the owned item rows + planes); follows the
        rank's context, which is rebuilt whenever a buffer of the engine was (re-)allocated"""
        c = self._ctx()
        if getattr(self, "_sctx_src", None) is not c:
            s = _lib.Ctx()
            C.memmove(C.byref(s), C.byref(c), C.sizeof(_lib.Ctx))
            s.d = self.dims_cand
            s.E = self.E.data_ptr() + 4 * self.n0 * self.geo.ek
            if self.onehot:
                self.ws.bind(s, self._score_specs(), {"ce_ws": "ce_ws_floats"}, only=self.SCTX_FAMILY)
            else:
                s.oh16 = s.tclip = s.dP = s.qz = None
            self._sctx, self._sctx_src = s, c
        return self._sctx

    _update_ctx = _shard_ctx

    def _serve_ctx(self):
        """the shard's context of the serving pieces (tcar_shard_serve_begin / _fold): candidate side = this rank's shard, none of the
        training step's scoring workspaces (an engine that only serves never allocates them)"""
        c = self._ctx()
        if getattr(self, "_svctx_src", None) is not c:
            s = _lib.Ctx()
            C.memmove(C.byref(s), C.byref(c), C.sizeof(_lib.Ctx))
            s.d = self.dims_cand
            s.E = self.E.data_ptr() + 4 * self.n0 * self.geo.ek
            self._svctx, self._svctx_src = s, c
        return self._svctx

    def _update_local(self):
        """clip + Adam: arena on every rank, the item rows of the shard by their owner; returns the staging buffer of collective 6
        (this rank's updated rows in its slot) and the installer that copies the gathered table into E"""
        g = self.geo
        check(self.lib.tcar_step_update(C.byref(self._update_ctx()), self._lr_t(), self._stream()), "tcar_step_update")
        self._after_update()
        if not self.xch.collective:
            return None
        self._stage[self.dp_rank, :self.nl].copy_(self.E[self.n0:self.n0 + self.nl, :g.ldh])

        def install(stage):
            self.E[:g.N, :g.ldh].copy_(stage.view(-1, g.ldh)[:g.N])
        return self._stage, install

    def flush(self):
        """a deferred update (one rank, train_step(defer_update=True)) applied now + the pending item-row all-gather of the last
        update (every reader of the item table calls flush)"""
        super().flush()
        self.xch.wait_rows()

    @property
    def can_defer(self) -> bool:
        """the split (deferred) update of the single-GPU step applies when this rank owns the whole table and nothing is exchanged
        behind the update: ONE rank.  With more ranks the owned rows must reach the other ranks before their next gather, so the
        update (1 / world of the table) stays inside its step."""
        return self.world == 1 and not self.xch.collective and self.overlap and hasattr(self, "adam_bitmap")

    # ------------------------------------------------------------------------------------------- public API
    score_batch = property(lambda self: self.world * max(self.cap, 1))

    def train_step(self, batch, bt: Optional[Batch] = None, cap_rows: Optional[int] = None, cap: Optional[int] = None,
                   T: Optional[int] = None, K: Optional[int] = None, defer_update: bool = False):
        """`batch` / `bt` = this rank's sessions (None: its shard of the global batch is empty — it still joins every
        collective and must be told the step's input length T and negative count K, which every rank knows from the bucket
        schedule).  cap = rows every rank contributes to the all-gathers (>= the largest local batch of the step; default: the
        local batch size — weak-scaling runs with equal batches); cap_rows (dp.DPEngine's argument: cap * T) is accepted
        for drop-in use.  No metadata collective, no host synchronisation."""
        # defer_update (TcarEngine's split update): on ONE rank the update of this step is applied at the start of the next one
        # (tcar_shard_begin) or by flush(), as in the single-GPU step; with more ranks it is ignored — the sharded update is followed
        # by the all-gather of the updated rows, which the next step's gathers need: there is nothing to defer it behind
        self._refuse_ragged(batch, bt, "train_step")
        if bt is None and batch is not None:
            bt = self.upload(batch)
        if bt is not None:
            T = bt.T
            K = bt.K if bt.neg else 0
        elif T is None or K is None:
            raise ValueError("an empty rank needs the step's T and K")
        if cap is None:
            cap = (cap_rows // max(T, 1)) if cap_rows else (bt.B if bt is not None else 1)
        if bt is not None and self.can_defer and (defer_update or self._pending_lr is not None):
            self._step_deferred(lambda lr: self._step(bt, cap, K, False, T, lr_pending=-1.0 if lr is None else lr), defer_update)
            return self._loss_rows(bt, cap, K)
        self.flush()
        self._step(bt, cap, K, True, T)
        self.poll_fork_errors()                   # (a flag fork of this step's pieces that timed out: never silent)
        if bt is None:
            return torch.zeros(0, device=self.dev)
        return self._loss_rows(bt, cap, K)

    def _loss_rows(self, bt, cap, K):
        if K:
            return self.loss[:bt.B]
        # label_neg fed as [B, 0]: the negative term is the constant neg_weight * ln 2 (model_combine.py:142-147)
        return self.s_ce[self.dp_rank * cap:self.dp_rank * cap + bt.B] + float(np.float32(self.neg_weight) * np.float32(np.log(2.0)))

    def loss_and_grads(self, batch, bt: Optional[Batch] = None, cap_rows: Optional[int] = None, cap: Optional[int] = None):
        self._refuse_ragged(batch, bt, "loss_and_grads")
        bt = bt or self.upload(batch)
        if cap is None:
            cap = (cap_rows // max(bt.T, 1)) if cap_rows else bt.B
        K = bt.K if bt.neg else 0
        self.flush()
        self._step(bt, cap, K, False, bt.T)
        return self._loss_rows(bt, cap, K)

    def update(self):
        out = self._update_local()
        if out is not None:
            self.xch.share_rows(*out)

    def eval_step(self, batch, k: int = 20, bt: Optional[Batch] = None, keep_logits: bool = False):
        """local sessions against the WHOLE catalog on the fp32 GEMM (evaluation runs once per epoch)"""
        self._refuse_ragged(batch, bt, "eval_step")
        self.flush()
        bt = bt or self.upload(batch)
        g, lib, st, p = self.geo, self.lib, self._stream(), self._p
        B = bt.B
        self._ensure_work(B, bt.T)
        self.ws.ensure([Spec("ev_logits", (self.work_B, g.Npad), F32), Spec("topk", (self.work_B, k), I32)])
        full = Dims(g.N, g.H, g.Ht, g.ldh, g.ldt)
        if getattr(self, "_ev_mw", None) is None:
            self._ev_mw = torch.tensor(np.ascontiguousarray(self._mwdhm_full, dtype=np.int32), device=self.dev)
        check(lib.tcar_cand_time_fwd(C.byref(full), C.byref(self._time_ptrs()), p(self._ev_mw), p(self.E), st), "tcar_cand_time_fwd")
        check(lib.tcar_step_session_forward(C.byref(self._ctx()), C.byref(bt), st), "tcar_step_session_forward")
        check(lib.tcar_gemm_f32(1, B, g.N, g.ek, p(self.attout), g.ek, p(self.E), g.ek, p(self.ev_logits), g.Npad, None, 0, 0, 1,
                                st), "tcar_gemm_f32")
        check(lib.tcar_eval_rows(B, g.N, p(self.ev_logits), g.Npad, C.c_void_p(bt.label), k, p(self.rank), p(self.topk),
                                 p(self.ce), st), "tcar_eval_rows")
        out = (self.rank[:B], self.topk[:B], self.ce[:B])
        return out + (self.ev_logits[:B, :g.N].clone(),) if keep_logits else out

    # ---- streamed score-and-select over the shards (include/tcar_serve_shard.h; the collectives: ShardExchange.serve)
    def default_panel(self) -> int:
        """columns per panel when the caller names none: the widest a fold takes, at most the shard's rows"""
        return int(max(128, min(self.SERVE_MAX_PANEL, _ru(self.nl, 128))))

    def serve_pieces(self, batch, k: int = 20, labelled: bool = True, exclude_seen: bool = False, exclude=None,
                     panel: Optional[int] = None, window=None, max_per_category: Optional[int] = None, cap: Optional[int] = None,
                     T: Optional[int] = None, bt: Optional[Batch] = None) -> _ServePieces:
        """The armed local pieces of ONE ShardExchange.serve for this rank's sessions (`batch` / `bt`; both None: none — then T and
        cap are needed): eval_step_streamed (labelled) and recommend hand them to the exchange; a caller that moves the buffers
        itself calls begin / prepare / label_scores / fold / finish in that order.  No buffer of the catalog's width is touched:
        every rank scores its shard's rows only."""
        self._refuse_ragged_shard(batch, bt)
        k, panel, quota = self._serve_request(k, panel, window, max_per_category, _ru(self.nl, 128))
        bt, cap, X, meta = self._gathered_inputs(batch, bt, labelled, exclude_seen, exclude, window, cap, T, panel)
        self.ws.ensure([Spec("sv_state", (self.world * cap, 2 * k + 4), I32), Spec("sv_merged", (cap, 2 * k + 4), I32),
                        Spec("sel_score", (cap, k), F32), Spec("sel_topk", (cap, k), I32), Spec("sel_rank", (cap,), I32),
                        Spec("sel_ce", (cap,), F32)])
        pc = getattr(self, "_serve_pc", None)
        if pc is None:
            pc = self._serve_pc = _ServePieces(self)
        pc.arm(bt, cap, k, panel, labelled, meta, X, window is not None, quota)
        return pc

    def _refuse_ragged_shard(self, batch, bt=None) -> None:
        if self.is_ragged(batch) or getattr(bt, "_rg", None) is not None:      # (the sharded session forward is rectangular)
            raise ValueError("the catalog-sharded engine takes rectangular feeds: ragged batches (sessions of mixed lengths) are for "
                             "the single-engine serving calls")

    def _gathered_inputs(self, batch, bt, labelled: bool, exclude_seen: bool, exclude, window, cap, T, panel: int):
        """What every serving collective of this engine prepares behind its request checks: the uploaded local sessions (`batch` /
        `bt`; both None: none — then T and cap are needed), the rows every rank contributes, the width X of the exclusion lists every
        rank packs, the workspace of begin / prepare (`_ServePieces`) and the ints that ride behind attout, one row per local
        session -> (bt, cap, X, meta)."""
        g = self.geo
        self.flush()
        excl = None
        if labelled:
            if bt is None and batch is not None:
                bt = self.upload(batch)
        elif batch is not None:
            bt, excl = self._recommend_inputs(batch, exclude_seen, exclude)
        if bt is not None:
            T = bt.T
            bt = self._without_neg(bt)
            if not bt.label:                                # (the pack reads a label per live session; unlabelled: a placeholder)
                bt.label = self._label0(bt.B)
        elif T is None or cap is None:
            raise ValueError("a rank without sessions needs the step's T and cap")
        elif not labelled:                                  # the exclusion width every rank packs
            ex = np.asarray(exclude) if exclude is not None else np.zeros((0, 0))
            X = (T if exclude_seen else 0) + (int(ex.shape[1]) if ex.ndim == 2 else 0)
            excl = torch.zeros(0, X, dtype=torch.int32, device=self.dev) if X else None
        B = bt.B if bt is not None else 0
        cap = max(cap or 0, B, 1)
        self._ensure_work(max(B, 1), T)
        X = int(excl.shape[1]) if excl is not None else 0
        Bq, K = self.world * cap, 2 + X
        ld = _ru(g.ek + 2 + K, 4)
        rp = _ru(Bq, 128)
        self.ws.ensure([Spec("sv_head", (cap, ld), F32, 0), Spec("sv_lab", (Bq,), I32, -1), Spec("sv_coef", (Bq,), F32, 0),
                        Spec("sv_meta", (Bq, K), I32, -1), Spec("sv_lohi", (2, Bq), I32, 0), Spec("sv_excl", (Bq, max(X, 1)), I32, -1),
                        Spec("sv_a16h", (rp, g.ek), BF16, 0), Spec("sv_a16l", (rp, g.ek), BF16, 0),
                        Spec("sv_lab_part", (Bq,), F32, 0), Spec("sv_lab_score", (Bq,), F32, 0), Spec("sv_panel", (Bq, panel), F32)])
        meta = None
        if B:
            # the ints that ride behind attout: [lo | hi | exclusion ids], one row per local session
            if window is not None:
                lo, hi = self._window_bounds(window, B)
                lohi = torch.from_numpy(np.stack([lo, hi], axis=1)).to(self.dev)
            else:
                lohi = torch.zeros(B, 2, dtype=torch.int32, device=self.dev)
            meta = torch.cat([lohi, excl], dim=1).contiguous() if X else lohi
        return bt, cap, X, meta

    def _exchange(self, pc: _ServePieces):
        out = self.xch.serve(pc, pc.cap, pc.labelled)
        self.poll_fork_errors()
        return out

    def _label0(self, B: int) -> int:
        self.ws.ensure([Spec("sv_label0", (B,), I32, 0)])
        return self.sv_label0.data_ptr()

    def eval_step_streamed(self, batch, k: int = 20, bt: Optional[Batch] = None, panel: Optional[int] = None, window=None,
                           max_per_category: Optional[int] = None, cap: Optional[int] = None, T: Optional[int] = None):
        """TcarEngine.eval_step_streamed over the shards: (rank[B] int32, topk[B,k] int32, ce[B] f32) of THIS rank's sessions against
        the whole catalog, `last_scores` the scores of the lists.  A COLLECTIVE: every rank calls it — `batch` = None (and `bt` =
        None) on a rank without sessions, which must then be told the step's input length T and `cap`, the rows every rank
        contributes to the all-gathers (>= the largest local batch; default: the local batch size).  topk, scores and rank are the
        bits the unsharded streamed call gives for the same scores; ce differs by the rounding of the repartitioned sum."""
        pc = self.serve_pieces(batch, k, True, panel=panel, window=window, max_per_category=max_per_category, cap=cap, T=T, bt=bt)
        rank, topk, ce, self.last_scores = self._exchange(pc)
        return rank, topk, ce

    def recommend(self, batch, k: int = 20, exclude_seen: bool = True, exclude=None, panel: Optional[int] = None, window=None,
                  max_per_category: Optional[int] = None, cap: Optional[int] = None, T: Optional[int] = None):
        """TcarEngine.recommend over the shards: (topk [B,k] int32, scores [B,k] f32) of this rank's sessions.  A COLLECTIVE, as
        eval_step_streamed; every rank passes exclusion lists of the same width (exclude_seen adds T ids, `exclude` its columns)."""
        pc = self.serve_pieces(batch, k, False, exclude_seen, exclude, panel, window, max_per_category, cap, T)
        _, topk, _, self.last_scores = self._exchange(pc)
        return topk, self.last_scores

    def score_candidates(self, batch, candidates, clicked=None, bt: Optional[Batch] = None):
        """not on the catalog-sharded engine: a candidate's row lives on one rank only (include/tcar_cand.h takes the whole catalog)"""
        raise _lib.TcarError("candidate scoring needs the whole catalog on one engine (no shard): the catalog-sharded engine has none")

    def retrieve(self, batch, C, exclude_seen: bool = True, exclude=None, panel: Optional[int] = None, window=None):      # noqa: N803
        """not on the catalog-sharded engine: the shortlists of the shards would have to be merged (include/tcar_retrieve.h takes the
        whole catalog)"""
        raise _lib.TcarError("retrieve() needs the whole catalog on one engine (no shard): the catalog-sharded engine cannot merge "
                             "shortlists")

    @staticmethod
    def _refuse_diversity(diversity) -> None:
        if diversity is not None:
            raise _lib.TcarError("diversity (the MMR walk of recommend_two_stage) needs the whole catalog on one engine: the "
                                 "catalog-sharded two-stage call does not take the keyword yet")

    def diversify(self, candidates, scores, k: int = 20, diversity: float = 1.0):
        """not on the catalog-sharded engine (TcarEngine.diversify reads the content table of a whole-catalog engine)"""
        raise _lib.TcarError("diversify() needs the whole catalog on one engine (no shard)")

    def recommend_two_stage(self, batch, k: int = 20, shortlist: int = 256, exclude_seen: bool = True, exclude=None,
                            panel: Optional[int] = None, window=None, diversity=None):
        """not on the catalog-sharded engine: its first stage is retrieve(), its second score_candidates()"""
        self._refuse_diversity(diversity)
        raise _lib.TcarError("recommend_two_stage() needs the whole catalog on one engine (no shard): the catalog-sharded engine "
                             "has neither retrieve() nor score_candidates()")

    def recommend_sections(self, batch, sections, k: int = 10, exclude_seen: bool = True, exclude=None, panel: Optional[int] = None,
                           window=None, overall: Optional[int] = None):
        """not on the catalog-sharded engine: the B G state rows of the shards are what tcar_select_merge merges, but the exchange
        that would carry them is not built (include/tcar_sections.h takes the whole catalog)"""
        raise _lib.TcarError("recommend_sections() needs the whole catalog on one engine (no shard): sections over shards are not "
                             "built yet")

    def similar_items(self, ids=None, k: int = 20, content=None, exclude_self: bool = True, exclude=None, panel: Optional[int] = None,
                      window=None, max_per_category: Optional[int] = None):
        """not on the catalog-sharded engine (TcarEngine.similar_items is written for a whole-catalog engine and its workspace; the
        form over shards is not built)"""
        raise _lib.TcarError("similar_items() needs the whole catalog on one engine (no shard): related items over shards are not "
                             "built yet")

    def find_duplicates(self, threshold: float = 0.98, window=None, stripe: Optional[int] = None):
        """not on the catalog-sharded engine (TcarEngine.find_duplicates pairs every row with every other row of ONE table; the audit
        over shards as a collective is not built)"""
        raise _lib.TcarError("find_duplicates() needs the whole catalog on one engine (no shard): the audit over shards is not "
                             "built yet")

    def warm_start_items(self, ids, k: int = 16, min_sim: float = 0.0, exclude=None, window=None, panel: Optional[int] = None):
        """not on the catalog-sharded engine (TcarEngine.warm_start_items reads the donors' rows and the content of ONE table and
        writes through the whole-catalog update; the collective form over shards is not built)"""
        raise _lib.TcarError("warm_start_items() needs the whole catalog on one engine (no shard): the warm start over shards is "
                             "not built yet")

    def update_items(self, ids, content=None, item_rows=None, mwdhm=None, keys=None, categories=None):
        """not under this name on the catalog-sharded engine (include/tcar_catalog.h takes the whole catalog): a row's derived state
        lives on the rank that owns it and the ranks have to agree on the update — that is shard_update_items(), a collective"""
        raise _lib.TcarError("update_items() needs the whole catalog on one engine (no shard): the catalog-sharded engine does not "
                             "route rows to their owners")

    # ---- in-place catalog updates over the shards (include/tcar_catalog_shard.h).  A name of its own, as the calls below: it is a
    # COLLECTIVE, which the single-engine call (refused above) is not.
    _mwdhm_full_own = False       # (`_mwdhm_full` may be the caller's array: shard_update_items copies it before its first write)

    def shard_update_items(self, ids, content=None, item_rows=None, mwdhm=None, keys=None, categories=None, verify: bool = True) -> None:
        """TcarEngine.update_items over the shards: the arguments, the ValueErrors and the guarantee are its own — after the call
        every buffer of every rank holds the bytes of an engine built from the final tables.  A COLLECTIVE when `verify` is set and
        collectives are live: EVERY rank passes the SAME request (the whole update, not its own rows).  In this order: the request is
        validated; flush() installs the pending item-row all-gather of the last training update (its install() would otherwise
        overwrite freshly written rows of E); the ranks compare the digest of the request (dp.Collectives.agree: one all-gather of
        16 bytes and the ONE host synchronisation of the call — a disagreement raises TcarError on every rank, nothing written);
        one staged copy and ONE tcar_catalog_update_owned on the engine's stream: E, the key and category tables and the whole
        publish-time table of eval_step on every rank, the planes, the clipped time block (where it was clean: it stays clean), the
        one-hot row, the moments and the shard's publish times by the rank that owns the row; then the host copies.
        verify=False skips the comparison and with it the synchronisation: the caller vouches for the request.
        A changed publish time of an OWNED row marks this rank's inverted index stale (rebuilt in front of the next training step)."""
        ids, content, item_rows, mwdhm, keys, categories = req = self._update_request(ids, content, item_rows, mwdhm, keys, categories)
        self.flush()
        if verify:
            self.xch.agree(dp.update_digest(*req), device=self.dev)
        d = self._stage_update(ids, content, item_rows, mwdhm, keys, categories)
        oh = getattr(self, "s_oh16", None) if self.onehot else None          # the shard's one-hot plane, once its scoring family exists
        if mwdhm is not None and oh is not None:
            d.onehot, d.onehot_inner = oh.data_ptr(), 160
        ev_mw = getattr(self, "_ev_mw", None) if mwdhm is not None else None
        check(self.lib.tcar_catalog_update_owned(C.byref(self._catalog_ctx()), C.byref(d), self.n0, self.nl,
                                                 None if ev_mw is None else C.c_void_p(ev_mw.data_ptr()), self._stream()),
              "tcar_catalog_update_owned")
        # the host copies follow: load_params / export read the content, the index is rebuilt from the owned publish times
        if content is not None:
            if not self._content_own:
                self._content, self._content_own = np.array(self._content, dtype=np.float32), True
            self._content[1 + ids] = content
        if mwdhm is not None:
            if not self._mwdhm_full_own:
                self._mwdhm_full, self._mwdhm_full_own = np.array(self._mwdhm_full, dtype=np.int32), True
            self._mwdhm_full[ids] = mwdhm
            own = (ids >= self.n0) & (ids < self.n0 + self.nl)
            loc = ids[own] - self.n0
            if own.any() and (self._mwdhm_host[loc] != mwdhm[own]).any():
                self._mwdhm_host[loc] = mwdhm[own]
                self._index_stale = True

    # ---- retrieval, candidate scoring and the two-stage call over the shards (include/tcar_retrieve_shard.h; the collectives:
    # ShardExchange.retrieve / .candidates).  New names: they are COLLECTIVES with cap / T arguments, which the single-engine calls of
    # the same purpose (refused above) do not have.
    def retrieve_pieces(self, batch, C, k: Optional[int] = None, exclude_seen: bool = True, exclude=None,      # noqa: N803
                        panel: Optional[int] = None, window=None, cap: Optional[int] = None, T: Optional[int] = None) -> _RetrievePieces:
        """The armed local pieces of ONE ShardExchange.retrieve for this rank's sessions (`batch` None: none — then T and cap are
        needed); k None: a retrieval, else the two-stage call.  A caller that moves the buffers itself calls begin / prepare / fold /
        merge (/ scores / rerank) in that order.  The request is validated before any upload (TcarEngine._retrieve_request, the
        shard's padded rows as the panel bound).  No buffer of the catalog's width is touched."""
        self._refuse_ragged_shard(batch)
        panel = self._retrieve_request(C, k, panel, window, _ru(self.nl, 128))
        C_, k = int(C), (int(k) if k is not None else None)
        bt, cap, X, meta = self._gathered_inputs(batch, None, False, exclude_seen, exclude, window, cap, T, panel)
        Bq, rw = self.world * cap, 2 * C_ + 4
        self.ws.ensure([Spec("rs_state", (Bq, rw), I32), Spec("rs_merged", (cap, rw), I32), Spec("rs_ids", (cap, C_), I32),
                        Spec("rs_scores", (cap, C_), F32)])
        if k is not None:
            self.ws.ensure([Spec("rs_part", (Bq, C_), F32), Spec("rs_exact", (cap, C_), F32), Spec("rs_rank", (2, cap, C_), I32),
                            Spec("rs_topk", (cap, k), I32), Spec("rs_topscore", (cap, k), F32)])
        pc = getattr(self, "_retrieve_pc", None)
        if pc is None:
            pc = self._retrieve_pc = _RetrievePieces(self)
        pc.arm(bt, cap, C_, k, panel, meta, X, window is not None)
        return pc

    def cand_pieces(self, batch, candidates, clicked=None, cap: Optional[int] = None, T: Optional[int] = None,
                    C: Optional[int] = None) -> _CandPieces:      # noqa: N803
        """The armed local pieces of ONE ShardExchange.candidates (`batch` None: a rank without sessions — then T, cap and the list
        length C are needed).  The request is validated before any upload (TcarEngine._cand_request)."""
        self._refuse_ragged_shard(batch)
        if batch is not None:
            cand, clk = self._cand_request(self._sessions(batch), candidates, clicked)
            C_ = cand.shape[1]
        else:
            if isinstance(C, bool) or not isinstance(C, (int, np.integer)) or not 1 <= C <= self.CAND_MAX_C:
                raise ValueError("a rank without sessions needs the step's list length: C must be in [1, %d]" % self.CAND_MAX_C)
            cand, clk, C_ = None, None, int(C)
        bt, cap, _, meta = self._gathered_inputs(batch, None, False, False, None, None, cap, T, 128)
        self.ws.ensure([Spec("cs_in", (2, cap, C_), I32), Spec("rs_part", (self.world * cap, C_), F32), Spec("cs_score", (cap, C_), F32),
                        Spec("cs_rank", (2, cap, C_), I32), Spec("cs_counts", (cap, 3), I32), Spec("cs_metrics", (cap, 3), F32)])
        # cand and clicked are the two planes of ONE workspace entry: they go up in one copy; rows past the local batch: empty slots
        self.cs_in[0].fill_(-1)
        if cand is not None:
            if clk is None:
                self.cs_in[0, :cand.shape[0]].copy_(torch.from_numpy(cand))
            else:
                self.cs_in[:, :cand.shape[0]].copy_(torch.from_numpy(np.stack([cand, clk])))
        pc = getattr(self, "_cand_pc", None)
        if pc is None:
            pc = self._cand_pc = _CandPieces(self)
        pc.arm(bt, cap, C_, meta, clk is not None)
        return pc

    def shard_retrieve(self, batch, C, exclude_seen: bool = True, exclude=None, panel: Optional[int] = None, window=None,      # noqa: N803
                       cap: Optional[int] = None, T: Optional[int] = None):
        """TcarEngine.retrieve over the shards: (ids [B, C] int32, coarse_scores [B, C] f32) of this rank's sessions against the
        whole catalog — every shard's top-C state of the hi-plane scores, merged exactly (tcar_retrieve_merge).  A COLLECTIVE, as
        eval_step_streamed: `batch` = None on a rank without sessions, with T and cap; every rank passes exclusion lists of the same
        width.  Views of the workspace, valid until the next call."""
        pc = self.retrieve_pieces(batch, C, None, exclude_seen, exclude, panel, window, cap, T)
        out = self.xch.retrieve(pc, pc.cap, False)
        self.poll_fork_errors()
        return out

    def shard_recommend_two_stage(self, batch, k: int = 20, shortlist: int = 256, exclude_seen: bool = True, exclude=None,
                                  panel: Optional[int] = None, window=None, cap: Optional[int] = None, T: Optional[int] = None,
                                  diversity=None):
        """TcarEngine.recommend_two_stage over the shards: (topk [B, k] int32, scores [B, k] f32), the k best of the shortlist's exact
        scores, each slot scored by the shard that owns its row (the bits a whole-catalog engine computes from the same operands).
        A COLLECTIVE, as shard_retrieve.  `last_shortlist` / `last_exact` hold the shortlist [B, shortlist] and its exact scores.
        diversity: refused — the MMR walk of include/tcar_mmr.h is not run over shards yet (every rank keeps the fp32 image E whole,
        so the owner rank of a session could run it)."""
        self._refuse_diversity(diversity)
        pc = self.retrieve_pieces(batch, shortlist, k, exclude_seen, exclude, panel, window, cap, T)
        out = self.xch.retrieve(pc, pc.cap, True)
        self.poll_fork_errors()
        self.last_shortlist, self.last_exact = self.rs_ids[:pc.B], self.rs_exact[:pc.B]
        return out

    def shard_score_candidates(self, batch, candidates, clicked=None, cap: Optional[int] = None, T: Optional[int] = None,
                               C: Optional[int] = None) -> CandResult:      # noqa: N803
        """TcarEngine.score_candidates over the shards: CandResult of this rank's sessions; every slot is scored by the shard that
        owns its row.  A COLLECTIVE: `batch` = None on a rank without sessions, with T, cap and the list length C; every rank passes
        lists of the same length."""
        pc = self.cand_pieces(batch, candidates, clicked, cap, T, C)
        out = self.xch.candidates(pc, pc.cap)
        self.poll_fork_errors()
        return out

    # ------------------------------------------------------------------------------ inspection (tests, export)
    def _item_rows_full(self, local: torch.Tensor) -> np.ndarray:
        """this rank's [nl, ldh] rows of a candidate-side table -> the whole [N + 1, H] table in the reference's shape (row 0
        = the pad row, zero).  A COLLECTIVE: every rank calls it — and so export_state and export_grads are collectives here
        (the Adam moments and the gradient of the item table live on their owners; every rank gets the full state,
        host/model.py lets rank 0 write the file).  load_state: every rank reads the same file and keeps the rows of its shard."""
        g = self.geo
        mine = torch.zeros(self.S, g.ldh, dtype=torch.float32, device=self.dev)
        mine[:self.nl] = local
        full = self.xch.all_gather(mine)             # [W, S, ldh], rank-major
        item = np.zeros((g.N + 1, g.H), dtype=np.float32)
        item[1:] = full.view(-1, g.ldh)[:g.N, :g.H].cpu().numpy()
        return item


