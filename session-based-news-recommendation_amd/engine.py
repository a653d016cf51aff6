"""Device-resident TCAR model state and the per-batch step, driving the C-ABI of include/tcar_hip.h.

PyTorch is used here for three things only: device memory (tensors as buffers), the current HIP stream, and
(in `dp.py`) torch.distributed.  Every arithmetic operation of the step is a hand-written gfx950 kernel behind
`libtcar_hip.so`; there is no eager/CPU fallback — constructing an engine without the library or a GPU raises.

HBM layout (fp32, "padded-concat space", see include/tcar_hip.h):
  E        [Npad, ek]   candidate matrix: item table | frozen content | clipped candidate time vectors.
                        The trainable item table LIVES in E[:, 0:ldh] (no per-step concat / copy,
                        model_combine.py:135-136); Npad = N rounded up to 64, padding rows are zero.
  W/G/M/V  flat arenas  the other 22 trainable variables (padded), their gradients and Adam moments, at identical
                        offsets; the tables that receive atomic adds come first so one memset clears them.
  Gi/Mi/Vi [N, ldh]     item-table gradient and Adam moments.
  work     per-batch activations sized for the largest (B, T) seen.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import OrderedDict
from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._lib import Batch, Cand, Dims, Grads, Ragged, Rerank, Retrieve, Sections, Segments, Quota, Serve, Tables, Window, check
from .oplevel import OpLevelStep
from .workspace import F32, HOST_I32, I32, U8, ScoreForm, Spec, Workspace, ru as _ru, scoring_specs

TIME_NAMES = ["month_embedding", "day_embedding", "week_embedding", "hour_embedding", "minute_embedding"]
TIME_SHORT = [n[:-len("_embedding")] for n in TIME_NAMES]           # their arena names (ARENA below)
TIME_VOCAB = [13, 32, 8, 25, 61]
TABLE_VARS = ["dec_pos", "duration_embedding"] + TIME_NAMES          # gathered tables: IndexedSlices norm pieces only
# TF creation order of the 23 trainable variables (model_combine.py:52-128) = squared-norm slot index
VAR_ORDER = ["item_emb", "dec_pos"] + TIME_NAMES + ["duration_embedding",
             "multi_attention/input_linear_trans/w_3d", "multi_attention/cont_linear_trans/w_3d",
             "multi_attention/inter_linear_trans/w_3d", "multi_attention/res_linear_trans/w_3d",
             "multi_attention/query_trans1/w1", "multi_attention/query_trans1/b1",
             "multi_attention/query_trans2/w1", "multi_attention/query_trans2/b1",
             "attout_item_cont_trans/w1", "attout_item_cont_trans/b1",
             "cont_attention/input_linear_trans/w_3d", "cont_attention/cont_linear_trans/w_3d",
             "cont_attention/res_linear_trans/w_3d", "attout_pt_trans/w1", "attout_pt_trans/b1"]
SLOT = {n: i for i, n in enumerate(VAR_ORDER)}
# Variables whose gradient is accumulated in a fixed order by the fused step of the split-bf16 modes (bitwise repeatable from
# step to step): ALL of them — the item table (sorted segmented sum, csrc/segsum.hip), the seven small tables (one workgroup
# per destination row, sources in order, embed.hip), the nine weight matrices (un-split K up to 1,536 batch rows: longer
# batches split K with float atomics), the four biases and the two residual weights (column sums in a fixed order).  In fp32
# mode the biases and residual weights still go through float atomics (ATOMIC_IN_F32).
# tests/test_gpu_configs.py::test_same_step_twice_bitwise_report keeps both lists honest.
DETERMINISTIC_GRADS: tuple = tuple(VAR_ORDER)
ATOMIC_IN_F32: tuple = tuple(n for n in VAR_ORDER if n.endswith("/b1") or n.endswith("res_linear_trans/w_3d"))


class Geometry:
    def __init__(self, n_items: int, H: int, Ht: int):
        self.N, self.H, self.Ht = int(n_items), int(H), int(Ht)
        self.ldh = _ru(H, 64)
        self.ldt = 64 if Ht <= 64 else (128 if Ht <= 128 else 256)
        if self.ldh > 512 or Ht > 256 or 5 * self.ldt > 512:
            raise ValueError("unsupported hidden sizes for the gfx950 kernels: H<=512, Ht<=64 (5*ldt<=512)")
        self.ic, self.pt, self.ct = 2 * self.ldh, 5 * self.ldt, 2 * self.ldt
        self.ek = self.ic + self.pt
        self.Npad = _ru(self.N, 128)        # KB32 planes are blocked in 128-row units

    def idx(self, kind: str) -> np.ndarray:
        """logical index -> padded index for a dimension of the given kind."""
        H, Ht, ldh, ldt = self.H, self.Ht, self.ldh, self.ldt
        if kind == "H":
            return np.arange(H)
        if kind == "2H":
            return np.concatenate([np.arange(H), ldh + np.arange(H)])
        if kind == "T":
            return np.arange(Ht)
        if kind == "2T":
            return np.concatenate([np.arange(Ht) + k * ldt for k in range(2)])
        if kind == "5T":
            return np.concatenate([np.arange(Ht) + k * ldt for k in range(5)])
        if kind.startswith("V"):
            return np.arange(int(kind[1:]))
        raise KeyError(kind)

    def padded(self, kind: str) -> int:
        return {"H": self.ldh, "2H": self.ic, "T": self.ldt, "2T": self.ct, "5T": self.pt}.get(kind) or int(kind[1:])


# (short name, reference variable name, row kind, col kind or None for vectors); order = arena order.
# First block = accumulated with atomics (zeroed every step); time tables + dur contiguous (tcar_grads_t).
ARENA = [
    ("pos", "dec_pos", "V40", "H"),
    ("month", "month_embedding", "V13", "T"), ("day", "day_embedding", "V32", "T"),
    ("week", "week_embedding", "V8", "T"), ("hour", "hour_embedding", "V25", "T"),
    ("minute", "minute_embedding", "V61", "T"), ("dur", "duration_embedding", "V11", "T"),
    ("m_wres", "multi_attention/res_linear_trans/w_3d", "H", None),
    ("s_wres", "cont_attention/res_linear_trans/w_3d", "H", None),
    # ---- written by GEMM / column-sum epilogues (no zeroing needed)
    ("m_win", "multi_attention/input_linear_trans/w_3d", "2H", "H"),
    ("m_wc", "multi_attention/cont_linear_trans/w_3d", "H", "H"),
    ("m_wint", "multi_attention/inter_linear_trans/w_3d", "T", "H"),
    ("q1_w", "multi_attention/query_trans1/w1", "2T", "H"), ("q1_b", "multi_attention/query_trans1/b1", "H", None),
    ("q2_w", "multi_attention/query_trans2/w1", "H", "2H"), ("q2_b", "multi_attention/query_trans2/b1", "2H", None),
    ("o_w", "attout_item_cont_trans/w1", "2H", "2H"), ("o_b", "attout_item_cont_trans/b1", "2H", None),
    ("s_win", "cont_attention/input_linear_trans/w_3d", "5T", "H"),
    ("s_wc", "cont_attention/cont_linear_trans/w_3d", "H", "H"),
    ("ot_w", "attout_pt_trans/w1", "5T", "5T"), ("ot_b", "attout_pt_trans/b1", "5T", None),
]
N_ATOMIC = 9


_HP_STREAMS: Dict[int, "torch.cuda.Stream"] = {}


def use_priority_stream(dev: torch.device) -> None:
    """Make ONE process-wide high-priority stream the current stream of `dev`.  The main chain of a step (logits ->
    softmax -> dX -> the long tail of small kernels -> Adam) is the critical path, the aux stream's dE GEMM and
    candidate-time work have slack: with the main chain on a priority -1 stream its workgroups are dispatched first
    whenever both streams have work queued (measured 0.752 -> 0.731 ms per step).  Setting the current stream once
    (instead of entering / leaving a stream per step) costs no per-step events.
    SIDE EFFECT: torch.cuda.current_stream(dev) changes for the whole process; code that mixes the engine with launches
    on the NULL stream must pass torch.cuda.current_stream().cuda_stream instead.  TCAR_NO_PRIO=1 disables it."""
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    hp = _HP_STREAMS.get(idx)
    if hp is None:
        hp = _HP_STREAMS[idx] = torch.cuda.Stream(dev, priority=-1)
    cur = torch.cuda.current_stream(dev)
    if cur != hp:
        hp.wait_stream(cur)
        torch.cuda.set_stream(hp)


class Switches(NamedTuple):
    """The Python-level TCAR_* environment switches of the engines, read ONCE per engine, at construction (`Switches.read`).  (The
    switches of tcar_tuning_t are `_lib.tuning`, those of the collectives `dp.Collectives`.)"""
    no_prio: bool; no_overlap: bool; atomic_colsums: bool; atomic_wgrad: bool; no_onehot: bool; no_onehot_bwd: bool
    no_ce_anchor: bool; no_stream3: bool; no_flag_fork: bool; no_fold_scratch: bool; shard_all_flags: bool
    shard_materialised: bool; shard_py_step: bool
    splitk: int                                   # TCAR_SPLITK (0: not set)

    @classmethod
    def read(cls) -> "Switches":
        env = os.environ.get
        return cls(*[bool(env("TCAR_" + f.upper())) for f in cls._fields[:-1]], splitk=int(env("TCAR_SPLITK") or 0))


class StepForm(NamedTuple):
    """Which optional pointers a tcar_ctx_t carries — that IS the step's algorithm: fused_ce / onehot_fwd / onehot_bwd / ce_anchored /
    sorted_rows of csrc/step.hip are predicates over them.  Decided in one place per engine kind (TcarEngine._form)."""
    score: ScoreForm
    det_colsums: bool         # gw_rows: bias / residual-weight gradients as order-fixed column sums
    wgrad_ks: int             # wgrad_slabs: rows per K split of the weight gradients, folded in split order (0: none, float atomics)
    sorted_rows: bool         # stream2 + segsum_ws + small_det_ws: second stream, order-fixed item-row and small-table sums
    stream3: bool; flag_forks: bool; fold_scratch: bool


# The per-batch activations of tcar_ctx_t ("workspace"): (attribute = field, rows kind, columns, dtype, fill).  Rows kinds: "r" =
# session-item rows B * T, "B" = sessions; columns: an attribute of Geometry, a number, None = a vector.
WORK = ([(n, "r", c, F32, None) for n, c in (("x_icp", "ic"), ("x_pt", "pt"), ("x_act", "ldt"), ("pre1", "ldh"), ("pre2", "ldh"),
                                             ("dx_icp", "ic"), ("dx_pt", "pt"), ("dx_act", "ldt"), ("dpre1", "ldh"), ("dpre2", "ldh"))]
        + [("alpha", "3r", None, F32, None)]
        + [(n, "B", c, F32, None) for n, c in (("click_t", "ct"), ("q1", "ldh"), ("q", "ic"), ("pooled", "ek"), ("attout", "ek"),
                                               ("ce", None), ("dattout", "ek"), ("dpooled", "ek"), ("dq", "ic"), ("dq1", "ldh"),
                                               ("gw_rows", "ic"),        # per-session d w_res rows (tcar_colsum_det)
                                               ("dclick", "ct"))]
        + [(n, "B", c, F32, 0) for n, c in (("neg_fb", None), ("loss", None), ("neg_coef", None), ("negpart", "ic"))]
        + [("rank", "B", None, I32, None), ("topk", "B", 20, I32, None)])
# tcar_ctx_t fields that take the engine attribute of the same name: parameters / optimizer state, then the workspace
CTX_STATE = ["E", "W", "Gx", "M", "V", "big", "Mi", "Vi", "sqn_dense", "use_dense", "mwdhm", "inv_n", "inv_off", "ct_ws", "et_perm",
             "adam_bitmap"]
CTX_WS = ["x_icp", "x_pt", "x_act", "click_t", "pre1", "pre2", "q1", "q", "alpha", "pooled", "attout", "logits", "ce", "neg_fb", "loss",
          "neg_coef", "negpart", "dattout", "dpooled", "dq", "dq1", "dclick", "slabs", "dx_icp", "dx_pt", "dx_act", "dpre1", "dpre2"]
# the element-count field that goes with a pointer field
CTX_SIZES = {"wgrad_slabs": "wgrad_slab_floats", "proj_slabs": "proj_slab_floats", "ce_ws": "ce_ws_floats", "segsum_ws": "segsum_bytes",
             "small_det_ws": "small_det_ws_floats", "fold_scratch": "fold_scratch_words"}


class TcarEngine(OpLevelStep):
    def __init__(self, params: Dict[str, np.ndarray], content_emb: np.ndarray, mwdhm: np.ndarray, lr: float = 1e-3,
                 max_grad: Optional[float] = 150.0, neg_weight: float = 0.01, device: str = "cuda:0",
                 splitk: Optional[int] = None, scoring: str = "f32", shard: Optional[tuple] = None,
                 switches: Optional["Switches"] = None):
        """shard = (n0, n_loc): catalog-sharded data parallelism (sharded.py) — the candidate-side state (bf16 planes of E,
        dense item gradient, candidate-time block, Adam moments, inverted index) covers the catalog rows [n0, n0 + n_loc)
        only; E itself stays whole (the session-side gathers read any row)."""
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.TcarError("TcarEngine needs an MI355X (no CPU fallback)")
        self.dev = torch.device(device)
        self.is_cuda = self.dev.type == "cuda"
        self.sw = sw = switches or Switches.read()
        if self.overlap is None:
            self.overlap = not sw.no_overlap
        if self.is_cuda and self.overlap and self.native and self.priority_stream and not sw.no_prio:
            use_priority_stream(self.dev)
        self.ws = Workspace(self, self.dev)
        N, H = content_emb.shape[0] - 1, content_emb.shape[1]
        Ht = params["month_embedding"].shape[1]
        self.geo = g = Geometry(N, H, Ht)
        self.lr, self.max_grad, self.neg_weight = float(lr), max_grad, float(neg_weight)
        self.b1, self.b2, self.eps = 0.9, 0.999, 1e-8
        self.b1_pow, self.b2_pow = np.float32(self.b1), np.float32(self.b2)
        self.step = 0
        # split-K of dX = dlogits E (slabs + reduce): 16 in fp32; 18 in the mixed mode (64 from 2^20 catalog rows, where the GEMM takes
        # its 256 x 384 tile); 36 in the materialised-logits bf16 modes (profiles/r04_ab_experiments.txt, r06_ab_experiments.txt)
        big_catalog = int(np.asarray(content_emb).shape[0]) - 1 >= (1 << 20)
        self.splitk = sw.splitk or splitk or (16 if scoring == "f32" else (64 if big_catalog else 18) if scoring == "bf16x3-mixed" else 36)
        # precision of the three full-catalog scoring GEMMs: "f32" (fp32 MFMA), "bf16x3" (split-bf16 planes, three
        # bf16 MFMAs per product, fp32-class accuracy), "bf16" (hi plane only)
        # "bf16x3-mixed": logits in bf16x3 (fp32-class), the two gradient GEMMs in plain bf16 (mixed-precision backward)
        if scoring not in ("f32", "bf16x3", "bf16x3-mixed", "bf16"):
            raise ValueError("scoring must be f32 | bf16x3 | bf16x3-mixed | bf16")
        self.scoring = scoring
        self.scoring_code = {"f32": 0, "bf16": 1, "bf16x3": 3, "bf16x3-mixed": 3}[scoring]
        self.scoring_bwd = 1 if scoring == "bf16x3-mixed" else 0
        f32 = dict(dtype=torch.float32, device=self.dev)
        # arena layout ------------------------------------------------------------------------------------
        self.seg = OrderedDict()
        off = 0
        for short, ref, rk, ck in ARENA:
            rows = g.padded(rk)
            cols = g.padded(ck) if ck else 1
            n = rows * cols
            self.seg[short] = dict(off=off, rows=rows, cols=cols, n=n, ref=ref, rk=rk, ck=ck, slot=SLOT[ref])
            off += n
        self.arena_n = off
        self.atomic_n = sum(self.seg[a[0]]["n"] for a in ARENA[:N_ATOMIC])
        self.W = torch.zeros(off, **f32)
        # gradients + the per-row norm pieces live in ONE buffer (a single all-reduce in the data-parallel path)
        self.Gx = torch.zeros(off + _lib.NSLOT, **f32)
        self.G = self.Gx[:off]
        self.M = torch.zeros(off, **f32)
        self.V = torch.zeros(off, **f32)
        self.E = torch.zeros(g.Npad, g.ek, **f32)
        self.shard = (0, g.N) if shard is None else (int(shard[0]), int(shard[1]))
        n0, nl = self.shard                       # candidate-side state covers rows [n0, n0 + nl)
        nlpad = _ru(nl, 128)
        if self.scoring_code:
            self.e16h = torch.zeros(nlpad, g.ek, dtype=torch.bfloat16, device=self.dev)
            self.e16l = torch.zeros(nlpad, g.ek, dtype=torch.bfloat16, device=self.dev)
        # dense item-table gradient and the candidate-side time block of dE, contiguous for the same reason
        self.big = torch.zeros(nl * (g.ldh + g.pt), **f32)
        self.Gi = self.big[:nl * g.ldh].view(nl, g.ldh)
        self.d_et = self.big[nl * g.ldh:].view(nl, g.pt)
        self.Mi = torch.zeros(nl, g.ldh, **f32)
        self.Vi = torch.zeros(nl, g.ldh, **f32)
        self.sqn_dense = torch.zeros(_lib.NSLOT, **f32)
        self.sqn_pieces = self.Gx[off:]
        use = np.ones(_lib.NSLOT, dtype=np.int32)
        for n in TABLE_VARS:
            use[SLOT[n]] = 0
        self.use_dense = torch.tensor(use, device=self.dev)
        # (a host copy of its own: update_items writes it, and the index below is rebuilt from it)
        self._mwdhm_host = np.array(np.asarray(mwdhm)[n0:n0 + nl], dtype=np.int32, order="C")
        self.mwdhm = torch.tensor(self._mwdhm_host, device=self.dev)
        self.dims = Dims(g.N, g.H, g.Ht, g.ldh, g.ldt)
        self.dims_cand = Dims(nl, g.H, g.Ht, g.ldh, g.ldt)        # the candidate-side kernels see the shard as a catalog
        self._build_time_index()
        self.adam_bitmap = torch.zeros(((nl + 31) // 32 + 15) // 16 * 16, dtype=torch.int32, device=self.dev)   # split update marks, whole 64-byte units
        self.ct_ws = torch.zeros(self.lib.tcar_cand_time_ws_floats(C.byref(self.dims_cand)), **f32)
        # segment tables for the optimizer kernels
        self.segs_all = self._segments([a[0] for a in ARENA])
        self.segs_dense = self._segments([a[0] for a in ARENA if a[1] not in TABLE_VARS])
        self._use_np = use
        self.load_params(params, content_emb)
        self.work_rows, self.work_B = 0, 0
        self._time_dirty = True
        self.pin = None

    def _segments(self, names) -> Segments:
        s = Segments()
        s.nseg = len(names)
        for i, n in enumerate(names):
            sg = self.seg[n]
            s.off[i], s.len[i], s.slot[i] = sg["off"], sg["n"], sg["slot"]
        return s

    _index_stale = False      # update_items changed publish times: the index below is rebuilt in front of the next training step

    def _build_time_index(self):
        """The static inverted index of publish_time_MWDHM (the host copy `_mwdhm_host` of the rows this engine owns): candidates
        listed per time-table row (cand_time_bwd_indexed).  Built when the engine is; rebuilt INTO the same device buffers — the
        pointers a context carries stay valid — in front of the first training step after update_items changed a publish time."""
        nl = self.shard[1]
        mw = self._mwdhm_host.astype(np.int64)
        rowoff = np.array([0, 13, 45, 53, 78])
        key = (np.clip(mw, 0, np.array(TIME_VOCAB) - 1) + rowoff[None, :]).T.reshape(-1)          # [5N], k-major
        order = np.argsort(key, kind="stable")
        inv_off = np.zeros(140, dtype=np.int32)
        inv_off[1:] = np.cumsum(np.bincount(key, minlength=139))
        # inverse of the index: position of (k, n) in list order.  In the bf16 scoring modes the dE GEMM writes the time
        # block of dE in THAT order (tcar_gemm_bf16_perm), so the candidate-time backward streams contiguous lists
        et_perm = np.empty(5 * nl, dtype=np.int32)
        et_perm[order] = np.arange(5 * nl, dtype=np.int32)
        for name, host in (("inv_n", (order % nl).astype(np.int32)), ("inv_off", inv_off), ("et_perm", et_perm)):
            if getattr(self, name, None) is None:
                setattr(self, name, torch.tensor(host, device=self.dev))
            else:
                getattr(self, name).copy_(torch.from_numpy(host))
        self._index_stale = False

    # --------------------------------------------------------------------------------- parameter (un)packing
    def load_params(self, params: Dict[str, np.ndarray], content_emb: Optional[np.ndarray] = None):
        if getattr(self, "_pending_lr", None) is not None:
            self.flush()
        g = self.geo
        self.W.copy_(torch.from_numpy(self._pack_arena(params)))
        if content_emb is not None:
            self._content = np.asarray(content_emb, dtype=np.float32)
            self._content_own = False         # (may be the caller's array: update_items copies it before its first write)
        item = np.asarray(params["item_emb"], dtype=np.float32)
        # the candidate matrix is assembled on the device in row chunks: no [Npad, ek] host image (33 GB at 10 M items)
        self.E.zero_()
        for lo in range(0, g.N, 1 << 20):
            hi = min(g.N, lo + (1 << 20))
            self.E[lo:hi, :g.H].copy_(torch.from_numpy(np.ascontiguousarray(item[1 + lo:1 + hi])))
            self.E[lo:hi, g.ldh:g.ldh + g.H].copy_(torch.from_numpy(np.ascontiguousarray(self._content[1 + lo:1 + hi])))
        if self.scoring_code:
            n0, nl = self.shard
            check(self.lib.tcar_split_bf16(self._p(self.E, n0 * g.ek), g.ek, nl, g.ek, self._p(self.e16h), self._p(self.e16l),
                                           g.ek, None, None, 0, 0, 0, self._stream()), "tcar_split_bf16")
        self._item_row0 = np.asarray(params["item_emb"], dtype=np.float32)[0].copy()
        self._time_dirty = True

    def _pack_arena(self, values: Dict[str, np.ndarray]) -> np.ndarray:
        """reference-shaped arrays of the 22 arena variables -> one padded flat fp32 arena (pads zero)"""
        g = self.geo
        W = np.zeros(self.arena_n, dtype=np.float32)
        for short, sg in self.seg.items():
            src = np.asarray(values[sg["ref"]], dtype=np.float32)
            dst = W[sg["off"]:sg["off"] + sg["n"]].reshape(sg["rows"], sg["cols"])
            ri = g.idx(sg["rk"])
            if sg["ck"] is None:
                dst[ri, 0] = src.reshape(-1)
            else:
                dst[np.ix_(ri, g.idx(sg["ck"]))] = src
        return W

    # ------------------------------------------------------------------------------------- checkpoint state
    def _probe_flag_forks(self) -> bool:
        """tcar_flag_fork_selftest: a polling kernel on the aux stream and a kernel enqueued behind it on the main stream"""
        ok = C.c_int32(0)
        check(self.lib.tcar_flag_fork_selftest(self._sig.data_ptr(), self._stream(), self._aux.cuda_stream, C.byref(ok)),
              "tcar_flag_fork_selftest")
        return bool(ok.value)

    _FORK_MSG = ("%d flag-fork poll(s) timed out: the step's streams are not running concurrently and a consumer may have run "
                 "ahead of its producer — results since the last check are invalid (set TCAR_FLAG_FORK=0 to fork with events)")

    def poll_fork_errors(self):
        """Fail fast, WITHOUT synchronising: a poll that gives up also counts in a pinned host word (tcar_ctx_t.sig_err_host,
        system-scope atomic), which the host reads here after every step.  A time-out is seen at most a step or two after it
        happened (the host runs ahead of the device by that much), long before an epoch ends or anything is reported."""
        eh = getattr(self, "_sig_err_np", None)
        if eh is not None and eh[0]:
            raise RuntimeError(self._FORK_MSG % int(eh[0]))

    def check_forks(self):
        """Raise if a polling kernel of a flag fork (tcar_ctx_t.sig_dev) ever gave up waiting: the side streams did not run
        beside the main stream (kernels serialised by a profiler's counter collection, or streams sharing one hardware queue),
        and a consumer may have run ahead of its producer.  Synchronises the device; called wherever the host reads results
        back: every evaluation step, export_state / export_params (checkpoints), the training loop's epoch end, bench.py after
        its timed loop.  Between those, poll_fork_errors() tests the host-visible mirror after every training step."""
        if getattr(self, "_sig", None) is not None:
            n = int(self._sig[32].item())
            if n:
                raise RuntimeError(self._FORK_MSG % n)
        self.poll_fork_errors()

    def _item_rows_full(self, local: torch.Tensor) -> np.ndarray:
        """the [n_loc, ldh] rows this engine holds of a candidate-side table -> the whole [N + 1, H] table (row 0 = the pad row, zero)"""
        g = self.geo
        item = np.zeros((g.N + 1, g.H), dtype=np.float32)
        item[1:] = local[:, :g.H].cpu().numpy()
        return item

    def _item_rows_mine(self, full: np.ndarray) -> np.ndarray:
        """inverse: the whole [N + 1, H] table -> the [n_loc, ldh] rows this engine holds"""
        g, (n0, nl) = self.geo, self.shard
        it = np.zeros((nl, g.ldh), dtype=np.float32)
        it[:, :g.H] = full[1 + n0:1 + n0 + nl]
        return it

    def export_state(self) -> Dict[str, np.ndarray]:
        """Everything a resumed run needs, as plain arrays (np.savez, loadable with allow_pickle=False): the 23 variables
        `var/<name>`, the Adam moments `m/<name>`, `v/<name>` in the reference's shapes, the beta powers and the step
        count (tf.train.AdamOptimizer's beta1_power / beta2_power non-slot variables, model_combine.py:155)."""
        self.flush()
        self.check_forks()
        out = {"var/" + k: v for k, v in self.export_params().items()}
        for tag, arena, item in (("m/", self.M, self.Mi), ("v/", self.V, self.Vi)):
            d = self._unpack_arena(arena.cpu().numpy())
            d["item_emb"] = self._item_rows_full(item)
            out.update({tag + k: d[k] for k in VAR_ORDER})
        out["meta/step"] = np.asarray(self.step, dtype=np.int64)
        out["meta/beta_pow"] = np.asarray([self.b1_pow, self.b2_pow], dtype=np.float32)
        return out

    def load_state(self, st) -> None:
        """Inverse of export_state (moments / powers / step are optional: a variables-only file restores the weights)."""
        self.load_params({k[4:]: np.asarray(st[k]) for k in st if k.startswith("var/")})
        if all(("m/" + k) in st and ("v/" + k) in st for k in VAR_ORDER):
            for tag, arena, item in (("m/", self.M, self.Mi), ("v/", self.V, self.Vi)):
                vals = {k: np.asarray(st[tag + k]) for k in VAR_ORDER}
                arena.copy_(torch.from_numpy(self._pack_arena(vals)))
                item.copy_(torch.from_numpy(self._item_rows_mine(vals["item_emb"])))
        if "meta/step" in st:
            self.step = int(np.asarray(st["meta/step"]))
        if "meta/beta_pow" in st:
            bp = np.asarray(st["meta/beta_pow"], dtype=np.float32)
            self.b1_pow, self.b2_pow = np.float32(bp[0]), np.float32(bp[1])

    def _unpack_arena(self, flat: np.ndarray) -> "OrderedDict[str, np.ndarray]":
        g = self.geo
        out = {}
        for short, sg in self.seg.items():
            src = flat[sg["off"]:sg["off"] + sg["n"]].reshape(sg["rows"], sg["cols"])
            ri = g.idx(sg["rk"])
            if sg["ck"] is None:
                v = src[ri, 0]
                out[sg["ref"]] = v.reshape(-1, 1).copy() if sg["ref"].endswith("w_3d") else v.copy()
            else:
                out[sg["ref"]] = src[np.ix_(ri, g.idx(sg["ck"]))].copy()
        return out

    def export_params(self) -> "OrderedDict[str, np.ndarray]":
        """All 23 trainable variables in the reference's shapes."""
        self.flush()
        self.check_forks()
        g = self.geo
        out = self._unpack_arena(self.W.cpu().numpy())
        item = np.zeros((g.N + 1, g.H), dtype=np.float32)
        item[0] = self._item_row0
        item[1:] = self.E[:g.N, :g.H].cpu().numpy()
        out["item_emb"] = item
        return OrderedDict((k, out[k]) for k in VAR_ORDER)

    def export_grads(self) -> "OrderedDict[str, np.ndarray]":
        """Summed dense gradients of the last backward, reference shapes (item row 0 has no gradient)."""
        out = self._unpack_arena(self.G.cpu().numpy())
        out["item_emb"] = self._item_rows_full(self.Gi)
        return OrderedDict((k, out[k]) for k in VAR_ORDER)

    def export_sqnorms(self) -> Dict[str, float]:
        d = self.sqn_dense.cpu().numpy().astype(np.float64)
        p = self.sqn_pieces.cpu().numpy().astype(np.float64)
        return {n: float(self._use_np[i] * d[i] + p[i]) for i, n in enumerate(VAR_ORDER)}

    # ------------------------------------------------------------------------------------------- workspace
    def _ensure_work(self, B: int, T: int, rows: Optional[int] = None):
        """the workspace covers the largest row count (B * T; `rows` = R of a ragged batch) and the largest B seen (WORK + the
        materialised part of the scoring family)"""
        g, kinds = self.geo, ()
        rows = B * T if rows is None else int(rows)
        if rows > self.work_rows:
            self.work_rows, kinds = rows, ("r", "3r")
        if B > self.work_B:
            self.work_B, kinds = B, kinds + ("B",)
        if kinds:
            rows = {"r": self.work_rows, "3r": 3 * self.work_rows, "B": self.work_B}
            self.ws.ensure(Spec(n, (rows[k],) if c is None else (rows[k], getattr(g, c) if isinstance(c, str) else c), dt, fill)
                           for n, k, c, dt, fill in WORK if k in kinds)
            if "B" in kinds:
                self.ws.ensure(self._scoring_specs(ScoreForm(planes=bool(self.scoring_code))))

    def _scoring_specs(self, form: ScoreForm) -> List[Spec]:
        """the scoring family of this engine: work_B sessions against the WHOLE catalog (also where it owns a shard of the candidate
        side: the one-hot forms exist only where it owns all of it); the optional buffers carry a leading underscore"""
        plain = ("slabs", "logits", "a16h", "a16l", "ap16h", "ap16l", "dl16h", "dl16l")
        return scoring_specs(self.geo, self.work_B, self.geo.N, self.splitk, form, lambda f: f if f in plain else "_" + f,
                             self._fill_onehot)

    def _fill_onehot(self, oh16: torch.Tensor):
        """the static one-hot plane of publish_time_MWDHM of the candidate rows this engine owns"""
        check(self.lib.tcar_time_onehot(C.byref(self.dims_cand), self._p(self.mwdhm), self._p(oh16), 160, self._stream()),
              "tcar_time_onehot")

    # --------------------------------------------------------------------------------------------- helpers
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    @staticmethod
    def _p(t: torch.Tensor, off: int = 0):
        return C.c_void_p(t.data_ptr() + 4 * off)

    def _w(self, name: str):
        return C.c_void_p(self.W.data_ptr() + 4 * self.seg[name]["off"])

    def _g(self, name: str):
        return C.c_void_p(self.G.data_ptr() + 4 * self.seg[name]["off"])

    def make_resident(self, batch: Dict[str, np.ndarray]) -> Batch:
        """Upload a batch into its OWN device buffer (kept alive by the engine) and return its descriptor.  The staging
        state of upload() (pinned double buffer, events, cursor) is saved and restored as a whole, so uploads before and
        after are unaffected."""
        names = ("pin", "pin_np", "ibufs", "pin_evt", "pin_used", "pin_i")
        save = {n: getattr(self, n, None) for n in names}
        self.pin = None
        try:
            bt = self.upload(batch)
            torch.cuda.current_stream(self.dev).synchronize()
            self._resident = getattr(self, "_resident", []) + [self.ibufs]
        finally:
            for n in names:
                setattr(self, n, save[n])
        return bt

    def _tables(self) -> Tables:
        t = Tables()
        t.E = self.E.data_ptr()
        t.pos = self._w("pos").value
        for k, n in enumerate(TIME_SHORT):
            t.time[k] = self._w(n).value
        t.dur = self._w("dur").value
        return t

    def _grads(self) -> Grads:
        gr = Grads()
        gr.g_item = self.Gi.data_ptr()
        gr.g_pos = self._g("pos").value
        for k, n in enumerate(TIME_SHORT):
            gr.g_time[k] = self._g(n).value
            gr.slot_time[k] = SLOT[TIME_NAMES[k]]
        gr.g_dur = self._g("dur").value
        gr.sqn = self.sqn_pieces.data_ptr()
        gr.slot_item, gr.slot_pos, gr.slot_dur = SLOT["item_emb"], SLOT["dec_pos"], SLOT["duration_embedding"]
        return gr

    def _time_ptrs(self):
        arr = (C.c_void_p * 5)()
        for k, n in enumerate(TIME_SHORT):
            arr[k] = self._w(n).value
        return arr

    # ----------------------------------------------------------------------------------------------- batch
    def upload(self, batch: Dict[str, np.ndarray]) -> Batch:
        """Pack the feed arrays into ONE int32 buffer, one H2D copy; returns the C batch descriptor."""
        ragged = "len" in batch                  # a ragged feed (sessions of mixed lengths): flat [R] rows + len [B]
        if ragged:
            parts, B, T, rows = self._ragged_parts(batch)
            K = 0
        else:
            seq = np.ascontiguousarray(batch["seq"], dtype=np.int32)
            B, T = seq.shape
            rows = B * T
            if T > 40:
                raise IndexError("session longer than the 40-row position table (model_combine.py:57)")
            if seq.min() < 1 or seq.max() > self.geo.N:
                raise IndexError("item id outside [1, N]")
            neg = batch.get("neg", None)
            K = 0 if neg is None or np.asarray(neg).size == 0 else np.asarray(neg).shape[1]
            parts = [seq.reshape(-1)] + [np.asarray(batch[k], dtype=np.int32).reshape(-1) for k in
                                         ("pm", "pd", "pw", "ph", "pmi", "gap", "cw", "ch", "label")]
            if K:
                parts.append(np.asarray(neg, dtype=np.int32).reshape(-1))
        total = sum(x.size for x in parts)
        if self.pin is None or self.pin[0].numel() < total:
            n = max(total, 1 << 16)
            self.pin = [torch.empty(n, dtype=torch.int32).pin_memory() for _ in range(2)]
            self.pin_np = [t.numpy() for t in self.pin]          # numpy views of the pinned staging buffers
            self.ibufs = [torch.empty(n, dtype=torch.int32, device=self.dev) for _ in range(2)]
            self.pin_evt = [torch.cuda.Event(), torch.cuda.Event()] if self.is_cuda else [None, None]
            self.pin_used = [False, False]
            self.pin_i = 0
        i = self.pin_i = self.pin_i ^ 1          # two staging buffers: the host may run one step ahead
        if self.pin_used[i]:
            self.pin_evt[i].synchronize()        # the H2D copy that last used this pinned buffer has finished
        np.concatenate(parts, out=self.pin_np[i][:total])        # packed straight into pinned memory
        self.ibufs[i][:total].copy_(self.pin[i][:total], non_blocking=True)
        if self.is_cuda:
            self.pin_evt[i].record(torch.cuda.current_stream(self.dev))
            self.pin_used[i] = True
        base = self.ibufs[i].data_ptr()
        bt = Batch()
        bt.B, bt.T, bt.K = B, T, K
        o = 0
        bt.seq = base
        o += rows
        for k in range(5):
            bt.pub[k] = base + 4 * o
            o += rows
        bt.gap = base + 4 * o
        o += rows
        bt.cw = base + 4 * o
        o += B
        bt.ch = base + 4 * o
        o += B
        bt.label = base + 4 * o
        o += B
        bt.neg = (base + 4 * o) if K else None
        o += B * K
        if ragged:                               # off [B + 1] | pos [R] ride behind the feed in the same buffer
            rg = Ragged()
            rg.R, rg.off, rg.pos = rows, base + 4 * o, base + 4 * (o + B + 1)
            bt._rg, bt._len = rg, parts[-2][1:] - parts[-2][:-1]
        bt._seq_t = self.ibufs[i][:rows]            # tensor view of `seq` (ids of the sparse-row exchange)
        bt._keep = self.ibufs[i]
        return bt

    @staticmethod
    def is_ragged(batch) -> bool:
        """is this feed a ragged one (flat rows + "len")?"""
        return isinstance(batch, dict) and "len" in batch

    @staticmethod
    def _sessions(batch) -> int:
        """the number of sessions of a feed, rectangular or ragged"""
        return int(np.asarray(batch["len"]).shape[0]) if "len" in batch else int(np.asarray(batch["seq"]).shape[0])

    @staticmethod
    def _rows(bt: Batch) -> int:
        """session rows of an uploaded batch: R of a ragged one, B * T else"""
        rg = getattr(bt, "_rg", None)
        return int(rg.R) if rg is not None else bt.B * bt.T

    def _ragged_parts(self, batch):
        """A ragged feed, validated before anything is uploaded -> (the int32 arrays of the packed buffer — the feed's own, then
        off [B + 1] and pos [R] —, B, the longest length, R).  "label" is optional (zeros)."""
        ln = np.asarray(batch["len"])
        if ln.ndim != 1 or ln.size == 0 or not np.issubdtype(ln.dtype, np.integer):
            raise ValueError("len must be an integer array [B] of at least one session")
        if "neg" in batch and batch["neg"] is not None and np.asarray(batch["neg"]).size:
            raise ValueError("a ragged feed carries no negatives (training stays rectangular)")
        if int(ln.min()) < 1 or int(ln.max()) > 40:
            raise IndexError("session length outside [1, 40], the 40-row position table (model_combine.py:57)")
        B, R = int(ln.size), int(ln.sum())
        seq = np.ascontiguousarray(batch["seq"], dtype=np.int32).reshape(-1)
        if seq.size != R:
            raise ValueError("sum(len) = %d, but seq holds %d rows" % (R, seq.size))
        if seq.min() < 1 or seq.max() > self.geo.N:
            raise IndexError("item id outside [1, N]")
        parts = [seq]
        for k in ("pm", "pd", "pw", "ph", "pmi", "gap"):
            x = np.asarray(batch[k], dtype=np.int32).reshape(-1)
            if x.size != R:
                raise ValueError("sum(len) = %d, but %s holds %d rows" % (R, k, x.size))
            parts.append(x)
        for k in ("cw", "ch", "label"):
            x = np.zeros(B, dtype=np.int32) if k == "label" and k not in batch else np.asarray(batch[k], dtype=np.int32).reshape(-1)
            if x.size != B:
                raise ValueError("%s must hold one entry per session, B = %d" % (k, B))
            parts.append(x)
        from .host.data import ragged_offsets
        off, pos = ragged_offsets(ln)
        return parts + [off, pos], B, int(ln.max()), R

    # ------------------------------------------------------------------------------ native (C++) step driver
    # second HIP stream for the independent dE / candidate-time chains (C++ driver only).  None: from TCAR_NO_OVERLAP when the engine
    # is constructed; a class or an instance may set True / False
    overlap = None
    native = True        # drive the step from libtcar_hip.so (tcar_train_step / tcar_eval_step); False = Python (oplevel.py)
    slot_item = SLOT["item_emb"]
    _ctx_key = None      # what the cached tcar_ctx_t was built for; None forces a rebuild (set_tuning; bench.py after changing _ev)

    def _form(self) -> StepForm:
        """switches + geometry + scoring mode -> the form of this engine's step (nothing else derives it).  The one-hot forms need the
        whole catalog on this engine; the forward one does not need the backward one (ldt != 64)."""
        sw, g, bf, ov = self.sw, self.geo, bool(self.scoring_code), bool(self.overlap)
        ce = bf and self.scoring_bwd == 1
        oh = ce and self.shard == (0, g.N) and not sw.no_onehot
        ohb = oh and g.ldt == 64 and not sw.no_onehot_bwd
        wks = max(1, int((self.tune if self.tune is not None else _lib.tuning()).wgrad_ks))
        return StepForm(ScoreForm(planes=bf, fused_ce=ce, onehot_fwd=oh, onehot_bwd=ohb, anchored=ohb and not sw.no_ce_anchor),
                        det_colsums=bf and not sw.atomic_colsums, wgrad_ks=wks if self.work_rows > wks and not sw.atomic_wgrad else 0,
                        sorted_rows=ov, stream3=ov and not sw.no_stream3,
                        flag_forks=ov and self.flag_forks and not sw.no_flag_fork, fold_scratch=not sw.no_fold_scratch)

    def _optional_specs(self, f: StepForm) -> List[Spec]:
        """the optional workspaces of tcar_ctx_t outside the scoring family (sizes: the comments of their fields in include/tcar_hip.h)"""
        g, r, B, out = self.geo, self.work_rows, self.work_B, []
        u = lambda k: (k + 127) // 128
        if f.wgrad_ks:            # wgrad_slabs: one slab of the nine weight gradients per K split, at most 16
            per = g.ic * g.ic + g.pt * g.pt + g.ldh * g.ic + g.ct * g.ldh + g.ic * g.ldh + 2 * g.ldh * g.ldh + g.ldt * g.ldh + g.pt * g.ldh
            out.append(Spec("_wgrad_slabs", (min(16, (r + f.wgrad_ks - 1) // f.wgrad_ks) * per,), F32, None, "wgrad_slabs"))
        if f.score.planes:        # proj_slabs: one slab per 128-deep K chunk of the forward projections; the backward reuses it
            out.append(Spec("_proj_slabs", (max((u(g.ic) + 2 * u(g.ldh) + u(g.ldt) + u(g.pt)) * r * g.ldh, max(u(g.ic), u(g.pt)) * B * g.ek),),
                            F32, None, "proj_slabs"))
        if f.score.anchored:      # ce_form: ONE host int
            out.append(Spec("_ce_form", (1,), HOST_I32, None, "ce_form"))
        if f.sorted_rows:         # segsum_ws: sized for the workspace's largest batch; small_det_ws: fixed
            out += [Spec("_segsum_ws", (int(self.lib.tcar_segsum_ws_bytes(C.byref(self.dims), max(1, r + B * 64))),), U8, None, "segsum_ws"),
                    Spec("_small_det_ws", (int(self.lib.tcar_small_det_ws_floats()),), F32, None, "small_det_ws")]
        if f.fold_scratch:        # fold_scratch: zeroed words of the order-fixed last-arrival fold
            out.append(Spec("_fold_scratch", (128,), I32, 0, "fold_scratch"))
        return out

    def _ctx(self) -> "_lib.Ctx":
        """tcar_ctx_t for the current workspace: rebuilt when a buffer was (re-)allocated (Workspace.version), when the timing state
        or the tuning copy changed, or when _ctx_key was cleared — and only then"""
        if self._ctx_key == (self.ws.version, id(self._ev), id(self.tune)):
            return self._ctx_obj
        c, form = _lib.Ctx(), self._form()
        specs = self.ws.ensure(self._scoring_specs(form.score) + self._optional_specs(form))
        c.d, c.splitk, c.arena_n = self.dims, self.splitk, self.arena_n
        for i, (short, sg) in enumerate(self.seg.items()):
            c.slot_of[i], c.off[i] = sg["slot"], sg["off"]
        c.slot_item = self.slot_item
        c.b1, c.b2, c.eps, c.neg_weight = self.b1, self.b2, self.eps, self.neg_weight
        c.clip = float(self.max_grad) if self.max_grad else 0.0
        c.segs_all, c.segs_dense = self.segs_all, self.segs_dense
        c.scoring, c.scoring_bwd = self.scoring_code, self.scoring_bwd
        for n in CTX_STATE + CTX_WS + ["rank", "topk"] + (["e16h", "e16l"] if self.scoring_code else []):
            setattr(c, n, getattr(self, n).data_ptr())
        self.ws.bind(c, specs, CTX_SIZES)
        if form.det_colsums:
            c.gw_rows = self.gw_rows.data_ptr()
        if form.sorted_rows:
            if not hasattr(self, "_aux"):
                self._aux = torch.cuda.Stream(self.dev)
                self._aux_ev = [torch.cuda.Event() for _ in range(6)]
                for e in self._aux_ev:
                    e.record(torch.cuda.current_stream(self.dev))      # materialise the hipEvent_t handles
            c.stream2 = self._aux.cuda_stream
            for i, e in enumerate(self._aux_ev):
                c.ev[i] = e.cuda_event
        if form.stream3:
            if not hasattr(self, "_aux3"):
                self._aux3 = torch.cuda.Stream(self.dev)
                self._aux3_ev = torch.cuda.Event()
                self._aux3_ev.record(torch.cuda.current_stream(self.dev))
            c.stream3, c.ev3 = self._aux3.cuda_stream, self._aux3_ev.cuda_event
        # flag forks (tcar_ctx_t.sig_dev): a polling kernel must never sit in FRONT of the work it waits for in a hardware queue.
        # Every poll of the step is enqueued BEHIND its producer's launch, and a producer depends only on work enqueued before
        # it — so whatever shares the poll's queue ahead of it (another of our streams, a collective's stream) never waits for
        # the poll: the single-process engine and the catalog-sharded one (whose pieces between the collectives fork and join
        # our own streams only) use them; DPEngine, whose exchange is enqueued in the middle of the fused backward, keeps events
        if form.flag_forks:
            if not hasattr(self, "_sig"):
                self._sig = torch.zeros(80, dtype=torch.int32, device=self.dev)
                # the driver's fork slots and epoch counter: host memory owned by THIS engine (nothing per thread / process)
                self._fork_host = (C.c_uint8 * int(self.lib.tcar_fork_state_bytes()))()
                # time-outs are mirrored into a pinned, device-visible host word: poll_fork_errors() reads it without a sync
                self._sig_err = torch.zeros(16, dtype=torch.int32).pin_memory()
                self._sig_err_np = self._sig_err.numpy()
                # one probe: do the side streams run BESIDE the main stream here?  (Not under a counter-collecting
                # profiler or with serialised kernels: every poll would sit out its time-out — events then.)
                if not self._probe_flag_forks():
                    import warnings
                    warnings.warn("tcar: kernels of different streams do not run concurrently here (profiler counter "
                                  "collection / serialised kernels / shared hardware queue): flag forks off, events instead")
                    self._sig = None
            if self._sig is not None:
                c.sig_dev, c.fork_host = self._sig.data_ptr(), C.cast(self._fork_host, C.c_void_p)
                c.sig_err_host = self._sig_err.data_ptr()
        if self.tune is not None:
            c.tune = C.cast(C.pointer(self.tune), C.c_void_p)
        if self._ev is not None:
            c.ev_start = C.cast(self._ev["start_arr"], C.c_void_p)
            c.ev_stop = C.cast(self._ev["stop_arr"], C.c_void_p)
            c.ev_n = self._ev["n"]
            c.ev_cursor = C.cast(self._ev["cursor"], C.c_void_p)
        self._ctx_key, self._ctx_obj = (self.ws.version, id(self._ev), id(self.tune)), c
        return c

    flag_forks = True    # may this engine class fork / join its streams through device flags (see _ctx)
    # does the engine make a process-wide high-priority stream the current one (use_priority_stream)?  The data-parallel engines
    # switch it off while collectives are live: with RCCL's copies / kernels on a priority stream AND the device sampler forming
    # batches on its normal-priority side stream, the step ran at 1.39 ms instead of 0.74 (round 6, one rank, every collective
    # forced: profiles/r06_ab_experiments.txt section 4)
    priority_stream = True
    _ev = None
    tune = None          # optional _lib.Tuning copy of THIS engine (set_tuning); None = the process-wide switch values

    def set_tuning(self, **overrides):
        """Give this engine its own copy of the TCAR_* switches with `overrides` applied (tests, tools: e.g.
        set_tuning(TCAR_FLAG_FORK=0)); other engines and the process-wide values are untouched."""
        self.flush()
        self.tune = _lib.tuning(**overrides)
        self._ctx_key = None

    TIMED_KERNELS = ("score_fwd", "score_dx", "score_dE", "session_proj", "gather_fwd")      # kinds 0..4 of tcar_ctx_t.ev_start / ev_stop

    def enable_native_timing(self, n: int):
        """HIP events around the three full-catalog GEMMs inside tcar_train_step (logits, dX, dE), each pair recorded on the
        stream its GEMM is launched on (bench.py roofline): n slots per kernel, used round-robin."""
        st = torch.cuda.current_stream(self.dev)
        k = len(self.TIMED_KERNELS)
        starts = [torch.cuda.Event(enable_timing=True) for _ in range(k * n)]
        stops = [torch.cuda.Event(enable_timing=True) for _ in range(k * n)]
        for e in starts + stops:
            e.record(st)                      # materialise the underlying hipEvent_t
        self._ev = {"n": n, "starts": starts, "stops": stops, "cursor": (C.c_int32 * 2)(0, 0),
                    "start_arr": (C.c_void_p * (k * n))(*[e.cuda_event for e in starts]),
                    "stop_arr": (C.c_void_p * (k * n))(*[e.cuda_event for e in stops])}

    def native_timing_ms(self, kind: int = 0):
        """per-launch milliseconds of kernel `kind` (index into TIMED_KERNELS); call after a device synchronize"""
        n = self._ev["n"]
        used = min(self._ev["cursor"][0], n)
        return [self._ev["starts"][kind * n + i].elapsed_time(self._ev["stops"][kind * n + i]) for i in range(used)]

    def step_form(self, bt: Batch) -> Dict[str, bool]:
        """The form a fused training step of `bt` takes on this engine (tcar_step_form: the driver's own predicates) —
        {"fused_ce", "onehot_fwd", "onehot_bwd", "sorted_rows", "ce_anchored"}.  Tools that label measurements ask this instead of
        re-deriving it from the environment."""
        self._ensure_work(bt.B, bt.T)
        out = (C.c_int32 * 5)()
        check(self.lib.tcar_step_form(C.byref(self._ctx()), C.byref(bt), out), "tcar_step_form")
        return {"fused_ce": bool(out[0]), "onehot_fwd": bool(out[1]), "onehot_bwd": bool(out[2]), "sorted_rows": bool(out[3]),
                "ce_anchored": bool(out[4])}

    def _lr_t(self) -> float:
        return float(np.float32(self.lr) * np.sqrt(np.float32(1) - self.b2_pow) / (np.float32(1) - self.b1_pow))

    def _after_update(self):
        self.step += 1
        self.b1_pow = np.float32(self.b1_pow * np.float32(self.b1))
        self.b2_pow = np.float32(self.b2_pow * np.float32(self.b2))
        self._time_dirty = True

    # ------------------------------------------------------------------------------------------ public API
    def _loss_view(self, bt: Batch) -> torch.Tensor:
        """per-session loss of model_combine.py:147 — written by the negative-term kernel.  Without negatives the reference
        still feeds label_neg as [B, 0]: neg_logits = 0 and every session's loss carries the constant
        neg_weight * -log(1 - sigmoid(0)) = neg_weight * ln 2 (no gradient)."""
        if bt.K > 0 and bt.neg:
            return self.loss[:bt.B]
        return self.ce[:bt.B] + float(np.float32(self.neg_weight) * np.float32(np.log(2.0)))

    _pending_lr = None        # bias-corrected rate of an optimizer update that has been deferred (train_step(defer_update=True))

    _update_ctx = _ctx        # the context an optimizer update covers (the sharded engine: its shard's)

    def flush(self):
        """Apply a deferred optimizer update now (no-op otherwise).  Every entry point except train_step(defer_update=True)
        calls it first, so a deferred update is never observable."""
        if self._pending_lr is not None:
            lr, self._pending_lr = self._pending_lr, None
            check(self.lib.tcar_step_update(C.byref(self._update_ctx()), lr, self._stream()), "tcar_step_update")

    def discard_pending_update(self) -> bool:
        """Forget a deferred optimizer update WITHOUT applying it; returns whether one was owed.  The step count and the beta powers
        have already advanced for it, so this is for a caller that replaces the whole state next (load_state) or reads the state in
        front of the owed update (tests)."""
        owed, self._pending_lr = self._pending_lr is not None, None
        return owed

    def _step_deferred(self, enqueue, defer_update: bool):
        """The deferred-update protocol: enqueue(lr) runs one step WITHOUT its optimizer update, applying the owed update of the step
        before (rate lr; None: nothing owed) at its start; this step's update is then owed in turn — to the next step or to flush()."""
        lr_owed, self._pending_lr = self._pending_lr, None
        enqueue(lr_owed)
        self._pending_lr = self._lr_t()
        self._after_update()              # step count / beta powers advance now; the device work is owed
        self.poll_fork_errors()
        if not defer_update:
            self.flush()

    def train_step(self, batch: Dict[str, np.ndarray], bt: Optional[Batch] = None, defer_update: bool = False) -> torch.Tensor:
        """One sess.run([loss, global_step, train_op]) (model_combine.py:231); returns loss[B] on device.
        defer_update=True (training loops): the Adam update of THIS step is applied at the start of the next train_step —
        arena + the item rows that step gathers first, the other item rows on the aux stream beside its forward pass
        (tcar_train_step_deferred) — or by flush(); results are identical, the HBM-bound pass over the item table leaves
        the critical path."""
        self._refuse_ragged(batch, bt, "train_step")
        if self._index_stale:
            self._build_time_index()
        bt = bt or self.upload(batch)
        if self.native:
            self._ensure_work(bt.B, bt.T)
            if defer_update or self._pending_lr is not None:
                self._step_deferred(lambda lr: check(self.lib.tcar_train_step_deferred(
                    C.byref(self._ctx()), C.byref(bt), int(self._time_dirty), int(lr is not None), 0.0 if lr is None else lr,
                    self._stream()), "tcar_train_step_deferred"), defer_update)
            else:
                check(self.lib.tcar_train_step(C.byref(self._ctx()), C.byref(bt), int(self._time_dirty), self._lr_t(),
                                               self._stream()), "tcar_train_step")
                self._after_update()
                self.poll_fork_errors()
        else:
            self.flush()
            self.forward(bt)
            self.backward(bt)
            self.update()
        return self._loss_view(bt)

    def loss_and_grads(self, batch, bt: Optional[Batch] = None) -> torch.Tensor:
        self._refuse_ragged(batch, bt, "loss_and_grads")
        self.flush()
        if self._index_stale:
            self._build_time_index()
        bt = bt or self.upload(batch)
        if self.native:
            self._ensure_work(bt.B, bt.T)
            ctx, st = self._ctx(), self._stream()
            check(self.lib.tcar_step_forward(C.byref(ctx), C.byref(bt), int(self._time_dirty), st), "tcar_step_forward")
            self._time_dirty = False
            check(self.lib.tcar_step_backward_local(C.byref(ctx), C.byref(bt), st), "tcar_step_backward_local")
            check(self.lib.tcar_step_finish(C.byref(ctx), C.byref(bt), st), "tcar_step_finish")
        else:
            self.forward(bt)
            self.backward(bt)
        return self._loss_view(bt)

    # ---- diversity metrics of the evaluation loop on the device (model_combine.py:174-194,301-313)
    def set_categories(self, cat_of_item: np.ndarray):
        """cat_of_item [N]: integer category code of every 0-based item (host/metrics.category_table); also allocates the
        byte map of recommended items behind `coverage()`."""
        cat = np.ascontiguousarray(np.asarray(cat_of_item).reshape(-1), dtype=np.int32)
        if cat.shape[0] != self.geo.N:
            raise ValueError("category table must have one entry per catalog item")
        self._cat = torch.tensor(cat, device=self.dev)
        self._seen = torch.zeros(self.geo.N, dtype=torch.uint8, device=self.dev)

    def reset_coverage(self):
        self._seen.zero_()

    def eval_diversity(self, bt: Batch, topk: torch.Tensor, block=None):
        """getILD / getUnexp pair counts of the sessions of `bt` for their top-k lists (int32 [B] each, on the device) and
        the recommended items marked in the coverage map; divide with host.metrics.diversity_from_counts.
        block = (row0, B, T): the B sessions of one length T whose item rows start at flat row `row0` of a ragged `bt` (the sessions
        of one packed feed, host.data.pack_sessions), `topk` their lists."""
        if block is None and getattr(bt, "_rg", None) is not None:
            raise ValueError("the diversity counts take sessions of one length: name a (row0, B, T) block of the ragged batch")
        row0, B, T = (0, bt.B, bt.T) if block is None else (int(x) for x in block)
        if row0 < 0 or B < 1 or T < 1 or row0 + B * T > self._rows(bt):
            raise ValueError("block = (row0, B, T) must lie inside the batch's rows")
        k = int(topk.shape[1])
        topk = topk[:B].contiguous()
        out = torch.empty(3, B, dtype=torch.int32, device=self.dev)
        p = self._p
        check(self.lib.tcar_eval_diversity(B, T, k, self.geo.N, p(topk), C.c_void_p(bt.seq + 4 * row0), p(self._cat), p(out[0]), p(out[1]),
                                           p(out[2]), C.c_void_p(self._seen.data_ptr()), self._stream()), "tcar_eval_diversity")
        return out[0], out[1], out[2]

    def coverage(self) -> int:
        """number of distinct items recommended since reset_coverage() (len(resultItemDict), model_combine.py:313)"""
        return int(self._seen.sum(dtype=torch.int64).item())

    def eval_step(self, batch, k: int = 20, bt: Optional[Batch] = None, keep_logits: bool = False):
        """sess.run([softmax_input, cross_loss]) (model_combine.py:283) + rank / top-k on device.
        Returns (rank[B] int32, topk[B,k] int32, ce[B] f32[, logits [B,N]])."""
        self._refuse_ragged(batch, bt, "eval_step")
        self.flush()
        bt = bt or self.upload(batch)
        B = bt.B
        self._ensure_work(B, bt.T)
        self.ws.get(Spec("topk", (self.work_B, k), I32))           # (another k: a new buffer, and with it a new context)
        if self.native and not keep_logits:
            check(self.lib.tcar_eval_step(C.byref(self._ctx()), C.byref(bt), int(self._time_dirty), k, self._stream()),
                  "tcar_eval_step")
            self._time_dirty = False
            self.poll_fork_errors()
            return (self.rank[:B], self.topk[:B], self.ce[:B])
        if self.native:
            check(self.lib.tcar_step_forward(C.byref(self._ctx()), C.byref(bt), int(self._time_dirty), self._stream()),
                  "tcar_step_forward")
            self._time_dirty = False
        else:
            self.forward(bt)
        g, lib, st, p = self.geo, self.lib, self._stream(), self._p
        check(lib.tcar_rank_topk(B, g.N, p(self.logits), g.Npad, C.c_void_p(bt.label), k, p(self.rank), p(self.topk), st),
              "tcar_rank_topk")
        logits = self.logits[:B, :g.N].clone() if keep_logits else None
        check(lib.tcar_softmax_ce(B, g.N, p(self.logits), g.Npad, C.c_void_p(bt.label), p(self.ce), st), "tcar_softmax_ce")
        out = (self.rank[:B], self.topk[:B], self.ce[:B])
        return out + (logits,) if keep_logits else out

    # ---- streamed score-and-select (include/tcar_serve.h): evaluation and recommendation without the [B, N] logits
    SERVE_MAX_PANEL = 49152        # columns one fold keeps in registers (tcar_select_panel: SEL_MAX_N of csrc/tcar_common.h)

    def default_panel(self) -> int:
        """Columns per panel when the caller names none: 49,152, the widest a fold takes (at most Npad) — at B = 512, k = 20 the
        fastest of {4096, 8192, 16384, 32768, 49152} at both measured catalog sizes (N = 46,033: 0.306 ms per evaluation step against
        0.322 at 16,384; N = 2^20: 4.13 against 5.02 ms; docs/EXPERIMENTS.md, streamed evaluation).  The panel buffer is then
        work_B x 49,152 floats (96 MiB at B = 512); other batch sizes were not measured."""
        return int(max(128, min(self.SERVE_MAX_PANEL, self.geo.Npad)))

    def set_item_keys(self, keys) -> None:
        """The int32 key of every catalog item ([N], e.g. its publish time in minutes), copied to the device once: what the
        `window=(lo, hi)` of eval_step_streamed / recommend compares (include/tcar_window.h).  None removes it."""
        if keys is None:
            self._item_keys = None
            return
        k = np.asarray(keys)
        if k.shape != (self.geo.N,) or not np.issubdtype(k.dtype, np.integer):
            raise ValueError("item keys: an integer array of length N = %d" % self.geo.N)
        if k.size and (int(k.min()) < -2 ** 31 or int(k.max()) >= 2 ** 31):
            raise ValueError("item keys must fit int32")
        self._item_keys = torch.from_numpy(np.array(k, dtype=np.int32, order="C")).to(self.dev)      # (np.array: a copy the caller cannot write)

    def _window_bounds(self, window, B: int):
        """(lo, hi), each a scalar or an int array [B] -> two int32 host arrays [B]; bounds beyond int32 are clipped to it"""
        try:
            lo, hi = window
            lo, hi = (np.ascontiguousarray(np.broadcast_to(np.clip(np.asarray(x, dtype=np.int64), -2 ** 31, 2 ** 31 - 1), (B,)),
                                           dtype=np.int32) for x in (lo, hi))
        except (TypeError, ValueError):
            raise ValueError("window = (lo, hi), each a scalar or an int array of length B = %d" % B) from None
        return lo, hi

    def _window(self, window, B: int) -> Window:
        """(lo, hi) -> the descriptor of a windowed call"""
        lo, hi = self._window_bounds(window, B)
        # lo and hi are the two rows of ONE workspace entry, so that they go up in one copy (measured: the host-to-device copies are
        # most of what a window costs a small catalog's step, docs/EXPERIMENTS.md)
        self.ws.ensure([Spec("win_lohi", (2, self.work_B), I32)])
        self.win_lohi[:, :B].copy_(torch.from_numpy(np.stack([lo, hi])))
        return self._window_desc(self._item_keys, self.win_lohi)

    @staticmethod
    def _window_desc(keys: torch.Tensor, lohi: torch.Tensor) -> Window:
        """the window descriptor over the item keys [N] and the bounds [2, >= B] (row 0: lo, row 1: hi) on the device"""
        w = Window()
        w.key, w.lo, w.hi = keys.data_ptr(), lohi[0].data_ptr(), lohi[1].data_ptr()
        return w

    @staticmethod
    def _serve_desc(k: int, panel: int, panel_buf: torch.Tensor, state: torch.Tensor, excl: Optional[torch.Tensor] = None, X: int = 0,
                    lab_score: Optional[torch.Tensor] = None, outputs=()) -> Serve:
        """the descriptor of a streamed call over device tensors: the panel buffer, the select state, the exclusion lists
        [>= B, X] (None: none), the label-score workspace and the (topk, score, rank, ce) a whole step writes (a fold alone: none)"""
        s = Serve()
        s.k, s.panel = k, panel
        s.panel_buf, s.state, s.state_bytes = panel_buf.data_ptr(), state.data_ptr(), state.numel() * 4
        if lab_score is not None:
            s.lab_score = lab_score.data_ptr()
        if excl is not None:
            s.excl, s.X = excl.data_ptr(), X
        for f, t in zip(("topk", "score", "rank", "ce"), outputs):
            setattr(s, f, t.data_ptr())
        return s

    def _quota(self, max_per_category) -> Quota:
        """max_per_category -> the descriptor of a capped call (include/tcar_quota.h) over the table of set_categories()"""
        if isinstance(max_per_category, bool) or not isinstance(max_per_category, (int, np.integer)) or max_per_category < 1:
            raise ValueError("max_per_category must be an int >= 1 (None: no cap)")
        if getattr(self, "_cat", None) is None:
            raise ValueError("max_per_category caps the items of one category: call set_categories(cat_of_item) first")
        q = Quota()
        q.cat, q.cap = self._cat.data_ptr(), int(min(max_per_category, 2 ** 31 - 1))
        return q

    def _serve_request(self, k: int, panel: Optional[int], window, max_per_category, width: int):
        """The request of a streamed call, validated before anything is launched -> (k, panel, quota): k, the columns per panel
        (`panel`, None or 0: default_panel()) clipped to `width`, the scored columns rounded up to 128, and the descriptor of
        `max_per_category` (None: no cap).  A `window` needs the item keys."""
        if not 1 <= k <= 64:
            raise ValueError("k must be in [1, 64]")
        quota = self._quota(max_per_category) if max_per_category is not None else None
        return k, self._panel_request(panel, window, width), quota

    def _panel_request(self, panel: Optional[int], window, width: int) -> int:
        """what every panel-streaming call checks of its request -> the columns per panel (`panel`, None or 0: default_panel())
        clipped to `width`.  A `window` needs the item keys."""
        if window is not None and getattr(self, "_item_keys", None) is None:
            raise ValueError("a window compares item keys: call set_item_keys(keys) first")
        panel = self.default_panel() if not panel else int(panel)
        if panel <= 0 or panel % 128 or panel > self.SERVE_MAX_PANEL:
            raise ValueError("panel must be a positive multiple of 128, at most %d" % self.SERVE_MAX_PANEL)
        return min(panel, width)

    def _ensure_fold(self, specs, excl: Optional[torch.Tensor], B: int):
        """the workspace `specs` of a panel-streaming call and, for its exclusion lists (`excl` [B, X] on the device; None: none),
        the entry `excl` [work_B, X] with the lists copied in -> the (excl, X) fields of the call's descriptor"""
        self.ws.ensure(specs + ([Spec("excl", (self.work_B, int(excl.shape[1])), I32)] if excl is not None else []))
        if excl is None:
            return None, 0
        self.excl[:B].copy_(excl)
        return self.excl.data_ptr(), int(excl.shape[1])

    def _serve(self, bt: Batch, k: int, panel: Optional[int], excl: Optional[torch.Tensor], labelled: bool, window=None,
               max_per_category=None):
        """one tcar_serve_step_quota (its window / quota NULL where the request has none); returns (rank, topk, ce, scores) views of
        the workspace (rank / ce only when `labelled`)"""
        g = self.geo
        if self.shard != (0, g.N):
            raise _lib.TcarError("streamed selection needs the whole catalog on this engine (no shard)")
        k, panel, quota = self._serve_request(k, panel, window, max_per_category, g.Npad)
        B = bt.B
        self._ensure_work(B, bt.T, self._rows(bt))
        wb = self.work_B
        state_words = int(self.lib.tcar_select_state_bytes(1, k)) // 4
        specs = [Spec("panel_buf", (wb, panel), F32), Spec("sel_state", (wb, state_words), I32), Spec("lab_score", (wb,), F32),
                 Spec("sel_score", (wb, k), F32), Spec("sel_topk", (wb, k), I32), Spec("sel_rank", (wb,), I32), Spec("sel_ce", (wb,), F32)]
        ex = self._ensure_fold(specs, excl, B)
        s = self._serve_desc(k, panel, self.panel_buf, self.sel_state, None, 0, self.lab_score,
                             (self.sel_topk, self.sel_score, self.sel_rank, self.sel_ce))
        s.excl, s.X = ex
        if not labelled:
            bt = self._without_neg(bt, label=False)
        w = self._window(window, B) if window is not None else None
        self._head_step("serve_step_quota", bt, C.byref(s), C.byref(w) if w is not None else None,
                        C.byref(quota) if quota is not None else None)
        return self.sel_rank[:B], self.sel_topk[:B], self.sel_ce[:B], self.sel_score[:B]

    @staticmethod
    def _without_neg(bt: Batch, label: bool = True) -> Batch:
        """a copy of the descriptor without its negatives (label=False: without its labels too)"""
        nb = Batch()
        C.memmove(C.byref(nb), C.byref(bt), C.sizeof(Batch))
        nb.neg, nb.K = None, 0
        if not label:
            nb.label = None
        nb._keep = getattr(bt, "_keep", None)
        for n in ("_rg", "_len", "_seq_t"):          # (a ragged batch stays one)
            if hasattr(bt, n):
                setattr(nb, n, getattr(bt, n))
        return nb

    def _refuse_ragged(self, batch, bt, what: str) -> None:
        """training and the materialised evaluation are rectangular: a ragged feed is refused before anything is uploaded"""
        if self.is_ragged(batch) or getattr(bt, "_rg", None) is not None:
            raise ValueError("%s takes a rectangular feed: ragged batches are for the streamed serving calls (eval_step_streamed, "
                             "recommend, retrieve, recommend_two_stage, score_candidates)" % what)

    def _head_step(self, name: str, bt: Batch, *args) -> None:
        """One serving step on the uploaded batch: tcar_<name>(ctx, bt, refresh_time, *args, stream), or, where `bt` is ragged, its
        twin of include/tcar_ragged.h (`tcar_serve_step_ragged` for serve_step_quota), which takes the descriptor behind bt."""
        rg = getattr(bt, "_rg", None)
        if rg is None:
            fn, head = "tcar_" + name, (C.byref(bt),)
        else:
            fn, head = "tcar_" + {"serve_step_quota": "serve_step"}.get(name, name) + "_ragged", (C.byref(bt), C.byref(rg))
        check(getattr(self.lib, fn)(C.byref(self._ctx()), *head, int(self._time_dirty), *args, self._stream()), fn)
        self._time_dirty = False
        self.poll_fork_errors()

    def eval_step_streamed(self, batch, k: int = 20, bt: Optional[Batch] = None, panel: Optional[int] = None, window=None,
                           max_per_category: Optional[int] = None):
        """eval_step without the [B, N] score matrix: the catalog is scored `panel` columns at a time and folded into a running
        top-k / rank / softmax state per session.  Returns (rank[B] int32, topk[B,k] int32, ce[B] f32) — views of the workspace,
        valid until the next streamed call.  `last_scores` holds the fp32 scores of the lists.
        window = (lo, hi), scalars or int arrays [B]: session b is evaluated inside its POOL — the items with lo[b] <= key < hi[b]
        (set_item_keys) and its label; the list (-1 where the pool holds fewer than k), the rank and the cross entropy are those of
        the pool alone.
        max_per_category = m >= 1: the list holds at most m items of one category of set_categories() (include/tcar_quota.h: the
        walk in list order that takes an item iff fewer than m of its category are taken); rank and ce stay those of the uncapped
        call, bit for bit."""
        self.flush()
        bt = bt or self.upload(batch)
        rank, topk, ce, self.last_scores = self._serve(bt, k, panel, None, True, window, max_per_category)
        return rank, topk, ce

    def _recommend_inputs(self, batch, exclude_seen: bool, exclude):
        """the uploaded sessions of a recommend() call and their exclusion lists [B, X] on the device (None: none)"""
        if "label" not in batch:
            batch = dict(batch, label=np.zeros(self._sessions(batch), dtype=np.int32))
        if "neg" in batch and not self.is_ragged(batch):
            batch = {n: v for n, v in batch.items() if n != "neg"}
        bt = self.upload(batch)
        parts = []
        if exclude_seen and getattr(bt, "_rg", None) is not None:
            # a ragged batch: [B, max len] on the host, -1 behind each session's own items
            ln = bt._len
            own = np.full((bt.B, bt.T), -1, dtype=np.int32)
            own[np.repeat(np.arange(bt.B), ln), np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln, ln)] = \
                np.asarray(batch["seq"], dtype=np.int32).reshape(-1) - 1
            parts.append(torch.from_numpy(own).to(self.dev))
        elif exclude_seen:               # built on the device from the uploaded ids: 1-based, so id 0 (a pad) becomes -1
            parts.append(bt._seq_t.view(bt.B, bt.T) - 1)
        if exclude is not None:
            ex = np.ascontiguousarray(np.asarray(exclude, dtype=np.int32).reshape(bt.B, -1))
            if ex.shape[1]:
                parts.append(torch.from_numpy(ex).to(self.dev))
        return bt, (torch.cat(parts, dim=1).contiguous() if parts else None)

    def recommend(self, batch, k: int = 20, exclude_seen: bool = True, exclude=None, panel: Optional[int] = None, window=None,
                  max_per_category: Optional[int] = None):
        """The k best next items of every session: (topk [B,k] int32, scores [B,k] f32), best first (score, then item id,
        descending); -1 where fewer than k items remain.  `batch` needs no "label" and no "neg".  exclude_seen drops the items of
        the session itself (seq - 1); `exclude` [B, X] names further 0-based ids (-1 = empty slot).  window = (lo, hi), scalars or
        int arrays [B]: only items with lo[b] <= key < hi[b] (set_item_keys) are candidates of session b; exclusions apply on top.
        max_per_category = m >= 1: at most m items of one category of set_categories() in a list (include/tcar_quota.h); excluded
        and out-of-window items consume no quota."""
        self.flush()
        bt, excl = self._recommend_inputs(batch, exclude_seen, exclude)
        _, topk, _, scores = self._serve(bt, k, panel, excl, False, window, max_per_category)
        return topk, scores

    # ---- one list per category from one pass over the catalog (include/tcar_sections.h)
    MAX_SECTIONS = 16              # sections of one call (TCAR_MAX_SECTIONS)

    def _sections_request(self, sections, k, overall, panel: Optional[int], window, width: int):
        """The request of a recommend_sections call, validated before anything is uploaded -> (codes int32 [G], panel)."""
        if getattr(self, "_cat", None) is None:
            raise ValueError("sections are categories: call set_categories(cat_of_item) first")
        try:
            codes = list(sections)
        except TypeError:
            raise ValueError("sections: 1 to %d distinct integer category codes" % self.MAX_SECTIONS) from None
        if not 1 <= len(codes) <= self.MAX_SECTIONS:
            raise ValueError("sections: 1 to %d category codes, not %d" % (self.MAX_SECTIONS, len(codes)))
        if any(isinstance(c, (bool, np.bool_)) or not isinstance(c, (int, np.integer)) for c in codes):
            raise ValueError("section codes must be integers")
        codes = [int(c) for c in codes]
        if min(codes) < -2 ** 31 or max(codes) >= 2 ** 31:
            raise ValueError("section codes must fit int32")
        if len(set(codes)) != len(codes):
            raise ValueError("section codes must be pairwise distinct")
        for name, v in (("k", k), ("overall", overall)):
            if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= 64):
                raise ValueError("%s must be an int in [1, 64]" % name)
        if k is None:
            raise ValueError("k must be an int in [1, 64]")
        return np.asarray(codes, dtype=np.int32), self._panel_request(panel, window, width)

    def recommend_sections(self, batch, sections, k: int = 10, exclude_seen: bool = True, exclude=None, panel: Optional[int] = None,
                           window=None, overall: Optional[int] = None) -> "SectionLists":
        """One list PER CATEGORY from one pass over the catalog: `sections` names G category codes of set_categories(), 1 <= G <= 16,
        pairwise distinct, and list g of a session is the k best items (1 <= k <= 64) of category sections[g] — best first (score, then
        item id, descending), -1 where the category holds fewer than k eligible items.  One session forward, one scoring GEMM per panel
        and one fold for all G lists; each list carries the bits of recommend(k, window=(code, code + 1)) on an engine whose item keys
        are the categories.  exclude_seen, exclude, panel and window (a publish-time window over set_item_keys, on top of the section)
        as recommend() takes them.  overall = k0 (1 .. 64): also the one list over all categories, the bits of recommend(k0) with the
        same window and exclusions, from the same panels (one more fold, no more GEMM).
        Returns SectionLists(topk [B, G, k] int32, scores [B, G, k] f32, overall_topk, overall_scores [B, k0] or None): views of the
        workspace, valid until the next streamed call."""
        g = self.geo
        codes, panel = self._sections_request(sections, k, overall, panel, window, g.Npad)
        if self.shard != (0, g.N):
            raise _lib.TcarError("sectioned selection needs the whole catalog on this engine (no shard)")
        k, G = int(k), len(codes)
        self.flush()
        bt, excl = self._recommend_inputs(batch, exclude_seen, exclude)
        B = bt.B
        self._ensure_work(B, bt.T, self._rows(bt))
        wb = self.work_B
        words = lambda kk: int(self.lib.tcar_select_state_bytes(1, kk)) // 4      # noqa: E731
        specs = [Spec("panel_buf", (wb, panel), F32), Spec("sec_state", (wb, G, words(k)), I32), Spec("sec_topk", (wb, G, k), I32),
                 Spec("sec_score", (wb, G, k), F32)]
        if overall is not None:
            k0 = int(overall)
            specs += [Spec("sel_state", (wb, words(k0)), I32), Spec("sel_topk", (wb, k0), I32), Spec("sel_score", (wb, k0), F32)]
        d = Sections()
        d.excl, d.X = self._ensure_fold(specs, excl, B)
        d.k, d.G, d.cat = k, G, self._cat.data_ptr()
        for i, c in enumerate(codes):
            d.sections[i] = int(c)
        d.panel, d.panel_buf = panel, self.panel_buf.data_ptr()
        d.state, d.state_bytes = self.sec_state.data_ptr(), self.sec_state.numel() * 4
        d.topk, d.score = self.sec_topk.data_ptr(), self.sec_score.data_ptr()
        w = self._window(window, B) if window is not None else None
        if w is not None:
            d.window = C.addressof(w)            # (w and o stay alive until the call has returned)
        o = None
        if overall is not None:
            o = self._serve_desc(k0, panel, self.panel_buf, self.sel_state, outputs=(self.sel_topk, self.sel_score))
            d.overall = C.addressof(o)
        self._head_step("sections_step", self._without_neg(bt, label=False), C.byref(d))
        if o is None:
            return SectionLists(self.sec_topk[:B], self.sec_score[:B], None, None)
        return SectionLists(self.sec_topk[:B], self.sec_score[:B], self.sel_topk[:B], self.sel_score[:B])

    # ---- in-place catalog updates (include/tcar_catalog.h): publish, correct and retire articles in a live engine
    def _catalog_ids(self, ids) -> np.ndarray:
        """the rows a call names, as update_items and warm_start_items take them: an integer array [U], U >= 1, 0-based, each in
        [0, N), pairwise distinct"""
        ids = ids.detach().cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)
        if ids.ndim != 1 or ids.size == 0 or not np.issubdtype(ids.dtype, np.integer):
            raise ValueError("ids must be an integer array [U] of at least one catalog row")
        if int(ids.min()) < 0 or int(ids.max()) >= self.geo.N:
            raise ValueError("ids must lie in [0, N = %d)" % self.geo.N)
        if np.unique(ids).size != ids.size:
            raise ValueError("ids must be pairwise distinct")
        return ids

    def _update_request(self, ids, content, item_rows, mwdhm, keys, categories):
        """The request of an update_items call, validated before anything is uploaded or launched -> (ids int32 [U], then content /
        item_rows float32 [U, H], mwdhm int32 [U, 5], keys / categories int32 [U], each None where the call brings none)."""
        g = self.geo
        ids = self._catalog_ids(ids)
        U = int(ids.size)
        if all(x is None for x in (content, item_rows, mwdhm, keys, categories)):
            raise ValueError("update_items needs at least one of content, item_rows, mwdhm, keys, categories")

        def table(x, what, shape, integer):
            if x is None:
                return None
            x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
            ok = np.issubdtype(x.dtype, np.integer) if integer else (np.issubdtype(x.dtype, np.floating) or np.issubdtype(x.dtype, np.integer))
            if not ok or x.shape != shape:
                raise ValueError("%s must be %s array [%s]" % (what, "an integer" if integer else "a float", ", ".join(str(n) for n in shape)))
            return x
        content, item_rows = table(content, "content", (U, g.H), False), table(item_rows, "item_rows", (U, g.H), False)
        mwdhm, keys = table(mwdhm, "mwdhm", (U, 5), True), table(keys, "keys", (U,), True)
        categories = table(categories, "categories", (U,), True)
        if keys is not None and getattr(self, "_item_keys", None) is None:
            raise ValueError("keys update the item keys: call set_item_keys(keys) first")
        if categories is not None and getattr(self, "_cat", None) is None:
            raise ValueError("categories update the category table: call set_categories(cat_of_item) first")
        for x, what in ((keys, "item keys"), (categories, "categories"), (mwdhm, "mwdhm")):
            if x is not None and (int(x.min()) < -2 ** 31 or int(x.max()) >= 2 ** 31):
                raise ValueError("%s must fit int32" % what)
        f32 = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float32)
        i32 = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.int32)
        return i32(ids), f32(content), f32(item_rows), i32(mwdhm), i32(keys), i32(categories)

    def _catalog_ctx(self) -> "_lib.Ctx":
        """the context of a catalog update: the catalog side alone (tables, planes, publish times, item moments, the arena for the
        five time tables) — no workspace, so a fresh engine can be updated before its first batch"""
        c = _lib.Ctx()
        c.d, c.arena_n, c.scoring = self.dims, self.arena_n, self.scoring_code
        for i, sg in enumerate(self.seg.values()):
            c.off[i] = sg["off"]
        for n in ["E", "W", "Mi", "Vi", "mwdhm"] + (["e16h", "e16l"] if self.scoring_code else []):
            setattr(c, n, getattr(self, n).data_ptr())
        return c

    def _stage_update(self, ids, content, item_rows, mwdhm, keys, categories) -> "_lib.CatalogUpdate":
        """The validated request of a catalog update on the device -> its descriptor (tcar_catalog_update_t), all but the one-hot
        plane: the payload in ONE pinned buffer and ONE copy on the engine's stream; the pinned words are reused, so a call waits for
        the COPY of the update before it, no more.  refresh_time as every engine wants it: publish times given and the time block
        clean — a dirty one is rebuilt whole, from the updated table, by the next call anyway; a clean one stays clean."""
        g = self.geo
        U, ldr = int(ids.size), _ru(g.H, 4)
        # the payload in ONE buffer of 4-byte words, every section on a 16-byte boundary: ids | mwdhm | keys | categories | item | content
        parts, off, words = [("ids", ids), ("mwdhm", mwdhm), ("key", keys), ("cat", categories), ("item", item_rows), ("content", content)], {}, 0
        for name, x in parts:
            if x is not None:
                off[name] = words
                words += _ru(U * ldr if x.dtype == np.float32 else x.size, 4)
        if getattr(self, "_upd_pin", None) is None or self._upd_pin.numel() < words:
            self._upd_pin = torch.empty(max(words, 1 << 12), dtype=torch.int32).pin_memory()
            self._upd_evt = None
        if self._upd_evt is not None:
            self._upd_evt.synchronize()          # the copy that last read the pinned words has finished
        host = self._upd_pin.numpy()
        for name, x in parts:
            if x is None:
                continue
            if x.dtype == np.float32:
                rows = host[off[name]:off[name] + U * ldr].view(np.float32).reshape(U, ldr)
                rows[:, :g.H], rows[:, g.H:] = x, 0.0
            else:
                host[off[name]:off[name] + x.size] = x.reshape(-1)
        self.ws.ensure([Spec("upd_stage", (max(words, 1 << 12),), I32)])
        self.upd_stage[:words].copy_(self._upd_pin[:words], non_blocking=True)
        self._upd_evt = torch.cuda.Event()
        self._upd_evt.record(torch.cuda.current_stream(self.dev))
        at = lambda name: self.upd_stage.data_ptr() + 4 * off[name] if name in off else None
        d = _lib.CatalogUpdate()
        d.U, d.ids = U, at("ids")
        d.item, d.ld_item, d.content, d.ld_content, d.mwdhm = at("item"), ldr, at("content"), ldr, at("mwdhm")
        d.refresh_time = int(mwdhm is not None and not self._time_dirty)
        if keys is not None:
            d.key, d.key_table = at("key"), self._item_keys.data_ptr()
        if categories is not None:
            d.cat, d.cat_table = at("cat"), self._cat.data_ptr()
        d.zero_moments = int(item_rows is not None)
        return d

    def update_items(self, ids, content=None, item_rows=None, mwdhm=None, keys=None, categories=None) -> None:
        """Replace rows of the catalog IN PLACE, between two calls of a live engine: ids int [U], 0-based as in `candidates` /
        `exclude`, each in [0, N), pairwise distinct; then any of content / item_rows float [U, H], mwdhm int [U, 5]
        (publish_time_MWDHM rows), keys int [U] (after set_item_keys), categories int [U] (after set_categories).  One staged copy
        and one tcar_catalog_update on the engine's stream, ordered behind every earlier call and in front of every later one; no
        device synchronisation (the pinned staging words are reused: a call waits for the COPY of the update before it, no more).  Every buffer the engine derives from a row — the fp32 image, the bf16 planes, the clipped time
        block, the one-hot row — then holds the bytes of an engine built from the final tables (include/tcar_catalog.h), and no
        whole-catalog refresh follows: where the time block was clean it stays clean.  item_rows zeroes the Adam moments of those
        rows (a replaced row has no optimizer history).  A changed publish time marks the inverted index of the training step stale;
        it is rebuilt once, in front of the next train_step / loss_and_grads.
        Publishing without growing N: build the engine with spare rows whose key lies above every window's `hi` — they are in no
        pool —, publish an article into one (content, mwdhm, keys = its minute, categories) and retire it by moving the key back."""
        ids, content, item_rows, mwdhm, keys, categories = self._update_request(ids, content, item_rows, mwdhm, keys, categories)
        g = self.geo
        if self.shard != (0, g.N):
            raise _lib.TcarError("update_items needs the whole catalog on this engine (no shard)")
        self.flush()
        d = self._stage_update(ids, content, item_rows, mwdhm, keys, categories)
        if mwdhm is not None and getattr(self, "_oh16", None) is not None:
            d.onehot, d.onehot_inner = self._oh16.data_ptr(), 160
        check(self.lib.tcar_catalog_update(C.byref(self._catalog_ctx()), C.byref(d), self._stream()), "tcar_catalog_update")
        # the host copies follow: load_params / export read the content, the index is rebuilt from the publish times
        if content is not None:
            if not self._content_own:
                self._content, self._content_own = np.array(self._content, dtype=np.float32), True
            self._content[1 + ids] = content
        if mwdhm is not None:
            self._mwdhm_host[ids] = mwdhm
            self._index_stale = True

    # ---- warm start (include/tcar_warm.h): item rows for newly published articles from the rows of their content neighbours
    def _warm_request(self, ids, k, min_sim, exclude, window, panel: Optional[int]):
        """The request of a warm_start_items call, validated before anything is uploaded -> (ids int32 [U], k, min_sim, exclude
        int32 [U, X] or None, (lo, hi) int32 [U] each or None, panel)"""
        ids = self._catalog_ids(ids)
        U = int(ids.size)
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or not 1 <= k <= 64:
            raise ValueError("k must be an int in [1, 64] (the donors of one row)")
        if isinstance(min_sim, (bool, np.bool_)) or not isinstance(min_sim, (int, float, np.integer, np.floating)) \
                or not 0.0 <= float(min_sim) <= 1.0:
            raise ValueError("min_sim must be a real number in [0, 1]")
        excl = None
        if exclude is not None:
            ex = exclude.detach().cpu().numpy() if isinstance(exclude, torch.Tensor) else np.asarray(exclude)
            if ex.ndim != 2 or ex.shape[0] != U or not np.issubdtype(ex.dtype, np.integer):
                raise ValueError("exclude must be an integer array [U, X] with U = %d rows" % U)
            if ex.shape[1]:
                e64 = ex.astype(np.int64)
                excl = np.ascontiguousarray(np.where((e64 < 0) | (e64 >= 2 ** 31), -1, e64), dtype=np.int32)
        panel = self._panel_request(panel, window, self.geo.Npad)
        bounds = self._window_bounds(window, U) if window is not None else None      # (ONE pair of scalars, or one pair per id)
        return np.ascontiguousarray(ids, dtype=np.int32), int(k), float(np.float32(min_sim)), excl, bounds, panel

    def warm_start_items(self, ids, k: int = 16, min_sim: float = 0.0, exclude=None, window=None, panel: Optional[int] = None) -> "WarmStart":
        """Give the COLD rows `ids` (int [U], validated as update_items validates them: 0-based, in [0, N), pairwise distinct) — newly
        published articles, whose item row is an untrained draw or a retired article's — the cosine-weighted mean of the trained
        item rows of their k nearest CONTENT neighbours (the rule of include/tcar_warm.h), computed on the device and installed in
        place; nothing crosses the host.  The neighbour lists are those of similar_items(ids, k, exclude = ids + exclude, window):
        every id of the call is excluded as a donor — cold rows do not donate to each other —, exclude int [U, X] adds more per
        row, and window = (lo, hi), ONE pair of scalars or one pair per id over the keys of set_item_keys, keeps spare and retired
        rows out of the donor pool (they carry keys above every hi).  A neighbour with a cosine <= 0 or below min_sim (in [0, 1])
        donates nothing; a row without donors becomes +0 (support 0), which adds nothing to a logit.
        flush() first, then three calls on the engine's stream, ordered as update_items is; no synchronisation.  Afterwards every
        buffer of the engine holds, for the named rows, the bytes of an engine built from tables whose item rows are `rows`, and
        their Adam moments are zero: the contract of update_items(item_rows=rows).  WarmStart(rows [U, H], support [U], wsum [U],
        donors [U, k], sims [U, k]): views of the workspace on the device, valid until the next streamed call.
        Workspace: besides the [U, panel] panel buffer of similar_items, the exclusion lists are int32 [U, U + X] — every row names
        every id of the call — so they grow with U SQUARED (64 MB at U = 4,096, 1 GB at U = 16,384), and every fold scans a row's
        list once per panel.  Publish a large batch in slices of a few thousand ids, naming the other slices' ids in `exclude` if
        they must not donate either, or keeping them out of the pool by `window`."""
        ids, k, min_sim, excl, bounds, panel = self._warm_request(ids, k, min_sim, exclude, window, panel)
        return self._warm_start(ids, k, min_sim, excl, bounds, panel, zero_moments=True)

    def _warm_start(self, ids: np.ndarray, k: int, min_sim: float, excl, bounds, panel: int, zero_moments: bool) -> "WarmStart":
        """one tcar_warm_step for a validated request; zero_moments False: the Mi / Vi rows keep every byte (test() hides and
        restores rows of a model it is not allowed to change)"""
        g = self.geo
        if self.shard != (0, g.N):
            raise _lib.TcarError("warm_start_items needs the whole catalog on one engine (no shard)")
        self.flush()
        U, X = int(ids.size), int(ids.size) + (int(excl.shape[1]) if excl is not None else 0)
        words = int(self.lib.tcar_select_state_bytes(1, k)) // 4
        self._sm_rows = max(getattr(self, "_sm_rows", 0), U)
        specs = [Spec("panel_buf", (U, panel), F32), Spec("sel_state", (U, words), I32), Spec("sel_topk", (U, k), I32),
                 Spec("sel_score", (U, k), F32), Spec("sm_xq", (U, g.ldh), F32), Spec("sm_rq", (U,), F32), Spec("sm_qid", (U,), I32),
                 Spec("excl", (U, X), I32), Spec("warm_rows", (U, _ru(g.H, 4)), F32), Spec("warm_support", (U,), I32),
                 Spec("warm_wsum", (U,), F32)]
        if bounds is not None:
            specs.append(Spec("sm_lohi", (2, self._sm_rows), I32))
        self.ws.ensure(specs)
        self.sm_qid[:U].copy_(torch.from_numpy(ids))
        self.excl[:U, :U] = self.sm_qid[:U][None, :]          # every named id, in every row: built on the device
        if excl is not None:
            self.excl[:U, U:].copy_(torch.from_numpy(excl))
        s = self._serve_desc(k, panel, self.panel_buf, self.sel_state, self.excl, X, outputs=(self.sel_topk, self.sel_score))
        win = None
        if bounds is not None:
            self.sm_lohi[:, :U].copy_(torch.from_numpy(np.stack(bounds)))
            win = self._window_desc(self._item_keys, self.sm_lohi)
        self.sel_score[:U].zero_()             # (the finish leaves the score of an empty place untouched: it reads 0)
        d = _lib.Warm()
        d.U, d.ids, d.min_sim = U, self.sm_qid.data_ptr(), min_sim
        d.xq, d.rq, d.serve, d.window = self.sm_xq.data_ptr(), self.sm_rq.data_ptr(), C.addressof(s), C.addressof(win) if win is not None else None
        d.rows, d.ld_rows = self.warm_rows.data_ptr(), _ru(g.H, 4)
        d.support, d.wsum, d.zero_moments = self.warm_support.data_ptr(), self.warm_wsum.data_ptr(), int(zero_moments)
        check(self.lib.tcar_warm_step(C.byref(self._catalog_ctx()), C.byref(d), self._stream()), "tcar_warm_step")
        return WarmStart(self.warm_rows[:U, :g.H], self.warm_support[:U], self.warm_wsum[:U], self.sel_topk[:U], self.sel_score[:U])

    def _hide_item_rows(self, ids: np.ndarray, rows: Optional[torch.Tensor] = None):
        """test(): write `rows` (device f32 [U, ldh]; None: zeros) over the item rows `ids` WITHOUT touching their Adam moments and
        return what _restore_item_rows takes to put the old rows back — (ids, the old rows), both on the device.  One gather and
        one tcar_catalog_update on the engine's stream; the planes follow, so a restore leaves every buffer as it was, byte for byte."""
        g = self.geo
        if self.shard != (0, g.N):
            raise _lib.TcarError("hiding item rows needs the whole catalog on one engine (no shard)")
        self.flush()
        ids_dev = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).to(self.dev)
        saved = self.E[ids_dev.long(), :g.ldh].contiguous()
        self._restore_item_rows((ids_dev, torch.zeros_like(saved) if rows is None else rows))
        return ids_dev, saved

    def _restore_item_rows(self, token) -> None:
        ids_dev, rows = token
        d = _lib.CatalogUpdate()
        d.U, d.ids, d.item, d.ld_item, d.zero_moments = int(ids_dev.numel()), ids_dev.data_ptr(), rows.data_ptr(), int(rows.stride(0)), 0
        check(self.lib.tcar_catalog_update(C.byref(self._catalog_ctx()), C.byref(d), self._stream()), "tcar_catalog_update")

    # ---- candidate-list scoring (include/tcar_cand.h): only the rows a session names are read
    CAND_MAX_C = 1024             # slots of one list (CAND_MAX_C of csrc/tcar_common.h)

    @staticmethod
    def _cand_request(B: int, candidates, clicked):
        """The request of a score_candidates call, validated before anything is launched -> (cand, clicked): contiguous int32 host
        arrays [B, C] (clicked: None when the call has none)."""
        def ints(x, what):
            x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
            if not np.issubdtype(x.dtype, np.integer):
                raise ValueError("%s must be an integer array" % what)
            return x
        cand = ints(candidates, "candidates")
        if cand.ndim != 2 or cand.shape[0] != B:
            raise ValueError("candidates must be [B, C] with B = %d sessions" % B)
        if not 1 <= cand.shape[1] <= TcarEngine.CAND_MAX_C:
            raise ValueError("C must be in [1, %d]" % TcarEngine.CAND_MAX_C)
        # (ids beyond int32 cannot be catalog items: they become empty slots like every id outside [0, N))
        c64 = cand.astype(np.int64)
        cand = np.ascontiguousarray(np.where((c64 < 0) | (c64 >= 2 ** 31), -1, c64), dtype=np.int32)
        if clicked is not None:
            clicked = ints(clicked, "clicked")
            if clicked.shape != cand.shape:
                raise ValueError("clicked must have the shape of candidates, [%d, %d]" % cand.shape)
            clicked = np.ascontiguousarray(clicked != 0, dtype=np.int32)
        return cand, clicked

    def score_candidates(self, batch, candidates, clicked=None, bt: Optional[Batch] = None) -> "CandResult":
        """Score and rank the C items every session names: candidates int [B, C], 0-based ids, -1 (any id outside the catalog) = an
        empty slot, repeats allowed.  One tcar_cand_step: the session forward, then B C gathered dots — no [B, N] matrix, no panel;
        `batch` needs no "label" and no "neg".  Returns CandResult(scores [B, C] f32 (-inf in empty slots), rank_of [B, C] int32
        (1-based, 0 = empty), order [B, C] int32 (slots best first, -1 behind the last), counts, metrics): views of the workspace,
        valid until the next call.  List order: score, then item id, descending, then slot ascending.  With clicked int [B, C]
        (0 / 1): counts [B, 3] int32 = (npos, nneg, auc2) and metrics [B, 3] f32 = (mrr, ndcg5, ndcg10) over each list's non-empty
        slots (host.metrics.impression_metrics divides); without: None."""
        if self.shard != (0, self.geo.N):
            raise _lib.TcarError("candidate scoring needs the whole catalog on one engine (no shard)")
        if bt is None:
            if "label" not in batch:
                batch = dict(batch, label=np.zeros(self._sessions(batch), dtype=np.int32))
            if not self.is_ragged(batch):
                batch = {n: v for n, v in batch.items() if n != "neg"}
        B = bt.B if bt is not None else self._sessions(batch)
        cand, clk = self._cand_request(B, candidates, clicked)
        self.flush()
        bt = self._without_neg(bt if bt is not None else self.upload(batch), label=False)
        C_ = cand.shape[1]
        self._ensure_work(B, bt.T, self._rows(bt))
        wb = self.work_B
        # cand and clicked are the two planes of ONE workspace entry: they go up in one copy
        self.ws.ensure([Spec("cand_in", (2, wb, C_), I32), Spec("cand_score", (wb, C_), F32), Spec("cand_rank", (2, wb, C_), I32),
                        Spec("cand_counts", (wb, 3), I32), Spec("cand_metrics", (wb, 3), F32)])
        if clk is None:
            self.cand_in[0, :B].copy_(torch.from_numpy(cand))
        else:
            self.cand_in[:, :B].copy_(torch.from_numpy(np.stack([cand, clk])))
        d = Cand()
        d.C, d.cand, d.ld_cand = C_, self.cand_in[0].data_ptr(), C_
        d.score, d.rank_of, d.order = self.cand_score.data_ptr(), self.cand_rank[0].data_ptr(), self.cand_rank[1].data_ptr()
        if clk is not None:
            d.clicked, d.counts, d.metrics = self.cand_in[1].data_ptr(), self.cand_counts.data_ptr(), self.cand_metrics.data_ptr()
        self._head_step("cand_step", bt, C.byref(d))
        return CandResult(self.cand_score[:B], self.cand_rank[0, :B], self.cand_rank[1, :B],
                          self.cand_counts[:B] if clk is not None else None, self.cand_metrics[:B] if clk is not None else None)

    # ---- retrieval and the two-stage call (include/tcar_retrieve.h): a shortlist of up to 1,024 items from coarse scores
    RETRIEVE_MAX_C = 1024          # entries of one shortlist (a candidate list of tcar_cand.h: CAND_MAX_C)

    def _retrieve_request(self, C_: int, k: Optional[int], panel: Optional[int], window, width: int) -> int:
        """The request of retrieve (k None) / recommend_two_stage, validated before anything is launched -> the columns per panel
        (`panel`, None or 0: default_panel()) clipped to `width`."""
        if isinstance(C_, bool) or not isinstance(C_, (int, np.integer)) or not 1 <= C_ <= self.RETRIEVE_MAX_C:
            raise ValueError("the shortlist must hold 1 to %d items" % self.RETRIEVE_MAX_C)
        if k is not None:
            if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= 64:
                raise ValueError("k must be in [1, 64]")
            if k > C_:
                raise ValueError("k = %d items cannot come out of a shortlist of %d" % (k, C_))
        return self._panel_request(panel, window, width)

    @staticmethod
    def _diversity_request(diversity) -> float:
        """The penalty of a diversified call (include/tcar_mmr.h), validated before anything is uploaded: a finite number >= 0 that is
        finite as fp32 too."""
        if isinstance(diversity, (bool, np.bool_)) or not isinstance(diversity, (int, float, np.integer, np.floating)):
            raise ValueError("diversity must be a number >= 0 (the penalty mu of include/tcar_mmr.h, in score units), or None")
        mu = float(diversity)
        if not 0.0 <= mu <= float(np.finfo(np.float32).max):
            raise ValueError("diversity must be finite and >= 0, not %r" % (diversity,))
        return mu

    def _retrieve(self, batch, C_: int, k: Optional[int], exclude_seen: bool, exclude, panel: Optional[int], window, diversity=None):
        """one tcar_retrieve_step (k None), tcar_retrieve_rerank_step or, with a penalty, tcar_mmr_rerank_step; returns views of the
        workspace"""
        g = self.geo
        if self.shard != (0, g.N):
            raise _lib.TcarError("retrieval needs the whole catalog on this engine (no shard)")
        panel = self._retrieve_request(C_, k, panel, window, g.Npad)
        mu = self._diversity_request(diversity) if diversity is not None else None
        C_ = int(C_)
        self.flush()
        bt, excl = self._recommend_inputs(batch, exclude_seen, exclude)
        B = bt.B
        self._ensure_work(B, bt.T, self._rows(bt))
        wb = self.work_B
        state_words = int(self.lib.tcar_retrieve_state_bytes(1, C_)) // 4
        specs = [Spec("panel_buf", (wb, panel), F32), Spec("rt_state", (wb, state_words), I32), Spec("rt_ids", (wb, C_), I32),
                 Spec("rt_scores", (wb, C_), F32)]
        if k is not None:
            k = int(k)
            specs += [Spec("rt_exact", (wb, C_), F32), Spec("rt_rank", (2, wb, C_), I32), Spec("rt_topk", (wb, k), I32),
                      Spec("rt_topscore", (wb, k), F32)]
            if mu is not None:
                specs.append(Spec("rt_msim", (wb, k), F32))
        d = Retrieve()
        d.excl, d.X = self._ensure_fold(specs, excl, B)
        d.C, d.panel, d.panel_buf = C_, panel, self.panel_buf.data_ptr()
        d.state, d.state_bytes = self.rt_state.data_ptr(), self.rt_state.numel() * 4
        d.ids, d.scores = self.rt_ids.data_ptr(), self.rt_scores.data_ptr()
        w = self._window(window, B) if window is not None else None
        if w is not None:
            d.window = C.addressof(w)            # (w stays alive until the call has returned)
        bt = self._without_neg(bt, label=False)
        if k is None:
            self._head_step("retrieve_step", bt, C.byref(d))
        else:
            r = Rerank()
            r.k, r.cand_score = k, self.rt_exact.data_ptr()
            r.rank_of, r.order = self.rt_rank[0].data_ptr(), self.rt_rank[1].data_ptr()
            r.topk, r.score = self.rt_topk.data_ptr(), self.rt_topscore.data_ptr()
            if mu is None:
                self._head_step("retrieve_rerank_step", bt, C.byref(d), C.byref(r))
            else:
                m = _lib.Mmr()
                m.mu, m.msim = mu, self.rt_msim.data_ptr()
                self._head_step("mmr_rerank_step", bt, C.byref(d), C.byref(r), C.byref(m))
        if k is None:
            return self.rt_ids[:B], self.rt_scores[:B]
        return self.rt_topk[:B], self.rt_topscore[:B]

    def retrieve(self, batch, C: int, exclude_seen: bool = True, exclude=None, panel: Optional[int] = None, window=None):      # noqa: N803
        """A shortlist of the C best next items of every session, 1 <= C <= 1024, from COARSE scores: (ids [B, C] int32,
        coarse_scores [B, C] f32), best first (score, then item id, descending); -1 / -inf where fewer than C items are eligible —
        the empty slot of score_candidates, so `ids` is a valid candidate list.  On a split-bf16 engine the coarse scores contract the
        hi planes alone (a third of the MFMA work, half of the plane bytes, about 2^-8 relative per operand); the fp32 engine has no
        cheaper operands and retrieves from its own scores.  exclude_seen, exclude and window as recommend() takes them.  Views of
        the workspace, valid until the next call."""
        return self._retrieve(batch, C, None, exclude_seen, exclude, panel, window)

    def recommend_two_stage(self, batch, k: int = 20, shortlist: int = 256, exclude_seen: bool = True, exclude=None,
                            panel: Optional[int] = None, window=None, diversity: Optional[float] = None):
        """recommend() in two stages with one session forward: retrieve(batch, shortlist) from coarse scores, then the exact scores
        of the shortlist (score_candidates' kernel, the engine's own scoring precision) and its k best: (topk [B,k] int32, scores
        [B,k] f32), best first; -1 where fewer than k items are eligible.  The list is the top k of the exact scores OVER THE
        SHORTLIST: an item the coarse scores rank below `shortlist` cannot enter it.  k <= 64 and k <= shortlist <= 1024.  Views of
        the workspace, valid until the next call; the shortlist itself is in `rt_ids` / `rt_scores`.
        diversity = mu >= 0 (finite): the k items are taken by the greedy MMR walk of include/tcar_mmr.h over the first 256 slots of
        the shortlist's exact order — each pick is the largest s - mu * m, m the largest content cosine to what the list already
        holds, so a verbatim duplicate of a listed item loses mu logits (mu = (1 - lambda) / lambda of the textbook weight).  The
        scores returned are the exact scores of the picks; `rt_msim` [B, k] holds m of every pick, beside `rt_ids` / `rt_exact`.
        mu = 0 gives the bits of the plain call; None IS the plain call, with its launches."""
        return self._retrieve(batch, shortlist, k, exclude_seen, exclude, panel, window, diversity)

    def diversify(self, candidates, scores, k: int = 20, diversity: float = 1.0):
        """The MMR walk of recommend_two_stage(diversity=...) for lists the caller already holds, e.g. what score_candidates returned:
        candidates int [B, C] (0-based ids; -1 or any id outside the catalog: an empty slot; repeats allowed), scores float [B, C],
        host arrays or tensors, 1 <= C <= 1024, 1 <= k <= 64, k <= C.  tcar_cand_rank, then tcar_mmr_walk over the engine's content
        table: no session forward.  Returns (topk [B, k] int32 (-1 once the pool is used up), scores [B, k] f32 (the given score of
        each pick), msim [B, k] f32 (m of each pick)); slots behind the last pick hold -1 / 0 / 0.  Views of the workspace, valid
        until the next call."""
        g = self.geo
        if self.shard != (0, g.N):
            raise _lib.TcarError("diversify needs the whole catalog on this engine (no shard)")
        mu = self._diversity_request(diversity)
        cand = candidates if isinstance(candidates, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(candidates))
        sc = scores if isinstance(scores, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(scores))
        if cand.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8) or cand.dim() != 2:
            raise ValueError("candidates must be an integer array [B, C]")
        if not sc.dtype.is_floating_point or tuple(sc.shape) != tuple(cand.shape):
            raise ValueError("scores must be a float array of the shape of candidates")
        B, C_ = int(cand.shape[0]), int(cand.shape[1])
        if not 1 <= C_ <= self.CAND_MAX_C:
            raise ValueError("C must be in [1, %d]" % self.CAND_MAX_C)
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= 64 or k > C_:
            raise ValueError("k must be in [1, 64] and <= C = %d" % C_)
        k = int(k)
        self.flush()
        rows = max(B, 1)
        self.ws.ensure([Spec("dv_cand", (rows, C_), I32), Spec("dv_score", (rows, C_), F32), Spec("dv_rank", (2, rows, C_), I32),
                        Spec("dv_topk", (rows, k), I32), Spec("dv_topscore", (rows, k), F32), Spec("dv_msim", (rows, k), F32)])
        c64 = cand.to(self.dev).to(torch.int64)
        self.dv_cand[:B].copy_(torch.where((c64 < 0) | (c64 >= g.N), torch.full_like(c64, -1), c64))
        self.dv_score[:B].copy_(sc.to(self.dev))
        self.dv_topscore[:B].zero_()
        self.dv_msim[:B].zero_()
        p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
        check(self.lib.tcar_cand_rank(B, C_, p(self.dv_score), C_, p(self.dv_cand), C_, None, 0, p(self.dv_rank[0]), p(self.dv_rank[1]),
                                      None, None, self._stream()), "tcar_cand_rank")
        check(self.lib.tcar_mmr_walk(B, C_, k, mu, g.N, g.H, C.c_void_p(self.E.data_ptr() + 4 * g.ldh), g.ek, p(self.dv_cand), C_,
                                     p(self.dv_score), C_, p(self.dv_rank[1]), p(self.dv_topk), p(self.dv_topscore), p(self.dv_msim),
                                     self._stream()), "tcar_mmr_walk")
        return self.dv_topk[:B], self.dv_topscore[:B], self.dv_msim[:B]

    # ---- related items by content cosine (include/tcar_similar.h): no session, no model — the content table under the panel folds
    def _similar_request(self, ids, k, content, exclude_self, exclude, panel: Optional[int], window, max_per_category):
        """The request of a similar_items call, validated before anything is uploaded -> (Q, qid int32 [Q] or None, rows f32 [Q, H]
        or None, excl int32 [Q, X] or None, (lo, hi) or None, quota or None, panel).  An id outside [0, N) becomes -1, the empty
        query."""
        g = self.geo
        if (ids is None) == (content is None):
            raise ValueError("similar_items takes exactly one of ids (catalog rows) and content (rows that are in no catalog)")
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= 64:
            raise ValueError("k must be an int in [1, 64]")
        qid = rows = None
        if ids is not None:
            a = ids.detach().cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)
            if a.ndim != 1 or a.size < 1 or not np.issubdtype(a.dtype, np.integer) or a.dtype == np.bool_:
                raise ValueError("ids must be an integer array [Q], Q >= 1 (0-based catalog rows; -1: an empty query)")
            a64 = a.astype(np.int64)
            qid = np.ascontiguousarray(np.where((a64 < 0) | (a64 >= g.N), -1, a64), dtype=np.int32)
        else:
            a = content.detach().cpu().numpy() if isinstance(content, torch.Tensor) else np.asarray(content)
            if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] != g.H or not np.issubdtype(a.dtype, np.floating):
                raise ValueError("content must be a float array [Q, H = %d], Q >= 1" % g.H)
            rows = np.ascontiguousarray(a, dtype=np.float32)
        Q = int(a.shape[0])
        if not isinstance(exclude_self, (bool, np.bool_)):
            raise ValueError("exclude_self must be True or False")
        parts = [qid[:, None]] if qid is not None and exclude_self else []
        if exclude is not None:
            ex = exclude.detach().cpu().numpy() if isinstance(exclude, torch.Tensor) else np.asarray(exclude)
            if ex.ndim != 2 or ex.shape[0] != Q or not np.issubdtype(ex.dtype, np.integer):
                raise ValueError("exclude must be an integer array [Q, X] with Q = %d queries" % Q)
            e64 = ex.astype(np.int64)
            if ex.shape[1]:
                parts.append(np.where((e64 < 0) | (e64 >= 2 ** 31), -1, e64).astype(np.int32))
        excl = np.ascontiguousarray(np.concatenate(parts, axis=1)) if parts else None
        quota = self._quota(max_per_category) if max_per_category is not None else None
        panel = self._panel_request(panel, window, g.Npad)
        bounds = self._window_bounds(window, Q) if window is not None else None
        return Q, qid, rows, excl, bounds, quota, panel

    def similar_items(self, ids=None, k: int = 20, content=None, exclude_self: bool = True, exclude=None, panel: Optional[int] = None,
                      window=None, max_per_category: Optional[int] = None):
        """The k catalog items whose CONTENT is most similar to each of Q query rows: (topk [Q, k] int32, sims [Q, k] f32), best
        first (cosine, then item id, descending); -1 (and a sim of 0) where fewer than k items are eligible.  The cosine is the
        `sim` of include/tcar_mmr.h over the frozen fp32 content columns, bit for bit what diversify() / `rt_msim` report for the
        same pair.  Exactly one of `ids` (int [Q], 0-based catalog rows; an id outside the catalog, e.g. -1, is an empty query and
        lists -1) and `content` (float [Q, H]: drafts that are in no catalog).  exclude_self (ids only) keeps a query out of its
        own list; exclude [Q, X], window = (lo, hi) per query, max_per_category and panel as recommend() takes them.  No session
        forward and no [Q, N] matrix: one cosine panel and one fold per `panel` columns (include/tcar_similar.h), ordered on the
        engine's stream behind every earlier update_items.  Views of the workspace, valid until the next streamed call."""
        Q, qid, rows, excl, bounds, quota, panel = self._similar_request(ids, k, content, exclude_self, exclude, panel, window,
                                                                         max_per_category)
        g = self.geo
        if self.shard != (0, g.N):
            raise _lib.TcarError("similar_items needs the whole catalog on this engine (no shard)")
        k = int(k)
        self.flush()
        words = int(self.lib.tcar_select_state_bytes(1, k)) // 4
        self._sm_rows = max(getattr(self, "_sm_rows", 0), Q)
        specs = [Spec("panel_buf", (Q, panel), F32), Spec("sel_state", (Q, words), I32), Spec("sel_topk", (Q, k), I32),
                 Spec("sel_score", (Q, k), F32), Spec("sm_xq", (Q, g.ldh), F32), Spec("sm_rq", (Q,), F32)]
        specs.append(Spec("sm_qid", (Q,), I32) if qid is not None else Spec("sm_qrow", (Q, g.H), F32))
        if excl is not None:
            specs.append(Spec("excl", (Q, int(excl.shape[1])), I32))
        if bounds is not None:
            specs.append(Spec("sm_lohi", (2, self._sm_rows), I32))
        self.ws.ensure(specs)
        d = _lib.Similar()
        d.xq, d.rq = self.sm_xq.data_ptr(), self.sm_rq.data_ptr()
        if qid is not None:
            self.sm_qid[:Q].copy_(torch.from_numpy(qid))
            d.qid = self.sm_qid.data_ptr()
        else:
            self.sm_qrow[:Q].copy_(torch.from_numpy(rows))
            d.qrow, d.ld_qrow = self.sm_qrow.data_ptr(), g.H
        s = self._serve_desc(k, panel, self.panel_buf, self.sel_state, outputs=(self.sel_topk, self.sel_score))
        if excl is not None:
            self.excl[:Q].copy_(torch.from_numpy(excl))
            s.excl, s.X = self.excl.data_ptr(), int(excl.shape[1])
        w = None
        if bounds is not None:
            self.sm_lohi[:, :Q].copy_(torch.from_numpy(np.stack(bounds)))
            w = self._window_desc(self._item_keys, self.sm_lohi)
        self.sel_score[:Q].zero_()             # (the finish leaves the score of an empty place untouched: it reads 0)
        check(self.lib.tcar_similar_step(C.byref(self._catalog_ctx()), Q, C.byref(d), C.byref(s), C.byref(w) if w is not None else None,
                                         C.byref(quota) if quota is not None else None, self._stream()), "tcar_similar_step")
        if qid is not None and (qid < 0).any():    # an empty query lists nothing (the kernels scored a zero row)
            gone = torch.from_numpy(np.flatnonzero(qid < 0)).to(self.dev)
            self.sel_topk[gone] = -1
            self.sel_score[gone] = 0.0
        return self.sel_topk[:Q], self.sel_score[:Q]

    # ---- the duplicate audit (include/tcar_dupes.h): every pair of content rows once, three numbers per item
    DUP_LAUNCH_TILES = 2 ** 18        # tiles of 64 x 64 pairs in one launch at the default stripe (a choice: every launch stays short)

    def _dupes_request(self, threshold, window, stripe):
        """The request of a find_duplicates call, validated before anything is uploaded -> (t, (lo, hi) or None, stripe)"""
        if isinstance(threshold, (bool, np.bool_)) or not isinstance(threshold, (int, float, np.integer, np.floating)) \
                or not 0.0 < float(np.float32(threshold)) <= 1.0:
            raise ValueError("threshold must be a real number in (0, 1]")
        bounds = None
        if window is not None:
            if getattr(self, "_item_keys", None) is None:
                raise ValueError("a window compares item keys: call set_item_keys(keys) first")
            try:
                lo, hi = (np.asarray(x) for x in window)
                if lo.ndim or hi.ndim or not (np.issubdtype(lo.dtype, np.integer) and np.issubdtype(hi.dtype, np.integer)):
                    raise TypeError
            except (TypeError, ValueError):
                raise ValueError("window = (lo, hi): ONE pair of integer scalars, the members are the items with lo <= key < hi") from None
            bounds = tuple(int(min(max(int(x), -2 ** 31), 2 ** 31 - 1)) for x in (lo, hi))
        blocks = (self.geo.N + 63) // 64
        if stripe is None:
            stripe = max(1, self.DUP_LAUNCH_TILES // blocks)
        elif isinstance(stripe, (bool, np.bool_)) or not isinstance(stripe, (int, np.integer)) or stripe < 1:
            raise ValueError("stripe must be an int >= 1 (row blocks of 64 items per launch; None: the default)")
        return float(np.float32(threshold)), bounds, int(min(stripe, blocks))

    def find_duplicates(self, threshold: float = 0.98, window=None, stripe: Optional[int] = None) -> "DuplicateAudit":
        """Which articles of the catalog are copies of each other?  For every item i, over the `sim` of similar_items (the content
        cosine of include/tcar_mmr.h, bit for bit): count[i] = the number of OTHER items j with sim(i, j) >= threshold, partner[i] =
        the most similar of them (cosine, then item id, descending; -1 where there is none) and sim[i] = sim(i, partner[i]) (0
        there).  DuplicateAudit(count int32 [N], partner int32 [N], sim f32 [N]): device views, valid until the next
        find_duplicates.  window = (lo, hi), ONE pair of scalars over the keys of set_item_keys: only the items with lo <= key < hi
        are audited, against each other (the others count 0).  One triangular pass over all pairs (include/tcar_dupes.h): no
        matrix, no pair list, nothing that can overflow; the result is the same bits on every run and for every `stripe` (row
        blocks of 64 items per launch; default: the most for which a launch holds at most 2^18 tiles).  Ordered on the engine's
        stream behind every earlier update_items; no host synchronisation.  similar_items(flagged ids) lists ALL partners of a
        flagged row."""
        t, bounds, stripe = self._dupes_request(threshold, window, stripe)
        g = self.geo
        if self.shard != (0, g.N):
            raise _lib.TcarError("find_duplicates needs the whole catalog on this engine (no shard)")
        self.flush()
        self.ws.ensure([Spec("dup_r", (g.N,), F32), Spec("dup_count", (g.N,), I32), Spec("dup_best", (g.N,), torch.int64),
                        Spec("dup_partner", (g.N,), I32), Spec("dup_sim", (g.N,), F32)])
        d = _lib.Dupes()
        d.t, d.stripe = t, stripe
        if bounds is not None:
            d.key, d.lo, d.hi = self._item_keys.data_ptr(), bounds[0], bounds[1]
        d.r, d.count, d.best = self.dup_r.data_ptr(), self.dup_count.data_ptr(), self.dup_best.data_ptr()
        d.partner, d.partner_sim = self.dup_partner.data_ptr(), self.dup_sim.data_ptr()
        check(self.lib.tcar_dupes_step(C.byref(self._catalog_ctx()), C.byref(d), self._stream()), "tcar_dupes_step")
        return DuplicateAudit(self.dup_count[:g.N], self.dup_partner[:g.N], self.dup_sim[:g.N])


class WarmStart(NamedTuple):
    """what TcarEngine.warm_start_items returns: device views, valid until the next streamed call"""
    rows: torch.Tensor                          # f32 [U, H]: the rows that were installed
    support: torch.Tensor                       # int32 [U]: donors with a weight > 0
    wsum: torch.Tensor                          # f32 [U]: the sum of their weights
    donors: torch.Tensor                        # int32 [U, k]: the neighbour lists (-1: an empty place)
    sims: torch.Tensor                          # f32 [U, k]: their cosines


class DuplicateAudit(NamedTuple):
    """what TcarEngine.find_duplicates returns: device views [N], valid until the next find_duplicates"""
    count: torch.Tensor                         # int32: other items at or above the threshold
    partner: torch.Tensor                       # int32: the most similar of them, -1 where there is none
    sim: torch.Tensor                           # f32: its similarity, 0 where there is none


class SectionLists(NamedTuple):
    """what TcarEngine.recommend_sections returns: device views, valid until the next streamed call"""
    topk: torch.Tensor                          # [B, G, k] int32
    scores: torch.Tensor                        # [B, G, k] f32
    overall_topk: Optional[torch.Tensor]        # [B, k0] int32, or None without `overall`
    overall_scores: Optional[torch.Tensor]      # [B, k0] f32


class CandResult(NamedTuple):
    """what TcarEngine.score_candidates returns: device views, valid until the next call"""
    scores: torch.Tensor
    rank_of: torch.Tensor
    order: torch.Tensor
    counts: Optional[torch.Tensor]
    metrics: Optional[torch.Tensor]
