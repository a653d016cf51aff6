"""Data-parallel TCAR step: one process per GPU, torch.distributed (backend "nccl" = RCCL over xGMI on ROCm).

The reference is single-process (no collectives anywhere); this layer is new design.  Examples are
independent given the weights and the loss is a SUM over sessions (model_combine.py:147,156), so the global
gradient is the plain sum of the ranks' gradients — no 1/W rescale — and every rank applies the same clip + Adam
to its replica.  What makes it more than one all-reduce is the clip: tf.clip_by_norm of an IndexedSlices uses the
norm of the concatenated slice VALUES, which is not additive for blocks that are sums over the
whole (global) batch.  The exchange has these steps (`GradExchange`; the collectives 1, 5, 3 are issued in that one
canonical order on every rank and do not depend on each other, the local steps 2, 4, 6 follow once they have landed):

  1. all-reduce  [ dE_item | dE_time ]      [N, ldh + pt] fp32 — the dense item-table block (scoring + densified
                                            negative part) and the candidate-side time block, BEFORE any per-row work
  2. local       ||dE_item||^2              -> dense norm piece of item_emb (now global)
  3. all-reduce  [ arena grads | pieces ]   dense weights, small tables (session-side rows only), per-row norm
                                            pieces (these ARE additive: each gathered row belongs to one rank)
  4. local       candidate-side clip backward of the reduced dE_time -> time-table grads + their norm pieces,
                                            added ONCE after step 3 (adding before would count them W times)
  5. all-gather  (item id, gradient row)    the "bucketed sparse-embedding exchange": B_local*T rows per rank,
                                            padded to a common row count with id 0 (skipped by the scatter)
  6. local       scatter-add all rows into dE_item, then the norms of the dense weights.

xGMI is point-to-point (7 links/GPU): step 1 moves ~106 MB per rank at the Globo size and dominates; it only
depends on dE, so the rank-local backward runs dE FIRST and `DPEngine` starts step 1 on a communication stream the
moment dE is complete (an event recorded by the C++ driver): the all-reduce runs beside dX, the attention / projection
backward and the weight gradients; the sparse-row all-gather and the arena all-reduce are queued behind it on the same
stream as soon as the rank-local backward has produced them, and the main stream joins once, before step 2.  Step 1 is
sent as two all-reduces, the candidate-time block first, so that step 4 can run (into a scratch block, added to the arena
after step 3) while the item block is still on the wire.
`GradExchange` is device-agnostic (tests run it over gloo on CPU tensors with the oracle's gradients).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Callable, Dict, Optional

import numpy as np
import torch
import torch.distributed as dist

from . import _lib
from ._lib import check
from .engine import TIME_SHORT, TcarEngine


class _GroupOps:
    """The process group behind the three calls of rccl.RcclComm (`Collectives.ops`, the known-answer check)."""

    def __init__(self, group):
        self.group = group

    def all_gather(self, send: torch.Tensor, recv: torch.Tensor):
        dist.all_gather_into_tensor(recv.view(-1), send.reshape(-1), group=self.group)

    def reduce_scatter(self, send: torch.Tensor, recv: torch.Tensor):
        dist.reduce_scatter_tensor(recv, send, group=self.group)

    def all_reduce(self, t: torch.Tensor):
        dist.all_reduce(t, group=self.group)

    def all_to_all(self, send: torch.Tensor, recv: torch.Tensor):
        dist.all_to_all_single(recv.view(-1), send.reshape(-1), group=self.group)


class Collectives:
    """The collectives of both exchanges (`GradExchange` below, `sharded.ShardExchange`: each is this layer plus its schedule),
    issued one way for both: `ops` is the direct RCCL communicator (rccl.py, on torch's current stream) or the process group.
    Every decision the exchanges need is taken here:
      collective   a live group of more than one rank, or `force` (TCAR_FORCE_COLLECTIVES=1: a group of ONE rank still issues
                   every collective of the schedule, with identity results); otherwise every collective short-circuits
      world, rank  the group's; arguments may set them only where no collective runs
      sim          the shapes of a `world`-rank job and no collective: every all-gather repeats the local rows, the reduce-scatter
                   keeps the first slice.  None: TCAR_SIM_WORLD=W on ONE process without a process group (rank 0 of W; the
                   per-rank compute of a large job on one GPU, results meaningless beyond their shapes)
      direct       None: RCCL directly on the nccl backend unless TCAR_RCCL_DIRECT=0; False: the process group; True: required
      reduce_scatter   None: where the backend has one (nccl); otherwise all-reduce + slice
      all_to_all   None: tried where collectives are live — the direct communicator says at its self-test whether it has one
                   (rccl.make_direct), a process group whose backend raises at the first call is remembered as having none;
                   without one all_to_all_rows is an all-gather + slice.  `all_to_all_path` names the path taken
    Collectives issued with a key are counted for bench.py and the tests: `order`, `bytes_moved`, and with `timing` on (never in a
    headline pass: an event pair costs its stream a few us) a span per call — CUDA events on the issuing stream, host seconds on
    CPU — averaged by collective_ms()."""

    def __init__(self, group=None, world: Optional[int] = None, rank: Optional[int] = None, sim: Optional[bool] = False,
                 reduce_scatter: Optional[bool] = None, force: Optional[bool] = None, direct: Optional[bool] = None,
                 all_to_all: Optional[bool] = None):
        live = dist.is_available() and dist.is_initialized()
        if sim is None:
            w = int(os.environ.get("TCAR_SIM_WORLD", "0")) if not live and world is None else 0
            sim = w > 1
            if sim:
                world, rank = w, 0
        self.group, self.sim = group, bool(sim)
        self.world = world if world is not None else (dist.get_world_size(group) if live else 1)
        self.rank = rank if rank is not None else (dist.get_rank(group) if live else 0)
        if force is None:
            force = bool(int(os.environ.get("TCAR_FORCE_COLLECTIVES", "0") or 0))
        self.collective = live and not self.sim and (self.world > 1 or bool(force))
        self.backend = dist.get_backend(group) if self.collective else "none"
        if self.collective and (self.world, self.rank) != (dist.get_world_size(group), dist.get_rank(group)):
            # (the reduce-scatter fallback slices, and the in-place item-row all-gather sends from, slot `rank`: RCCL's
            #  sendbuff == recvbuff + rank * count holds only for the communicator's own rank, which is the group's)
            raise ValueError("rank %d of %d, but the process group has this process as rank %d of %d"
                             % (self.rank, self.world, dist.get_rank(group), dist.get_world_size(group)))
        self.use_reduce_scatter = (self.backend == "nccl") if reduce_scatter is None else bool(reduce_scatter)
        # RCCL called directly adds no stream beside the four the step keeps busy (why that matters: rccl.py).  make_direct is a
        # collective: every rank of an nccl group calls it, also one whose `direct` / TCAR_RCCL_DIRECT says no (it votes no)
        self.direct = None
        if self.collective and self.backend == "nccl":
            from . import rccl
            self.direct = rccl.make_direct(group, want=direct is not False and os.environ.get("TCAR_RCCL_DIRECT", "1") != "0")
            if direct is True and self.direct is None:
                raise RuntimeError("the direct RCCL path was required and could not be built")
        self.ops = self.direct if self.direct is not None else _GroupOps(group)
        self.use_all_to_all = (getattr(self.ops, "has_all_to_all", True) if all_to_all is None else bool(all_to_all)) and self.collective
        self.all_to_all_path = "none"
        self.bytes_moved: Dict[str, int] = {}
        self.order = []
        self.timing = False
        self._times: Dict[str, list] = {}
        self._pending_rows = None

    def close(self):
        """Destroy the direct communicator (idempotent) once every collective issued on it has finished (the engines' close()
        synchronises first).  A collective issued afterwards goes to the destroyed communicator (an RCCL error), never silently to
        the process group."""
        if self.direct is not None:
            self.direct.destroy()

    def _timed(self, key, t, fn, *args, **kw):
        """issue collective fn(*args, **kw) and, when timing is on, bracket it (for an async collective: the issue only)"""
        if not self.timing or key is None:
            return fn(*args, **kw)
        if t.is_cuda:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*args, **kw)
            e1.record()
            self._times.setdefault(key, []).append((e0, e1))
        else:
            import time
            t0 = time.perf_counter()
            out = fn(*args, **kw)
            self._times.setdefault(key, []).append((t0, time.perf_counter()))
        return out

    def _note(self, key, t):
        if key is not None:
            self.bytes_moved[key] = t.numel() * t.element_size()
            self.order.append(key)

    def collective_ms(self) -> Dict[str, float]:
        """mean milliseconds per collective over the timed steps (call after a device synchronise)"""
        out = {}
        for key, spans in self._times.items():
            if not spans:
                continue
            if isinstance(spans[0][0], float):
                out[key] = round(1e3 * sum(b - a for a, b in spans) / len(spans), 4)
            else:
                out[key] = round(sum(a.elapsed_time(b) for a, b in spans) / len(spans), 4)
        return out

    def all_gather(self, t: torch.Tensor, key: Optional[str] = None) -> torch.Tensor:
        """[..] -> [W, ..] (rank-major); no collective: a view (sim: W copies)"""
        if self.sim:
            return t.unsqueeze(0).expand((self.world,) + tuple(t.shape)).contiguous()
        if not self.collective:
            return t.unsqueeze(0)
        out = torch.empty((self.world,) + tuple(t.shape), dtype=t.dtype, device=t.device)
        self._timed(key, t, self.ops.all_gather, t.contiguous(), out)
        self._note(key, out)
        return out

    def reduce_scatter_rows(self, full: torch.Tensor, cap: int, key: Optional[str] = None) -> torch.Tensor:
        """sum over the ranks of full [W*cap, C]; returns this rank's rows [cap, C]"""
        if not self.collective:
            return full[:cap]
        self._note(key, full)
        if self.use_reduce_scatter:
            out = torch.empty(cap, full.shape[1], dtype=full.dtype, device=full.device)
            self._timed(key, full, self.ops.reduce_scatter, full.contiguous(), out)
            return out
        self._timed(key, full, self.ops.all_reduce, full)     # gloo (CPU tests, single-GPU dry runs): all-reduce + slice
        return full[self.rank * cap:(self.rank + 1) * cap]

    def all_to_all_rows(self, t: torch.Tensor, cap: int, key: Optional[str] = None) -> torch.Tensor:
        """t [W*cap, x] -> [W, cap, x]: the rows [rank cap, (rank + 1) cap) of EVERY rank's t, rank-major — what this rank needs of a
        result every rank holds for the sessions of all ranks, a W-th of what an all-gather would move.  No collective: a view of
        this rank's rows (sim: W copies of them); a backend without an all-to-all: all-gather + slice, the same bytes out"""
        mine = t[self.rank * cap:(self.rank + 1) * cap]
        if self.sim:
            return mine.unsqueeze(0).expand((self.world,) + tuple(mine.shape)).contiguous()
        if not self.collective:
            return mine.unsqueeze(0)
        self._note(key, t)
        t = t.contiguous()
        if self.use_all_to_all:
            out = torch.empty((self.world, cap) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
            try:
                self._timed(key, t, self.ops.all_to_all, t, out)
                self.all_to_all_path = "all-to-all (%s)" % ("RCCL C API" if self.direct is not None else self.backend)
                return out
            except (RuntimeError, NotImplementedError, AttributeError) as e:
                # a backend without the collective refuses on every rank alike, before anything is sent: remembered, not fatal
                self.use_all_to_all = False
                self.all_to_all_error = "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:120] if str(e) else "")
        full = torch.empty((self.world,) + tuple(t.shape), dtype=t.dtype, device=t.device)
        self._timed(key, t, self.ops.all_gather, t, full)
        self.all_to_all_path = "all-gather + slice (%s)" % self.backend
        return full[:, self.rank * cap:(self.rank + 1) * cap].contiguous()

    def all_reduce(self, t: torch.Tensor, key: Optional[str] = None) -> torch.Tensor:
        """in-place sum over the ranks (direct: asserts contiguity — an in-place collective on a copy would be lost)"""
        if self.collective:
            self._timed(key, t, self.ops.all_reduce, t)
            self._note(key, t)
        return t

    def agree(self, digest: bytes, key: Optional[str] = "update_digest", device=None) -> None:
        """Every rank holds the same 16 bytes, or TcarError: ONE all-gather of the digest as four int32 words (on the CPU for a gloo
        group, on `device` — default: the current one — for nccl and the direct RCCL communicator), then every rank looks at the
        same [W, 4] table, so a disagreement raises on EVERY rank, naming the ranks whose digest differs from rank 0's.  The host
        reads the gathered table: this is the one synchronisation of a catalog update (shard_update_items / replica_update_items
        with verify=True); nothing else of an update waits for the device.  Without live collectives (one rank, a sim world): a
        no-op, nothing is gathered and nothing is waited for."""
        if not self.collective:
            return
        if len(digest) != 16:
            raise ValueError("agree() takes a digest of 16 bytes")
        words = torch.from_numpy(np.frombuffer(digest, dtype=np.int32).copy())
        if self.backend != "gloo":
            words = words.to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
        table = self.all_gather(words, key).cpu()
        differ = [r for r in range(self.world) if not torch.equal(table[r], table[0])]
        if differ:
            raise _lib.TcarError("the ranks do not agree on the update: the request of rank%s %s differs from rank 0's (seen on rank %d); "
                                 "nothing was written" % ("s" if len(differ) > 1 else "", ", ".join(str(r) for r in differ), self.rank))

    def share_rows(self, stage: torch.Tensor, install) -> None:
        """the item-row all-gather: `stage` [W, S, ldh] holds this rank's updated rows in slot `rank`; issued asynchronously —
        wait_rows() calls `install(stage)` to copy the gathered table into place once it has landed"""
        if not self.collective:
            return
        mine = stage[self.rank].reshape(-1)
        if self.direct is not None:
            # on the step's own stream: nothing of this rank runs between the update and the next step's gathers, which need the
            # rows anyway — a side stream would buy no overlap and cost a hardware queue (rccl.py).  IN PLACE: this rank's rows
            # already sit in their slot of the gathered table (RCCL: sendbuff == recvbuff + rank * sendcount), no staging copy
            work = self._timed("item_rows (issue)", stage, self.direct.all_gather, mine, stage.view(-1))
        else:
            mine = mine.clone()
            work = self._timed("item_rows (issue)", stage, dist.all_gather_into_tensor, stage.view(-1), mine, group=self.group,
                               async_op=True)
        self._note("item_rows", stage)
        self._pending_rows = (work, stage, install, mine)

    def wait_rows(self) -> None:
        if self._pending_rows is not None:
            work, stage, install, _ = self._pending_rows
            self._pending_rows = None
            if work is not None:
                work.wait()                   # NCCL: orders the current stream behind the collective, no host block
            install(stage)


def update_digest(ids, content, item_rows, mwdhm, keys, categories) -> bytes:
    """16 bytes that name the request of a catalog update — what the ranks compare in Collectives.agree.  Takes the VALIDATED arrays
    of TcarEngine._update_request (int32 / float32, None where the call brings none): blake2b over U, the mask of the fields that
    are present and the bytes of each, contiguous, in request order.  Requests that validate to the same arrays (a list, an int64
    array, a tensor of the same values) hash equal; any changed element, field or order does not."""
    import hashlib
    fields = (ids, content, item_rows, mwdhm, keys, categories)
    h = hashlib.blake2b(digest_size=16)
    h.update(np.asarray([int(ids.size), sum(1 << i for i, x in enumerate(fields) if x is not None)], dtype=np.int64).tobytes())
    for x, dt in zip(fields, (np.int32, np.float32, np.float32, np.int32, np.int32, np.int32)):
        if x is not None:
            h.update(np.ascontiguousarray(x, dtype=dt).tobytes())
    return h.digest()


class GradExchange(Collectives):
    """The collective schedule above, independent of where the local pieces come from."""

    def __init__(self, group=None, force=None, direct=None):
        super().__init__(group, force=force, direct=direct)

    def communicate(self, big: torch.Tensor, arena_pieces: torch.Tensor, ids: torch.Tensor, rows: torch.Tensor,
                    big_done: bool = False):
        """Every collective of the step, in ONE canonical order on every rank (also the ranks whose shard is empty):
        all-reduce big (1) -> all-gather ids, rows (5) -> all-reduce arena (3).  None of them depends on another one's
        result, so a caller may issue them back to back on a communication stream.  `big_done`: (1) was already issued."""
        if not self.collective:
            return ids.reshape(-1), rows.reshape(-1, rows.shape[-1])
        if not big_done:
            for part in (big if isinstance(big, (list, tuple)) else (big,)):
                self.all_reduce(part)                                       # 1  (parts in the caller's canonical order)
        all_ids = self.all_gather(ids)                                      # 5
        all_rows = self.all_gather(rows)
        self.all_reduce(arena_pieces)                                       # 3
        return all_ids.view(-1), all_rows.view(-1, rows.shape[-1])

    @staticmethod
    def finish(all_ids: torch.Tensor, all_rows: torch.Tensor, sqnorm_item: Callable[[], None],
               cand_time_bwd: Callable[[], None], scatter_rows: Callable[[torch.Tensor, torch.Tensor], None],
               sqnorm_dense: Callable[[], None]):
        """The local steps, once every collective has landed."""
        sqnorm_item()                                                       # 2  (before any row is scattered in: S5)
        cand_time_bwd()                                                     # 4  (once, on top of the reduced arena)
        scatter_rows(all_ids, all_rows)                                     # 6
        sqnorm_dense()

    def run(self, big: torch.Tensor, arena_pieces: torch.Tensor, ids: torch.Tensor, rows: torch.Tensor,
            sqnorm_item: Callable[[], None], cand_time_bwd: Callable[[], None],
            scatter_rows: Callable[[torch.Tensor, torch.Tensor], None], sqnorm_dense: Callable[[], None]):
        all_ids, all_rows = self.communicate(big, arena_pieces, ids, rows)
        self.finish(all_ids, all_rows, sqnorm_item, cand_time_bwd, scatter_rows, sqnorm_dense)


def known_answers(ops, world: int, rank: int, dev, caps: Optional[dict] = None) -> Optional[str]:
    """ONE tiny in-place all-reduce, all-gather and reduce-scatter (the three collectives the training exchanges use) through `ops` —
    the process group (`preflight`) or a direct communicator (rccl.make_direct) — on `dev`, then the results of those issued against
    their known answers (every rank issues all three first: a wrong answer stops no rank short of its peers' collectives).  Returns
    None, or "<collective>: <what went wrong>" for the first that answered wrongly, else for the one that raised.
    The all-to-all of the sharded retrieval (Collectives.all_to_all_rows) is OPTIONAL: it is issued last; where `ops` has none (it
    raises, on every rank alike) caps["all_to_all"] is False and nothing is reported — the layer falls back to all-gather + slice —,
    where it answers, the answer is checked like the others."""
    t = torch.full((4,), float(rank + 1), device=dev)
    mine, out = torch.full((3,), float(rank), device=dev), torch.empty(world * 3, device=dev)
    full, part = torch.arange(world * 2, dtype=torch.float32, device=dev) + rank, torch.empty(2, device=dev)
    step, err = "all_reduce", None
    try:
        ops.all_reduce(t)
        step = "all_gather"
        ops.all_gather(mine, out)
        step = "reduce_scatter"
        ops.reduce_scatter(full, part)
        step = "synchronize"
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
    except Exception as e:
        err = "%s: %s: %s" % (step, type(e).__name__, e)
    a2a_send = torch.arange(world * 2, dtype=torch.float32, device=dev) + 100 * rank
    a2a_recv, has_a2a = torch.empty(world * 2, device=dev), False
    if err is None or step == "reduce_scatter":
        try:
            ops.all_to_all(a2a_send, a2a_recv)
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)
            has_a2a = True
        except Exception as e:
            if caps is not None:
                caps["all_to_all_error"] = ("%s: %s" % (type(e).__name__, e)).splitlines()[0][:120]
    if caps is not None:
        caps["all_to_all"] = has_a2a
    for name, got, want in (("all_reduce", t, [world * (world + 1) / 2.0] * 4),
                            ("all_gather", out.view(world, 3)[:, 0], [float(r) for r in range(world)]),
                            ("reduce_scatter", part, [world * (2 * rank + j) + world * (world - 1) / 2.0 for j in range(2)])):
        if err is not None and name == step:
            break
        if got.tolist() != want:
            return "%s: returned %r, expected %r" % (name, got.tolist(), want)
    if has_a2a and a2a_recv.tolist() != [100.0 * r + 2 * rank + j for r in range(world) for j in range(2)]:
        return "all_to_all: returned %r" % (a2a_recv.tolist(),)
    return err


def preflight(group=None, device=None, verbose: bool = True) -> Dict[str, object]:
    """First contact with the process group: `known_answers` through it on `device`, before any large buffer exists.  A job whose
    collectives cannot run fails HERE with the backend, world size, device and library versions in the message instead of inside
    step 1.  Returns the capabilities ({"reduce_scatter": bool, ...}); `reduce_scatter` False (a backend without one: reported,
    not fatal) makes ShardedEngine reduce dX with an all-reduce."""
    import sys
    if not (dist.is_available() and dist.is_initialized()):
        return {"world": 1, "backend": "none", "reduce_scatter": False}
    world, rank, backend = dist.get_world_size(group), dist.get_rank(group), dist.get_backend(group)
    dev = torch.device(device) if device is not None else torch.device("cpu")
    info = {"world": world, "rank": rank, "backend": backend, "device": str(dev), "torch": torch.__version__,
            "hip": getattr(torch.version, "hip", None), "reduce_scatter": False}
    try:
        if backend == "nccl":
            info["rccl"] = ".".join(str(x) for x in torch.cuda.nccl.version())
    except Exception as e:                                   # version query only: never fatal
        info["rccl"] = "unknown (%s)" % type(e).__name__
    bad = known_answers(_GroupOps(group), world, rank, dev, info)
    if bad is not None and (backend == "nccl" or not bad.startswith("reduce_scatter:")):
        raise RuntimeError("collective preflight failed at %s (%s)" % (bad, info))
    info["reduce_scatter"] = bad is None
    if bad is not None:
        info["reduce_scatter_error"] = bad.splitlines()[0][:120]
    if verbose and rank == 0:
        print("[tcar] collective preflight ok: %s" % info, file=sys.stderr)
    return info


def shard_bounds(b: int, world: int, rank: int):
    """Contiguous split of a length-bucketed batch of b sessions (sampler.py:40-49) into `world` shards of
    ceil(b/world); trailing ranks may get fewer (or zero) rows.  Returns (lo, hi, cap)."""
    cap = (b + world - 1) // world
    lo = min(b, rank * cap)
    hi = min(b, lo + cap)
    return lo, hi, cap


class DPEngine(TcarEngine):
    """TcarEngine whose backward ends with the `GradExchange` schedule.  All ranks must call train_step with
    batches of the SAME input length T (they walk the same bucket schedule)."""

    flag_forks = False   # (the gradient exchange is enqueued inside the fused backward: event forks)

    def __init__(self, *a, group=None, force_collectives=None, direct_rccl=None, **kw):
        self.group = group
        self.xch = GradExchange(group, force=force_collectives, direct=direct_rccl)
        if self.xch.collective:
            # (TcarEngine.priority_stream: no priority stream beside live collectives.  One that an earlier engine of this process
            #  made current stays current: restoring the default stream is left for later)
            self.priority_stream = False
        super().__init__(*a, **kw)
        g = self.geo
        # step 1 in two parts, the candidate-time block FIRST: its clip backward can then run (into a scratch copy of the
        # time-table gradients) while the item block is still being reduced
        self.big_parts = [self.big[g.N * g.ldh:], self.big[:g.N * g.ldh]]
        self._ct_rows = 139 * g.ldt
        self._ct_scratch = torch.zeros(self._ct_rows + _lib.NSLOT, dtype=torch.float32, device=self.dev)
        self.rows_cap = 0

    def close(self):
        """Synchronise the device, then destroy the direct RCCL communicator (idempotent).  Call it before
        destroy_process_group(): nothing destroys the communicator at interpreter exit."""
        torch.cuda.synchronize(self.dev)
        self.xch.close()

    def update_items(self, ids, content=None, item_rows=None, mwdhm=None, keys=None, categories=None):
        """not under this name on a replica: every rank holds the whole catalog and the ranks have to agree on an update — that is
        replica_update_items(), a collective"""
        raise _lib.TcarError("update_items() is not for the data-parallel replicas: the ranks would have to agree on the update")

    def warm_start_items(self, ids, k: int = 16, min_sim: float = 0.0, exclude=None, window=None, panel=None):
        """not on a replica: the call writes catalog rows, and the ranks would have to agree on it as they do in
        replica_update_items(); the collective form is not built"""
        raise _lib.TcarError("warm_start_items() needs the whole catalog on one engine, not the data-parallel replicas: the ranks "
                             "would have to agree on the rows")

    def replica_update_items(self, ids, content=None, item_rows=None, mwdhm=None, keys=None, categories=None, verify: bool = True) -> None:
        """TcarEngine.update_items on every replica.  A COLLECTIVE when `verify` is set and collectives are live: every rank passes
        the same request; it is validated (the same ValueErrors, before anything else), the ranks compare its digest
        (Collectives.agree: one all-gather of 16 bytes, the one host synchronisation of the call — a disagreement raises TcarError
        on every rank and nothing is written), then every replica, which holds the whole catalog, applies it with the whole-catalog
        kernel.  verify=False skips the comparison and its synchronisation: the caller vouches for the request."""
        req = self._update_request(ids, content, item_rows, mwdhm, keys, categories)
        if verify:
            self.xch.agree(update_digest(*req), device=getattr(self, "dev", None))
        TcarEngine.update_items(self, *req)

    def _ensure_rows(self, rows: int):
        if rows > self.rows_cap:
            self.rows_buf = torch.zeros(rows, self.geo.ldh, dtype=torch.float32, device=self.dev)
            self.ids_buf = torch.zeros(rows, dtype=torch.int32, device=self.dev)
            self.rows_cap = rows

    def finish_backward(self, bt, cap_rows: Optional[int] = None):
        g, lib, st, p = self.geo, self.lib, self._stream(), self._p
        B, T = (bt.B, bt.T) if bt is not None else (0, 0)
        n_rows = B * T
        cap = max(cap_rows or 0, n_rows)
        self._ensure_rows(max(cap, 1))
        rows, ids = self.rows_buf[:max(cap, 1)], self.ids_buf[:max(cap, 1)]
        if cap > n_rows:
            rows[n_rows:].zero_()
            ids[n_rows:].zero_()
        if bt is not None:
            ids[:n_rows].copy_(bt._seq_t[:n_rows])
            tab, gr = self._tables(), self._grads()
            gr.rows_out = rows.data_ptr()
            check(lib.tcar_gather_clip_bwd(C.byref(self.dims), C.byref(tab), C.byref(bt), p(self.dx_icp), p(self.dx_pt),
                                           p(self.dx_act), p(self.dclick), C.byref(gr), st), "tcar_gather_clip_bwd")

        def scatter(all_ids, all_rows):
            check(lib.tcar_scatter_add_rows(C.byref(self.dims), p(all_ids), p(all_rows), all_ids.numel(), p(self.Gi),
                                            self._stream()), "tcar_scatter_add_rows")

        if self._comm_busy:
            # the big all-reduce is already running on the communication stream (start_big_reduce); queue the other
            # collectives behind it there — they need only the arena / rows this stream has just produced — and join once
            main = torch.cuda.current_stream(self.dev)
            self._comm.wait_stream(main)
            with torch.cuda.stream(self._comm):
                all_ids, all_rows = self.xch.communicate(self.big_parts, self.Gx, ids, rows, big_done=True)
            main.wait_stream(self._comm)
            main.wait_stream(self._aux)                  # the candidate-time backward into the scratch block
            all_ids.record_stream(main)
            all_rows.record_stream(main)
            self._comm_busy = False
            # its table gradients and norm pieces go on top of the REDUCED arena (once, like step 4 of the in-line order)
            o = self.seg["month"]["off"]
            self.Gx[o:o + self._ct_rows] += self._ct_scratch[:self._ct_rows]
            self.sqn_pieces += self._ct_scratch[self._ct_rows:]
            self.xch.finish(all_ids, all_rows, self._sqnorm_item, lambda: None, scatter, self._sqnorm_dense)
            return
        all_ids, all_rows = self.xch.communicate(self.big_parts, self.Gx, ids, rows)
        aux = getattr(self, "_aux", None)
        if aux is not None and self.big.is_cuda:
            # the candidate-time backward (needs only the reduced d_et; adds atomically into the reduced arena) runs on the
            # aux stream beside the item norm, the row scatter and the dense-weight norms
            main = torch.cuda.current_stream(self.dev)
            aux.wait_stream(main)
            with torch.cuda.stream(aux):
                self._cand_time_bwd()
            self.xch.finish(all_ids, all_rows, self._sqnorm_item, lambda: None, scatter, self._sqnorm_dense)
            main.wait_stream(aux)
        else:
            self.xch.finish(all_ids, all_rows, self._sqnorm_item, self._cand_time_bwd, scatter, self._sqnorm_dense)

    _comm_busy = False
    async_exchanges = 0      # steps whose collectives ran on the communication stream (tests assert the path is live)

    def start_big_reduce(self):
        """Step 1 of the exchange, started on a communication stream as soon as dE is complete (event 3 of the C++
        driver, recorded after the dE GEMM + negative rows) so that it overlaps chain A.  Falls back to the in-line
        all-reduce when there is no aux stream / single rank."""
        self._comm_busy = False
        if not self.xch.collective or not self.big.is_cuda or not getattr(self, "_aux_ev", None):
            return
        if not hasattr(self, "_comm"):
            self._comm = torch.cuda.Stream(self.dev)
        self._comm.wait_event(self._aux_ev[3])
        with torch.cuda.stream(self._comm):
            self.xch.all_reduce(self.big_parts[0])                      # candidate-time block
            det_done = torch.cuda.Event()
            det_done.record(self._comm)
            self.xch.all_reduce(self.big_parts[1])                      # item block
        # candidate-side clip backward of the reduced time block, on the aux stream beside the item block's all-reduce,
        # into a scratch copy of the time-table gradients / norm pieces (added to the arena after ITS all-reduce)
        self._aux.wait_event(det_done)
        with torch.cuda.stream(self._aux):
            self._ct_scratch.zero_()
            gr = self._grads()
            base = self._ct_scratch.data_ptr()
            o0 = self.seg["month"]["off"]
            for k, n in enumerate(TIME_SHORT):
                gr.g_time[k] = base + 4 * (self.seg[n]["off"] - o0)
            gr.sqn = base + 4 * self._ct_rows
            check(self.lib.tcar_cand_time_bwd_indexed(C.byref(self.dims), C.byref(self._time_ptrs()), self._p(self.inv_n),
                                                      self._p(self.inv_off), self._p(self.d_et), int(self.scoring_code != 0),
                                                      self._p(self.ct_ws), C.byref(gr), self._stream()),
                  "tcar_cand_time_bwd_indexed")
        self._comm_busy = True
        self.async_exchanges += 1

    def train_step(self, batch, bt=None, cap_rows: Optional[int] = None, T: Optional[int] = None, K: Optional[int] = None):
        """`batch` may be None for a rank whose shard of the global batch is empty (it still joins the collectives).
        T / K: accepted for interface parity with sharded.ShardedEngine (an empty rank needs them there)."""
        self._refuse_ragged(batch, bt, "train_step")
        if batch is None and bt is None:
            self.Gx.zero_()
            self.big.zero_()
            self.sqn_dense.zero_()
            self.finish_backward(None, cap_rows)
            self.update()
            return torch.zeros(0, device=self.dev)
        bt = bt or self.upload(batch)
        self._local(bt)
        self.finish_backward(bt, cap_rows)
        self.update()
        return self._loss_view(bt)

    def update(self):
        if self.native:
            if self.work_B == 0:
                # a rank whose very first shard is empty has no workspace yet: give it a minimal one, so that the update
                # always goes through tcar_step_update (which also refreshes the bf16 planes of the item table)
                self._ensure_work(1, 1)
            check(self.lib.tcar_step_update(C.byref(self._ctx()), self._lr_t(), self._stream()), "tcar_step_update")
            self._after_update()
        else:
            super().update()

    def _local(self, bt):
        """forward + rank-local backward, driven from C++ (tcar_step_forward / tcar_step_backward_local)."""
        self.flush()
        if self._index_stale:                      # (replica_update_items changed a publish time)
            self._build_time_index()
        if self.native:
            self._ensure_work(bt.B, bt.T)
            ctx, st = self._ctx(), self._stream()
            check(self.lib.tcar_step_forward(C.byref(ctx), C.byref(bt), int(self._time_dirty), st), "tcar_step_forward")
            self._time_dirty = False
            check(self.lib.tcar_step_backward_local(C.byref(ctx), C.byref(bt), st), "tcar_step_backward_local")
            self.start_big_reduce()
        else:
            self.forward(bt)
            self.backward_local(bt)

    def loss_and_grads(self, batch, bt=None, cap_rows: Optional[int] = None):
        self._refuse_ragged(batch, bt, "loss_and_grads")
        bt = bt or self.upload(batch)
        self._local(bt)
        self.finish_backward(bt, cap_rows)
        return self._loss_view(bt)

    def exchange_info(self) -> Dict[str, object]:
        """Bytes this rank hands to the collectives per step (bench.py prints it)."""
        g = self.geo
        big = 4 * g.N * (g.ldh + g.pt)
        arena = 4 * (self.arena_n + _lib.NSLOT)
        return {"mode": "replica", "world": self.xch.world, "allreduce_bytes": big + arena,
                "collectives": ("none" if not self.xch.collective else
                                "RCCL C API on the issuing stream (rccl.py)" if self.xch.direct is not None else
                                "torch.distributed process group"),
                "allgather_bytes_per_session_row": 4 * (g.ldh + 1),
                "note": "all-reduce of the dense item-table block + candidate-time block of dE, all-reduce of the arena, "
                        "all-gather of the (id, row) sparse item rows"}


def make_dp_engine(params, content_emb, mwdhm, device="cuda:0", group=None, scoring="bf16x3", mode="auto", **kw):
    """Data-parallel engine factory.  mode "replica": every rank holds the whole catalog and the dense item gradient is
    all-reduced (`DPEngine`); "sharded": catalog-sharded scoring (`sharded.ShardedEngine`, ~1/8 of the bytes); "auto"
    picks the sharded exchange when there is more than one rank."""
    from .sharded import ShardedEngine       # (here: sharded.py builds on this module)
    world = dist.get_world_size(group) if (dist.is_available() and dist.is_initialized()) else 1
    if mode == "auto":
        mode = "sharded" if (world > 1 and scoring != "f32") else "replica"
    if mode == "sharded":
        return ShardedEngine(params, content_emb, mwdhm, device=device, group=group, scoring=scoring, **kw)
    return DPEngine(params, content_emb, mwdhm, device=device, group=group, scoring=scoring, **kw)
