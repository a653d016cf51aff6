"""RCCL's C API through ctypes: the collectives of the two exchanges issued DIRECTLY on the stream the step runs on.

Why (round 6, `profiles/r06_ab_experiments.txt` section 4): `torch.distributed` runs every collective on a stream of
ProcessGroupNCCL's own.  The training step already keeps four streams busy (main, aux, third, the sampler's) and HIP multiplexes
streams onto FOUR hardware queues by default: with a fifth stream two of them share a queue, and — which two depends on creation
order and on GPU_MAX_HW_QUEUES — the catalog-sharded step with live collectives ran at 1.6-1.9 ms instead of 0.65-0.73 ms on a
world-1 communicator.  `ncclAllGather` / `ncclReduceScatter` / `ncclAllReduce` issued on OUR stream add no stream: they are
stream-ordered behind the kernels that produced their input and in front of the kernels that read their output, no event, no hop
(and one C call each: ~10 us of host time against ~30 through the process group).

The communicator is built once per exchange (dp.Collectives) from a `ncclUniqueId` that rank 0 creates and `torch.distributed`
broadcasts: the process group stays the rendezvous and the fallback — `make_direct` agrees through it, on ALL ranks, whether the
direct path is taken.  `librccl.so` is the copy bundled with PyTorch-ROCm (the one the `nccl` backend itself uses), so both paths
share one RCCL.

Not a compatibility layer: RCCL is the only backend this talks to."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch
import torch.distributed as dist

NCCL_UNIQUE_ID_BYTES = 128
_DT = {torch.float32: 7, torch.int32: 2, torch.uint8: 1, torch.int64: 4, torch.bfloat16: 9, torch.float64: 8}
_SUM, _MAX = 0, 2


class _UniqueId(C.Structure):
    _fields_ = [("internal", C.c_char * NCCL_UNIQUE_ID_BYTES)]


class RcclError(RuntimeError):
    pass


_LIB = None


def _lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        path = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
        lib = C.CDLL(path if os.path.exists(path) else "librccl.so")
        vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
        lib.ncclGetUniqueId.argtypes = [C.POINTER(_UniqueId)]
        lib.ncclCommInitRank.argtypes = [C.POINTER(vp), i32, _UniqueId, i32]
        lib.ncclCommDestroy.argtypes = [vp]
        lib.ncclAllGather.argtypes = [vp, vp, sz, i32, vp, vp]
        lib.ncclReduceScatter.argtypes = [vp, vp, sz, i32, i32, vp, vp]
        lib.ncclAllReduce.argtypes = [vp, vp, sz, i32, i32, vp, vp]
        if hasattr(lib, "ncclAllToAll"):          # (RCCL's own: the sharded retrieval falls back to all-gather + slice without it)
            lib.ncclAllToAll.argtypes = [vp, vp, sz, i32, vp, vp]
            lib.ncclAllToAll.restype = i32
        lib.ncclGetErrorString.argtypes = [i32]
        lib.ncclGetErrorString.restype = C.c_char_p
        for f in ("ncclGetUniqueId", "ncclCommInitRank", "ncclCommDestroy", "ncclAllGather", "ncclReduceScatter", "ncclAllReduce"):
            getattr(lib, f).restype = i32
        _LIB = lib
    return _LIB


def _ck(rc: int, what: str):
    if rc != 0:
        raise RcclError("%s failed: %s" % (what, _lib().ncclGetErrorString(rc).decode(errors="replace")))


class RcclComm:
    """One RCCL communicator over the ranks of `group` (a COLLECTIVE constructor: every rank of the group calls it, on the device
    it computes on).  Tensors must be contiguous and live on that device; `stream` defaults to torch's current stream."""

    def __init__(self, group=None, device=None):
        if not (dist.is_available() and dist.is_initialized()):
            raise RcclError("no process group to exchange the communicator id through")
        self.group = group
        self.world, self.rank = dist.get_world_size(group), dist.get_rank(group)
        self.dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        lib = _lib()
        uid = _UniqueId()
        if self.rank == 0:
            _ck(lib.ncclGetUniqueId(C.byref(uid)), "ncclGetUniqueId")
        on_dev = dist.get_backend(group) == "nccl"
        raw0 = C.string_at(C.addressof(uid), NCCL_UNIQUE_ID_BYTES) if self.rank == 0 else bytes(NCCL_UNIQUE_ID_BYTES)
        buf = torch.tensor(list(raw0), dtype=torch.uint8)
        if on_dev:
            buf = buf.to(self.dev)
        src = dist.get_global_rank(group, 0) if group is not None else 0
        dist.broadcast(buf, src, group=group)
        raw = bytes(buf.cpu().tolist())
        C.memmove(C.addressof(uid), raw, NCCL_UNIQUE_ID_BYTES)
        self.comm = C.c_void_p()
        with torch.cuda.device(self.dev):
            _ck(lib.ncclCommInitRank(C.byref(self.comm), self.world, uid, self.rank), "ncclCommInitRank")
        self._lib = lib

    def _st(self, stream):
        return C.c_void_p(stream if stream is not None else torch.cuda.current_stream(self.dev).cuda_stream)

    def all_gather(self, send: torch.Tensor, recv: torch.Tensor, stream: Optional[int] = None):
        """recv [world * send.numel()] <- every rank's send (rank-major)"""
        assert send.is_contiguous() and recv.is_contiguous() and recv.numel() == self.world * send.numel() and send.dtype == recv.dtype
        _ck(self._lib.ncclAllGather(C.c_void_p(send.data_ptr()), C.c_void_p(recv.data_ptr()), send.numel(), _DT[send.dtype], self.comm,
                                    self._st(stream)), "ncclAllGather")

    def reduce_scatter(self, send: torch.Tensor, recv: torch.Tensor, stream: Optional[int] = None):
        """recv [send.numel() / world] <- this rank's block of the element-wise sum of every rank's send"""
        assert send.is_contiguous() and recv.is_contiguous() and send.numel() == self.world * recv.numel() and send.dtype == recv.dtype
        _ck(self._lib.ncclReduceScatter(C.c_void_p(send.data_ptr()), C.c_void_p(recv.data_ptr()), recv.numel(), _DT[send.dtype], _SUM,
                                        self.comm, self._st(stream)), "ncclReduceScatter")

    def all_reduce(self, t: torch.Tensor, op: int = _SUM, stream: Optional[int] = None):
        """in place"""
        assert t.is_contiguous()
        _ck(self._lib.ncclAllReduce(C.c_void_p(t.data_ptr()), C.c_void_p(t.data_ptr()), t.numel(), _DT[t.dtype], op, self.comm,
                                    self._st(stream)), "ncclAllReduce")

    def all_to_all(self, send: torch.Tensor, recv: torch.Tensor, stream: Optional[int] = None):
        """recv block r <- block `rank` of rank r's send; blocks of send.numel() / world elements; never in place"""
        assert send.is_contiguous() and recv.is_contiguous() and send.numel() == recv.numel() and send.numel() % self.world == 0
        assert send.dtype == recv.dtype and send.data_ptr() != recv.data_ptr()
        _ck(self._lib.ncclAllToAll(C.c_void_p(send.data_ptr()), C.c_void_p(recv.data_ptr()), send.numel() // self.world, _DT[send.dtype],
                                   self.comm, self._st(stream)), "ncclAllToAll")

    def destroy(self):
        if getattr(self, "comm", None) is not None and self.comm.value:
            self._lib.ncclCommDestroy(self.comm)
            self.comm = C.c_void_p()


def _local_check(want: bool) -> Optional[str]:
    """What this rank can tell on its own: None when the direct path may be tried, else why not."""
    if not want:
        return "switched off"
    try:
        _lib()                                # librccl.so loads and every symbol it binds resolves
    except Exception as e:
        return "%s: %s" % (type(e).__name__, e)
    return None


def _agree(ok: bool, group, dev) -> bool:
    """True on every rank when `ok` holds on every rank (a MIN all-reduce through the process group)."""
    flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=dev)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
    return int(flag.item()) == 1


def make_direct(group=None, device=None, want: bool = True, verbose: bool = True) -> Optional[RcclComm]:
    """ONE direct communicator over the ranks of `group` (nccl backend), or None — on EVERY rank: a collective call that every rank
    makes, also one that does not `want` the direct path (TCAR_RCCL_DIRECT=0, direct=False: it votes no).  Two agreements through
    the process group: the first, before any rank broadcasts an id or enters ncclCommInitRank, over what each rank can check alone
    (`want`, librccl.so and its symbols); the second over the communicator's known answers (dp.known_answers).
    Not handled (left for later): a rank that fails or hangs INSIDE the id broadcast or ncclCommInitRank leaves its peers there —
    that needs a watchdog or the non-blocking ncclCommInitRankConfig."""
    from .dp import known_answers
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    err = _local_check(want)
    comm = None
    if _agree(err is None, group, dev):
        try:
            comm = RcclComm(group, dev)
            caps = {}
            err = known_answers(comm, comm.world, comm.rank, dev, caps)
            comm.has_all_to_all = bool(caps.get("all_to_all"))
        except Exception as e:
            err = "%s: %s" % (type(e).__name__, e)
        if _agree(err is None, group, dev):
            return comm
    if verbose and want:
        import sys
        print("[tcar] direct RCCL path unavailable (%s): collectives through torch.distributed" % (err or "on another rank"),
              file=sys.stderr)
    if comm is not None:
        comm.destroy()
    return None
