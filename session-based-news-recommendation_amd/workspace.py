"""Device workspace of the engines: ONE allocator of grow-only named buffers, and the sizes of the scoring family written once.

An engine states what it needs as rows of tables — `Spec(attr, shape, dtype, fill)` — and `Workspace.ensure` makes them real.  Every
(re-)allocation bumps `Workspace.version`; the descriptors that carry a buffer's pointer to the library (tcar_ctx_t, tcar_shard_t)
are keyed on it, so a re-allocation can never leave a stale pointer behind, and a warm step allocates nothing (version constant).
"""
from __future__ import annotations

import ctypes as C
import weakref
from typing import Callable, Iterable, List, NamedTuple, Optional, Union

import torch

F32, BF16, I32, U8 = torch.float32, torch.bfloat16, torch.int32, torch.uint8
HOST_I32 = C.c_int32          # dtype of a HOST int array (ctypes), e.g. the ints that carry a step's form from its forward to its backward half


def ru(x: int, m: int) -> int:
    return (x + m - 1) // m * m


class Spec(NamedTuple):
    attr: str                 # attribute of the engine the buffer is reachable under
    shape: tuple              # dimension 0 may be over-provided by an existing buffer; the others are strides C is told, and must match
    dtype: object
    fill: Union[None, int, float, Callable] = None      # None: uninitialised; a number: filled with it; callable(tensor): written once, on allocation
    field: Optional[str] = None                         # field of the descriptor that carries the pointer (default: attr)


class Workspace:
    """Grow-only named buffers, kept as attributes of `owner` (tests and tools read eng.logits, eng._ce_ws, eng.s_stats, ...)."""

    def __init__(self, owner, dev: torch.device):
        # (a weak reference: no cycle, so an engine and its device memory are freed the moment its last reference goes, without a gc pass)
        self.owner, self.dev, self.version = weakref.proxy(owner), dev, 0

    def get(self, s: Spec):
        """the buffer of `s`: the existing one when it is large enough, else a new one (and a new `version`)"""
        have, shape, host = getattr(self.owner, s.attr, None), tuple(int(x) for x in s.shape), s.dtype is HOST_I32
        if have is not None and (len(have) >= shape[0] if host else
                                 have.dtype == s.dtype and have.shape[0] >= shape[0] and tuple(have.shape[1:]) == shape[1:]):
            return have
        if host:
            buf = (C.c_int32 * shape[0])()
        elif s.fill is None or callable(s.fill):
            buf = torch.empty(shape, dtype=s.dtype, device=self.dev)
            if s.fill is not None:
                s.fill(buf)
        else:
            buf = torch.full(shape, s.fill, dtype=s.dtype, device=self.dev)
        setattr(self.owner, s.attr, buf)
        self.version += 1
        return buf

    def ensure(self, specs: Iterable[Spec]) -> List[Spec]:
        specs = list(specs)
        for s in specs:
            self.get(s)
        return specs

    def bind(self, desc, specs: Iterable[Spec], sizes: dict = {}, only=None) -> None:
        """desc.<field> = pointer and desc.<sizes[field]> = element count of the buffers of `specs` (`only`: of these fields)"""
        for s in specs:
            f = s.field or s.attr
            if only is not None and f not in only:
                continue
            buf = getattr(self.owner, s.attr)
            dev = isinstance(buf, torch.Tensor)
            setattr(desc, f, buf.data_ptr() if dev else C.cast(buf, C.c_void_p).value)      # (else: a host array)
            if f in sizes:
                setattr(desc, sizes[f], buf.numel() if dev else len(buf))


class ScoreForm(NamedTuple):
    """which optional buffers of the scoring family exist — the predicates of csrc/step.hip (fused_ce / onehot_fwd / onehot_bwd /
    ce_anchored) are over exactly these pointers"""
    planes: bool = False          # split-bf16 planes of the session side (every bf16 scoring mode)
    logits: bool = True           # materialised fp32 logits
    fused_ce: bool = False        # softmax epilogue of the logits GEMM
    onehot_fwd: bool = False      # one-hot form of the candidate-side time scores
    onehot_bwd: bool = False      # one-hot form of the two scoring-gradient GEMMs
    anchored: bool = False        # anchored softmax form


def scoring_specs(g, rows: int, n: int, splitk: int, form: ScoreForm, attr: Callable[[str], str], onehot_fill=None) -> List[Spec]:
    """The buffers of the scoring family for `rows` session rows against `n` candidate rows — TcarEngine: (work_B, N), the sharded
    engine: (world * cap, n_loc).  Every size is a contract with a comment of include/tcar_hip.h, named at its line; `field` is
    the tcar_ctx_t name, `attr(field)` the engine's attribute."""
    rp, npad, atp = ru(rows, 128), ru(n, 128), g.ldh + g.pt
    S = lambda f, shape, dtype, fill=None: Spec(attr(f), shape, dtype, fill, f)
    out = [S("slabs", (splitk, rows, g.ek), F32)]                                       # tcar_shard_t.slabs: [splitk, rows, ek]
    if form.logits:
        out.append(S("logits", (rows, npad), F32))                                      # tcar_shard_t.logits: [rows, ceil128(n)]
    if form.planes:                                                                     # tcar_ctx_t.scoring: a16* [B, ek], ap16* [B, ldh+pt], dl16* [B, Npad] (KB32: 128-row blocks)
        out += [S(f + x, (rp, c), BF16, 0) for f, c in (("a16", g.ek), ("ap16", atp), ("dl16", npad)) for x in "hl"]
    if form.fused_ce:                                                                   # tcar_ctx_t.ce_ws: B * (ceil(N / 64) + 8) * 2 + 4 B floats, 16-byte aligned, + two host ints
        out += [S("ce_ws", (rows * ((n + 63) // 64 + 8) * 2 + 4 * rows + 8,), F32), S("ce_geo", (2,), HOST_I32)]
    if form.onehot_fwd:                                                                 # tcar_ctx_t.oh16: [ceil128(N), 160] static, p16h / p16l [ceil128(B), 160]
        out += [S("oh16", (npad * 160,), BF16, onehot_fill), S("p16h", (rp * 160,), BF16, 0), S("p16l", (rp * 160,), BF16, 0)]
    if form.onehot_bwd:                                                                 # tcar_ctx_t.tclip: [160 ldt + 320], qz [5 N, 2], dP [B, 160]
        out += [S("tclip", (160 * g.ldt + 320,), F32, 0), S("qz", (5 * n * 2,), F32, 0), S("dP", (rows * 160,), F32, 0)]
    if form.anchored:                                                                   # tcar_ctx_t.ce_rowscale: [B, 2], aps16h [ceil128(B), ldh + 5 ldt]
        out += [S("ce_rowscale", (2 * rp,), F32, 0), S("aps16h", (rp, atp), BF16, 0)]
    return out
