"""The basics every GPU test shares: the skip without a GPU, the loaded library as a fixture, pointers into tensors, numpy copies of
device tensors, the KB32 plane layout, and the two comparisons the suite gates on — `close` (the project's logits gate, with a shape
check and an absolute floor) and `close_broadcast` (the same relative + scaled-absolute bound without either, tensors accepted).
The two are different arithmetics; a test keeps the one it was written against."""
import ctypes as C

import numpy as np
import pytest
import torch

RTOL = 1e-3            # north-star tolerance (BASELINE.json): 1e-3 relative


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def close(got, want, rtol=RTOL, atol_scale=2e-5, name=""):
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = max(float(np.abs(want).max()), 1e-30)
    err = np.abs(got - want)
    # absolute floor 1e-9: quantities below fp32 resolution of their inputs (e.g. the gradient through the
    # exp-normaliser of a length-1 session, ~1e-9 relative) are legitimately 0 in fp32 and ~1e-11 in fp64
    tol = rtol * np.abs(want) + atol_scale * scale + 1e-9
    bad = err > tol
    assert not bad.any(), "%s: %d/%d off, max err %.3e (scale %.3e) at %s" % (
        name, bad.sum(), bad.size, err.max(), scale, np.unravel_index(err.argmax(), err.shape))


def close_broadcast(got, want, rtol=RTOL, atol_scale=2e-5, name=""):
    """no shape assertion (the operands broadcast) and no absolute floor; tensors or arrays"""
    got = np.asarray(got.detach().cpu() if torch.is_tensor(got) else got, dtype=np.float64)
    want = np.asarray(want.detach().cpu() if torch.is_tensor(want) else want, dtype=np.float64)
    atol = atol_scale * max(1e-30, float(np.abs(want).max()))
    bad = np.abs(got - want) > atol + rtol * np.abs(want)
    assert not bad.any(), "%s: %d / %d off, max abs err %.3e (max |want| %.3e)" % (
        name, int(bad.sum()), bad.size, float(np.abs(got - want).max()), float(np.abs(want).max()))


@pytest.fixture(scope="module")
def lib():
    _need_gpu()
    from tcar_amd import _lib
    return _lib.load()


def ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off)


def ptr2(t):
    return C.c_void_p(t.data_ptr())


def _np(*ts):
    return [t.cpu().numpy().copy() for t in ts]


def _kb32_index(rows, inner):
    """numpy restatement of csrc/tcar_bf16_layout.h: flat element offset of every (row, k)."""
    r = np.arange(rows)[:, None]
    k = np.arange(inner)[None, :]
    blk = (r >> 7) * (inner // 32) + (k >> 5)
    rr, kk = r & 127, k & 31
    return blk * 4096 + rr * 32 + ((((kk >> 3) ^ ((rr >> 2) & 3)) << 3) | (kk & 7))


def _planes(lib, x):
    """fp32 [rows, cols] -> KB32 hi / lo planes through the product's own tcar_split_bf16; returns (hi, lo, inner, rows)."""
    rows, cols = x.shape
    inner = (cols + 31) // 32 * 32
    rp = (rows + 127) // 128 * 128
    xd = torch.tensor(np.ascontiguousarray(x)).cuda()
    hi = torch.full((rp * inner,), float("nan"), dtype=torch.bfloat16, device="cuda")
    lo = torch.full((rp * inner,), float("nan"), dtype=torch.bfloat16, device="cuda")
    rc = lib.tcar_split_bf16(ptr(xd), cols, rows, cols, ptr2(hi), ptr2(lo), inner, None, None, 0, 0, 0, None)
    assert rc == 0, ("tcar_split_bf16", rc, rows, cols)
    return hi, lo, inner, rows
