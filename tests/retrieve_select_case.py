"""What the op-level tests of the streamed top-C selector share (test_gpu_retrieve_select.py, test_fold_agreement.py;
include/tcar_retrieve.h: tcar_retrieve_reset / _panel / _finish): one fp32 matrix x [B = 5, ld = 5,120] with N = 5,000 scored columns,
exclusion lists, keys and windows, the numpy model's shortlists of them, the partitions of the columns into panels and the run over
one.  test_gpu_retrieve_select.py's header says what every row is there to break."""
import numpy as np
import torch

from gpu_util import ptr
from retrieve_ref import shortlist

B, N, LD, X = 5, 5000, 5120, 24
# (n0, n) of every panel; copied: the slices are copied into buffers of their own (row stride ceil4(n))
PARTITIONS = {"one panel": ([(0, N)], False),
              "panels of 128": ([(n0, min(128, N - n0)) for n0 in range(0, N, 128)], False),
              "1920 + 128 + 2952": ([(0, 1920), (1920, 128), (2048, 2952)], False),
              "1001 + 3999, copied": ([(0, 1001), (1001, 3999)], True)}
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1

_REF = {}


def reference():
    """inputs and the model's shortlists at C = 1,024 (a shortlist of C is their first C columns): computed once, never written"""
    if _REF:
        return _REF
    rng = np.random.RandomState(11)
    x = (rng.standard_normal((B, LD)) * 2).astype(np.float32)
    x[0, :N] = np.arange(N, dtype=np.float32) * 0.01 - 20.0
    x[1, :N] = 30.0 - np.arange(N, dtype=np.float32) * 0.01
    x[2, :N] = -0.75
    sp = rng.permutation(N)
    x[3, sp[:40]] = np.nan
    x[3, sp[40:43]] = np.inf
    x[3, sp[43:46]] = -np.inf
    x[3, sp[46:1300]] = -0.0                                # a quarter of the row each: ties of +0.0 and -0.0 reach every C
    x[3, sp[1300:2600]] = 0.0
    x[3, sp[2600:3800]] = -np.abs(x[3, sp[2600:3800]])      # the rest of the row below zero, so the zeros are inside every shortlist
    x[3, sp[3800:]] = -np.abs(x[3, sp[3800:]])
    x[3, sp[3800:3820]] = np.abs(x[3, sp[3800:3820]]) + 1.0
    x[:, N:] = 1e9
    key = rng.permutation(N).astype(np.int32)
    lo, hi = np.full(B, I32_MIN, np.int64), np.full(B, I32_MAX, np.int64)
    lo[4], hi[4] = 1000, 1200                                # 200 items in the window of row 4 ...
    excl = np.full((B, X), -1, np.int32)
    in_win = np.where((key >= 1000) & (key < 1200))[0]
    excl[4, :20] = in_win[:20]                               # ... 20 of them excluded: a pool of 180
    excl[4, 20:22] = in_win[:2]                              # repeats
    excl[4, 22] = N + 3                                      # an id past the catalog names nothing
    excl[3, 0], excl[3, 5] = sp[40 + 0], sp[3800]            # row 3: one +inf and one of the positive entries go
    excl[0, 3], excl[1, 7], excl[2, 1] = N - 1, 0, N - 1     # the winners of the sorted rows and of the tie row
    lo, hi = lo.astype(np.int32), hi.astype(np.int32)
    plain = shortlist(x[:, :N], 1024)
    full = shortlist(x[:, :N], 1024, excl=excl, key=key, lo=lo, hi=hi)
    assert (full[0][4] >= 0).sum() == 180 and (plain[0] >= 0).all(), ("the pool of row 4", int((full[0][4] >= 0).sum()))
    _REF.update(x=x, key=key, lo=lo, hi=hi, excl=excl, plain=plain, full=full)
    for v in (x, key, lo, hi, excl) + plain + full:
        v.setflags(write=False)
    return _REF


def run(lib, dev, C_, panels, copied, filtered, state=None):
    """reset, one fold per panel, finish -> (ids, scores) as numpy arrays, and the state tensor"""
    x = dev["x"]
    if state is None:
        state = torch.full((int(lib.tcar_retrieve_state_bytes(B, C_)) // 4,), 0x7f7f7f7f, dtype=torch.int32, device="cuda")
    ids = torch.full((B, C_), -7, dtype=torch.int32, device="cuda")
    scores = torch.full((B, C_), -7.0, device="cuda")
    rc = lib.tcar_retrieve_reset(B, C_, ptr(state), None)
    assert rc == 0, ("tcar_retrieve_reset", rc, C_)
    for n0, n in panels:
        if copied:
            ld = (n + 3) // 4 * 4
            buf = torch.full((B, ld), 1e9, device="cuda")
            buf[:, :n] = x[:, n0:n0 + n]
            pp = ptr(buf)
        else:
            ld, pp = LD, ptr(x, n0)
        if filtered:
            rc = lib.tcar_retrieve_panel(B, n0, n, pp, ld, C_, ptr(dev["excl"]), X, ptr(dev["key"]), ptr(dev["lo"]), ptr(dev["hi"]),
                                         ptr(state), None)
        else:
            rc = lib.tcar_retrieve_panel(B, n0, n, pp, ld, C_, None, 0, None, None, None, ptr(state), None)
        assert rc == 0, (n0, n, rc)
    rc = lib.tcar_retrieve_finish(B, C_, ptr(state), ptr(ids), ptr(scores), None)
    assert rc == 0, ("tcar_retrieve_finish", rc, C_)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), scores.cpu().numpy(), state
