"""The streamed top-C selector at the op level (include/tcar_retrieve.h: tcar_retrieve_reset / _panel / _finish) against the numpy
model of tests/retrieve_ref.py, bit for bit: the list order is total, so ids, scores and padding must be the same bits for every
partition of the columns into panels and on every run.

One fp32 matrix x [B = 5, ld = 5,120] with N = 5,000 scored columns (the padding holds 1e9 and must never be picked); the panels of
the first three partitions are pointer views into it (ld > n), the fourth copies its slices so that a panel may start at a column
that is no multiple of four (the key slice is then misaligned and the last group of a row is partial).  One row per thing to break:
  0  scores ascending in column order: every element is admitted, many prunes      3  NaN, +inf, -inf, -0.0 and +0.0 entries
  1  scores descending: nothing after the first C                                  4  random; with `excl` (repeats, -1 slots, ids
  2  all scores equal: the id alone decides                                           past the catalog) and a window its pool is 180 items
Every C runs plain (no excl, no window: the unwindowed kernel) and with excl + window (rows 0 - 3: a window of all int32)."""
import ctypes as C

import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401

from retrieve_ref import shortlist
from select_util import lib, ptr  # noqa: F401  (lib: the fixture)

pytestmark = pytest.mark.gpu

B, N, LD, X = 5, 5000, 5120, 24
CS = (1, 63, 64, 65, 128, 300, 1000, 1024)
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
    assert (full[0][4] >= 0).sum() == 180 and (plain[0] >= 0).all()
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
    assert lib.tcar_retrieve_reset(B, C_, ptr(state), None) == 0
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
    assert lib.tcar_retrieve_finish(B, C_, ptr(state), ptr(ids), ptr(scores), None) == 0
    torch.cuda.synchronize()
    return ids.cpu().numpy(), scores.cpu().numpy(), state


@pytest.fixture(scope="module")
def dev(lib):
    r = reference()
    return {n: torch.tensor(np.array(r[n])).cuda() for n in ("x", "key", "lo", "hi", "excl")}


@pytest.mark.parametrize("C_", CS)
def test_the_shortlist_is_the_models_for_every_partition_bit_for_bit(lib, dev, C_):
    r = reference()
    for filtered in (False, True):
        want_ids, want_sc = (a[:, :C_] for a in r["full" if filtered else "plain"])
        for name, (panels, copied) in PARTITIONS.items():
            ids, sc, state = run(lib, dev, C_, panels, copied, filtered)
            what = (C_, name, "excl + window" if filtered else "plain")
            for b in range(B):
                assert (ids[b] == want_ids[b]).all(), what + (b, int(np.argmax(ids[b] != want_ids[b])))
                assert sc[b].tobytes() == want_sc[b].tobytes(), what + (b,)
            if name == "1920 + 128 + 2952":         # a second reset / fold / finish on the same state: equal bits
                ids2, sc2, _ = run(lib, dev, C_, panels, copied, filtered, state=state)
                assert ids2.tobytes() == ids.tobytes() and sc2.tobytes() == sc.tobytes(), what


def test_argument_errors_launch_nothing(lib, dev):
    C_ = 64
    words = int(lib.tcar_retrieve_state_bytes(B, C_)) // 4
    assert words == B * (2 * C_ + 4)
    state = torch.full((words,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    ids = torch.full((B, C_), -7, dtype=torch.int32, device="cuda")
    big = torch.zeros(49160 + 8, device="cuda")
    x = dev["x"]
    fold = lambda n, p, ld, c, b=B: lib.tcar_retrieve_panel(b, 0, n, p, ld, c, None, 0, None, None, None, ptr(state), None)
    assert fold(N, ptr(x), LD, 0) == -1 and fold(N, ptr(x), LD, 1025) == -1
    assert fold(49153, ptr(big), 49156, C_, 1) == -1                      # n > 49,152
    assert fold(N, ptr(x, 1), LD, C_) == -1                                # a misaligned panel
    assert fold(N, ptr(x), LD - 2, C_) == -1                               # ld % 4
    assert lib.tcar_retrieve_reset(B, 0, ptr(state), None) == -1 and lib.tcar_retrieve_reset(B, 1025, ptr(state), None) == -1
    assert lib.tcar_retrieve_finish(B, 0, ptr(state), ptr(ids), None, None) == -1
    assert lib.tcar_retrieve_finish(B, 1025, ptr(state), ptr(ids), None, None) == -1
    # a short state: the step's descriptor names its size
    from tcar_amd import _lib
    ctx, bt, d = _lib.Ctx(), _lib.Batch(), _lib.Retrieve()
    bt.B, bt.T = B, 3
    d.C, d.panel, d.panel_buf, d.state, d.state_bytes, d.ids = C_, 128, x.data_ptr(), state.data_ptr(), words * 4 - 4, ids.data_ptr()
    assert lib.tcar_retrieve_step(C.byref(ctx), C.byref(bt), 0, C.byref(d), None) == -1
    torch.cuda.synchronize()
    assert bool((state == 0x5a5a5a5a).all()) and bool((ids == -7).all())
