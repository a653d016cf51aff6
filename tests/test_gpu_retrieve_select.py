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

from gpu_util import lib, ptr  # noqa: F401  (lib: the fixture)
from retrieve_select_case import B, LD, N, PARTITIONS, reference, run

pytestmark = pytest.mark.gpu

CS = (1, 63, 64, 65, 128, 300, 1000, 1024)


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
