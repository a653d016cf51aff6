"""Streamed selection at the op level (include/tcar_serve.h: tcar_select_reset / _panel / _finish) against numpy, exactly.

One fp32 matrix x [B, ldn] per catalog size (tests/select_case.py), built as in test_eval_rows_rank_topk_ce; the panels are pointer
views into it.  The
list, its scores and the rank follow a total order, so they must be the same bits for every partition and on every run."""
import numpy as np
import pytest

import tcar_amd  # noqa: F401

from gpu_util import close, lib  # noqa: F401  (lib: the fixture)
from select_case import KS, PANELS, case, check_lists, run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("N", sorted(PANELS))
def test_streamed_selection_is_exact_for_every_partition(lib, N, k):
    ref = case(N)
    outs = []
    for P in PANELS[N] + (PANELS[N][0],):                 # every partition, the first one twice (two runs)
        tk, sc, rank, ce = run(lib, ref, N, k, P)
        check_lists(ref, N, k, tk, sc, ref["top"])
        assert (rank == ref["rank"]).all(), (P, rank, ref["rank"])
        close(ce, ref["ce"], name="ce P=%d" % P)
        outs.append((tk, sc, rank))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("N", sorted(PANELS))
def test_excluded_items_leave_the_list_only(lib, N, k):
    from oracle.metrics_oracle import topk_list
    ref = case(N)
    B, x = ref["B"], ref["x"]
    P = min(PANELS[N])
    X = 8
    excl = np.full((B, X), -1, np.int32)
    for b in range(B):
        top1 = ref["top"][b][0]
        if N == 7:
            excl[b, :6] = [top1, (top1 + 1) % 7, (top1 + 2) % 7, (top1 + 3) % 7, (top1 + 4) % 7, top1]     # five of the seven, one twice
        else:
            other = (top1 + P) % N if N > P else (top1 + 3) % N       # an item of another panel
            excl[b, [0, 2, 5, 6]] = [top1, other, top1, ref["top"][b][min(3, N - 1)]]                     # slots 1, 3, 4, 7 stay empty
    want = []
    for b in range(B):
        keep = np.setdiff1d(np.arange(N), excl[b][excl[b] >= 0])        # ascending ids of the items that stay
        want.append([int(keep[j]) for j in topk_list(x[b, keep], k)])
    plain = {Pp: run(lib, ref, N, k, Pp) for Pp in PANELS[N]}
    for Pp in PANELS[N]:
        tk, sc, rank, ce = run(lib, ref, N, k, Pp, excl)
        check_lists(ref, N, k, tk, sc, want)
        assert (rank == plain[Pp][2]).all() and ce.tobytes() == plain[Pp][3].tobytes()      # count and softmax see every item
