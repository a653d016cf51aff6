"""tcar_cand_rank at the op level (include/tcar_cand.h) against the numpy model of tests/cand_ref.py: ranks, the list order and the
pair counts exactly — the scores are quantised to eight levels, so ties are everywhere and every level of the order is reached — and
the three float metrics within the bound of an fp32 sum."""
import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401

from cand_ref import rank_model
from gpu_util import lib, ptr  # noqa: F401  (lib: the fixture)

pytestmark = pytest.mark.gpu

B = 6
RTOL = 1e-4              # >= C 2^-24 at C = 1024: the bound of an fp32 sum of C positive terms


def _inputs(C):
    """scores on 8 levels (no NaN, no -0.0), ids from a small range (repeats), empty slots by id and by score; row 3 all positive,
    row 4 all negative, row 5 all empty.  The rows have strides of their own."""
    rng = np.random.RandomState(C)
    score = (rng.randint(0, 8, (B, C)) / 4.0 + 0.25).astype(np.float32)
    cand = rng.randint(0, max(2, C // 3), (B, C)).astype(np.int32)
    clicked = (rng.rand(B, C) < 0.3).astype(np.int32)
    gone = rng.rand(B, C) < 0.2
    gone[3:5] = False
    gone[5] = True
    cand[gone & (rng.rand(B, C) < 0.7)] = -1              # most empty slots carry -1 AND -inf, as tcar_cand_scores leaves them
    score[gone] = -np.inf
    clicked[3], clicked[4] = 1, 0
    return score, cand, clicked


def _padded(x, extra, fill):
    t = torch.full((x.shape[0], x.shape[1] + extra), fill, dtype=torch.from_numpy(x).dtype)
    t[:, :x.shape[1]] = torch.from_numpy(x)
    return t.cuda()


@pytest.mark.parametrize("C", [1, 2, 65, 1024])
def test_ranks_order_counts_and_metrics_equal_the_numpy_model(lib, C):
    score, cand, clicked = _inputs(C)
    want_rank, want_order, want_counts, want_metrics = rank_model(score, cand, clicked)
    st, ct, kt = _padded(score, 3, 7.0), _padded(cand, 1, 5), _padded(clicked, 2, 1)
    new = lambda shape, dtype: torch.full(shape, -77, dtype=dtype, device="cuda")
    rank_of, order, counts, metrics = new((B, C), torch.int32), new((B, C), torch.int32), new((B, 3), torch.int32), new((B, 3), torch.float32)
    call = lambda clk, r, o, c, m: lib.tcar_cand_rank(B, C, ptr(st), C + 3, ptr(ct), C + 1, ptr(clk) if clk is not None else None, C + 2,
                                                      ptr(r) if r is not None else None, ptr(o) if o is not None else None,
                                                      ptr(c) if c is not None else None, ptr(m) if m is not None else None, None)
    assert call(kt, rank_of, order, counts, metrics) == 0
    torch.cuda.synchronize()
    got = [t.cpu().numpy().copy() for t in (rank_of, order, counts, metrics)]
    assert (got[0] == want_rank).all() and (got[1] == want_order).all()
    assert (got[2] == want_counts).all(), (got[2], want_counts)
    print("C=%d metrics: max relative error %.3e" % (C, np.max(np.abs(got[3] - want_metrics) / np.maximum(want_metrics, 1e-30))))
    np.testing.assert_allclose(got[3], want_metrics, rtol=RTOL, atol=0)
    assert (got[3][4] == 0).all() and (got[3][5] == 0).all() and (got[2][5] == 0).all()             # no positive; nothing at all
    assert got[2][3].tolist() == [C, 0, 0] and got[2][4].tolist() == [0, C, 0]
    # a second run gives the same bits
    r2, o2, c2, m2 = new((B, C), torch.int32), new((B, C), torch.int32), new((B, 3), torch.int32), new((B, 3), torch.float32)
    assert call(kt, r2, o2, c2, m2) == 0
    torch.cuda.synchronize()
    for a, b in zip(got, (r2, o2, c2, m2)):
        assert a.tobytes() == b.cpu().numpy().tobytes()
    # NULL clicked: ranks only (the same ranks: clicked never enters the order)
    r3, o3 = new((B, C), torch.int32), new((B, C), torch.int32)
    assert call(None, r3, o3, None, None) == 0
    # NULL rank_of / order: the counts and metrics alone, and either one alone
    c4, m4, r5, o6 = new((B, 3), torch.int32), new((B, 3), torch.float32), new((B, C), torch.int32), new((B, C), torch.int32)
    assert call(kt, None, None, c4, m4) == 0 and call(kt, r5, None, None, None) == 0 and call(None, None, o6, None, None) == 0
    torch.cuda.synchronize()
    assert (r3.cpu().numpy() == want_rank).all() and (o3.cpu().numpy() == want_order).all()
    assert (c4.cpu().numpy() == want_counts).all() and m4.cpu().numpy().tobytes() == got[3].tobytes()
    assert (r5.cpu().numpy() == want_rank).all() and (o6.cpu().numpy() == want_order).all()
