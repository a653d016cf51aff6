"""Inputs that the tests of related items share (test_gpu_similar_panel.py, test_gpu_similar_serve.py): the exact content rows of
tests/test_gpu_mmr_walk.py (restated: a test file is nobody's library), a table inside a wider device matrix, and the planted
catalog on which fp64 decides every list."""
import numpy as np
import torch


def exact_content(rng, N, H):
    """`_exact_content` of test_gpu_mmr_walk.py, draw for draw: [N, H], four entries of 0.5 per row, on columns of one of a few runs
    of seven (the last run ends at H - 1: the partial chunk); item 0 is all zero.  Every norm is exactly 1 and every cosine is in
    {0, 1/4, 1/2, 3/4, 1} in ANY summation order.  H >= 4."""
    runs = [0] if H < 14 else [0, H // 4, H // 2, H - 7]
    x = np.zeros((N, H), np.float32)
    for n in range(1, N):
        x[n, runs[rng.randint(len(runs))] + rng.choice(min(7, H), 4, replace=False)] = 0.5
    return x


def padded(x, extra, fill, lead=0):
    """x [R, n] inside a wider device matrix [R, lead + n + extra], `fill` around it -> (matrix, leading dimension)"""
    t = torch.full((x.shape[0], lead + x.shape[1] + extra), fill, dtype=torch.from_numpy(x).dtype)
    t[:, lead:lead + x.shape[1]] = torch.from_numpy(x)
    return t.cuda(), lead + x.shape[1] + extra


# ---- the planted catalog: N = 3,000 rows of H = 250 columns, 32 queries with 24 planted neighbours each
P_N, P_H, P_Q, P_NEIGH = 3000, 250, 32, 24
_PLANTED = {}


def planted():
    """Query q is row q.  Its neighbour j (j = 0 .. 23) is row 100 + 24 q + j = s (c u_q + sqrt(1 - c^2) v) with c = 0.95 - 0.02 j,
    u_q the unit vector of the query, v a random unit vector orthogonal to u_q and s a random norm in [0.5, 2.5]: its cosine with the
    query is c up to the rounding of the fp32 row.  Every other row is random normal (cosines of about 1 / sqrt(250) = 0.06 with
    anything).  -> (content [N, H] fp32, query ids [Q]); computed once, shared, never written."""
    if not _PLANTED:
        rng = np.random.RandomState(41)
        x = rng.standard_normal((P_N, P_H))
        for q in range(P_Q):
            u = x[q] / np.sqrt(x[q] @ x[q])
            for j in range(P_NEIGH):
                v = rng.standard_normal(P_H)
                v -= (v @ u) * u
                v /= np.sqrt(v @ v)
                c = 0.95 - 0.02 * j
                x[100 + P_NEIGH * q + j] = rng.uniform(0.5, 2.5) * (c * u + np.sqrt(1 - c * c) * v)
        content = x.astype(np.float32)
        content.setflags(write=False)
        _PLANTED.update(content=content, ids=np.arange(P_Q, dtype=np.int32))
    return _PLANTED["content"], _PLANTED["ids"]
