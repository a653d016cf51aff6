"""The numpy model of related items (include/tcar_similar.h) that the host and the GPU tests share.

sims_f32 follows the definition in fp32, operation for operation: every dot through mmr_ref.dots_f32 (the eight chains and their close),
r = 1 / sqrt(x . x) with correctly rounded sqrt and division (0 for an all-zero row), sim = dot * (r_q * r_n).  As in mmr_ref there is
ONE difference to the kernels: they fuse each multiply-add of a dot and numpy rounds the product first, so the two agree bit for bit
where every product and partial sum is exact — the exact-arithmetic cases — and within TOL_SIM = (H + 8) 2^-24 elsewhere.
sims_f64 is the cosine straight from the definition in fp64.  lists() turns a [Q, N] block of scores into the lists of the library
through select_ref (score descending, then item id descending; exclusions, pools, per-category caps)."""
import numpy as np

from mmr_ref import dots_f32
from select_ref import finish, fold_state


def tol_sim(H):
    """the bound of tests/test_gpu_mmr_walk.py on one similarity: H roundings of a dot of rows with |x^| |y^| <= 1, eight for the
    normalisation"""
    return (H + 8) * 2.0 ** -24


def rnorm_f32(X):
    """r of every row of X [P, H] in fp32: 1 / sqrt(x . x), the dot in the kernel's order; 0 for an all-zero row"""
    X = np.asarray(X, dtype=np.float32)
    ss = np.array([dots_f32(X[p:p + 1], X[p])[0] for p in range(X.shape[0])], np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.float32(1) / np.sqrt(ss, dtype=np.float32)
    return np.where(ss > 0, r, np.float32(0)).astype(np.float32)


def query_rows(content, ids):
    """the rows the prologue gathers: content[id], a zero row for an id outside [0, N)"""
    content, ids = np.asarray(content, dtype=np.float32), np.asarray(ids, dtype=np.int64)
    ok = (ids >= 0) & (ids < content.shape[0])
    return np.where(ok[:, None], content[np.where(ok, ids, 0)], np.float32(0)).astype(np.float32)


def sims_f32(Xq, Y):
    """[Q, n] fp32: sim(query row q, item row j) = dot * (r_q * r_j)"""
    Xq, Y = np.asarray(Xq, dtype=np.float32), np.asarray(Y, dtype=np.float32)
    rq, ry = rnorm_f32(Xq), rnorm_f32(Y)
    out = np.empty((Xq.shape[0], Y.shape[0]), np.float32)
    for q in range(Xq.shape[0]):
        out[q] = dots_f32(Y, Xq[q]) * (rq[q] * ry)
    return out


def sims_f64(Xq, Y):
    """[Q, n] fp64 cosines from the definition; 0 where either row is all zero"""
    Xq, Y = np.asarray(Xq, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    nq, ny = np.sqrt((Xq * Xq).sum(1)), np.sqrt((Y * Y).sum(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (Xq @ Y.T) / (nq[:, None] * ny[None, :])
    return np.where((nq[:, None] > 0) & (ny[None, :] > 0), s, 0.0)


def lists(S, k, excl=None, pool=None, cat=None, cap=None, fill=0.0):
    """S [Q, N] fp32 scores of the items 0 .. N - 1 -> (topk [Q, k] int32, -1 behind the last entry; score [Q, k] fp32, `fill` there).
    excl: per query a sequence of ids that never enter its list; pool [Q, N] bool: the items of its window; cat [N] / cap: the capped
    walk of include/tcar_quota.h."""
    S = np.asarray(S, dtype=np.float32)
    Q, N = S.shape
    topk, score = np.full((Q, k), -1, np.int32), np.full((Q, k), fill, np.float32)
    for q in range(Q):
        st = fold_state(np.arange(N), S[q], k, pool=None if pool is None else pool[q], excl=() if excl is None else excl[q], cat=cat,
                        cap=cap)
        topk[q] = finish(st, k)[0]
        score[q, :len(st["ids"])] = st["scores"]
    return topk, score
