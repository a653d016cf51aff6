"""The warm-start rule of include/tcar_warm.h, stated in fp64 numpy over given neighbour lists: what tcar_rows_blend is checked
against, and the bound that its arithmetic — k fmas, a k-term sum, one division, all fp32 — cannot exceed.  The weights are decided
on the fp32 values the kernel sees (s > 0, s >= min_sim are comparisons of fp32 numbers); every sum is exact to fp64."""
import numpy as np

EPS = 2.0 ** -24


def blend(nbr, sim, table, min_sim=0.0):
    """nbr int [U, k], sim fp32 [U, k], table [N, H] -> (rows fp64 [U, H], support int [U], wsum fp64 [U], scale fp64 [U, H]):
    scale[u, c] = max |table[n_j, c]| over the donors of u with a weight > 0 (0 without one), the factor of the bound"""
    nbr, sim = np.asarray(nbr, dtype=np.int64), np.asarray(sim, dtype=np.float32)
    table = np.asarray(table, dtype=np.float64)
    N, H = table.shape
    U, k = nbr.shape
    assert sim.shape == (U, k) and 1 <= k <= 64
    ms = np.float32(min_sim)
    rows, scale = np.zeros((U, H)), np.zeros((U, H))
    support, wsum = np.zeros(U, np.int32), np.zeros(U)
    for u in range(U):
        acc, W = np.zeros(H), 0.0
        for j in range(k):                                           # j ascending, as the rule says
            n, s = int(nbr[u, j]), sim[u, j]
            if not (0 <= n < N and s > 0 and s >= ms):               # (a NaN s fails s > 0)
                continue
            acc += float(s) * table[n]
            W += float(s)
            support[u] += 1
            scale[u] = np.maximum(scale[u], np.abs(table[n]))
        if support[u]:
            rows[u], wsum[u] = acc / W, W
    return rows, support, wsum, scale


def bound(k, scale):
    """|row - ref| <= (2 k + 2) 2^-24 max_j |x_nj[c]|: each of the k fmas and of the k adds of W rounds once (relative 2^-24 of a
    partial sum that never exceeds W max|x| resp. W), the division once, and the first-order terms add to 2 k + 1; + 1 for the
    second-order remainder at k <= 64"""
    return (2 * k + 2) * EPS * np.asarray(scale, dtype=np.float64)


def check_rows(got, nbr, sim, table, min_sim=0.0, name=""):
    """assert the kernel's rows (fp32 [U, H]) against the reference within the bound; returns (worst error / bound, reference)"""
    ref, support, wsum, scale = blend(nbr, sim, table, min_sim)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err, lim = np.abs(got - ref), bound(np.asarray(nbr).shape[1], scale)
    worst = float((err / np.maximum(lim, 1e-300)).max()) if err.size else 0.0
    print("%s: worst error / bound = %.3f" % (name, worst))
    bad = err > lim
    assert not bad.any(), "%s: %d / %d entries beyond (2k + 2) 2^-24 max|x|, worst %.3e at %s" % (
        name, int(bad.sum()), bad.size, float(err.max()), np.unravel_index(err.argmax(), err.shape))
    return worst, (ref, support, wsum)
