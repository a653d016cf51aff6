"""The numpy restatement of the streamed top-C selector (include/tcar_retrieve.h) that the host and GPU tests share.

A row's shortlist is its eligible, non-NaN entries in the library's list order — score descending, then item id descending; -0.0 and
+0.0 are equal scores — cut to the first C and padded with -1 / -inf.  `np.lexsort` with the id as the secondary and the score as the
primary key sorts ascending in both; the list order is that sequence reversed."""
import numpy as np


def eligible_mask(N, b, excl=None, key=None, lo=None, hi=None):
    """items of [0, N) that session b may list: not in excl[b] (-1 and ids outside the catalog name nothing), inside its window"""
    ok = np.ones(N, bool)
    if excl is not None:
        e = np.asarray(excl[b], np.int64)
        ok[e[(e >= 0) & (e < N)]] = False
    if key is not None:
        ok &= (np.int64(lo[b]) <= key.astype(np.int64)) & (key.astype(np.int64) < np.int64(hi[b]))
    return ok


def shortlist(x, C, excl=None, key=None, lo=None, hi=None):
    """x [B, N] fp32 -> (ids [B, C] int32, scores [B, C] fp32): scores are x's own bits"""
    x = np.asarray(x, np.float32)
    B, N = x.shape
    ids = np.full((B, C), -1, np.int32)
    scores = np.full((B, C), -np.inf, np.float32)
    for b in range(B):
        items = np.where(eligible_mask(N, b, excl, key, lo, hi) & ~np.isnan(x[b]))[0]
        order = items[np.lexsort((items, x[b, items]))][::-1][:C]
        ids[b, :len(order)] = order
        scores[b, :len(order)] = x[b, order]
    return ids, scores


def shortlist_brute(x, C, excl=None, key=None, lo=None, hi=None):
    """the same lists by repeated arg-max under an explicit comparison of (score, id) pairs: O(N C), for tiny inputs"""
    x = np.asarray(x, np.float32)
    B, N = x.shape
    ids = np.full((B, C), -1, np.int32)
    scores = np.full((B, C), -np.inf, np.float32)
    for b in range(B):
        ok = eligible_mask(N, b, excl, key, lo, hi)
        left = [n for n in range(N) if ok[n] and not x[b, n] != x[b, n]]
        for r in range(C):
            if not left:
                break
            best = left[0]
            for n in left[1:]:
                if x[b, n] > x[b, best] or (x[b, n] == x[b, best] and n > best):
                    best = n
            ids[b, r], scores[b, r] = best, x[b, best]
            left.remove(best)
    return ids, scores
