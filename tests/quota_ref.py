"""The numpy model of a capped list (include/tcar_quota.h), shared by the quota tests."""
import numpy as np


def capped_walk(scores, cat, k, m, eligible=None):
    """Walk the eligible items of one session in list order — score descending, then item id descending — and take an item iff fewer
    than m items of its category have been taken; stop at k.  Returns the ids taken, in the order they were (at most k of them)."""
    scores, cat = np.asarray(scores), np.asarray(cat)
    ids = np.arange(scores.shape[0]) if eligible is None else np.where(np.asarray(eligible, dtype=bool))[0]
    order = ids[np.argsort(scores[ids], kind="stable")[::-1]]         # ascending ids, stable, reversed: ties by id descending
    c = cat[order]
    by_cat = np.argsort(c, kind="stable")                             # within a category: walk order
    cs = c[by_cat]
    start = np.r_[0, np.where(cs[1:] != cs[:-1])[0] + 1] if len(cs) else np.zeros(0, np.int64)
    size = np.diff(np.r_[start, len(cs)])
    nth = np.empty(len(cs), np.int64)                                 # how many of its category walk in front of an item
    nth[by_cat] = np.arange(len(cs)) - np.repeat(start, size)
    return [int(i) for i in order[nth < m][:k]]
