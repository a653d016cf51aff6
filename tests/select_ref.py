"""The numpy model of the streamed selection, shared by its tests: the capped list (include/tcar_quota.h), a select state and the merge of
S states (include/tcar_serve_shard.h).

A state is a dict: ids / scores (the list, at most k entries, in list order: score descending, then item id descending), count (scores of
the pool strictly above the label's, the label itself left out), m / s (max and sum exp(x - m) over the pool, fp64; m = -inf, s = 0
where nothing was folded)."""
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


def _walk(ids, scores, k, cat, cap):
    """the (capped) walk over entries (ids, scores) in list order -> positions taken; ids need not be sorted, ties go by id descending"""
    ids, scores = np.asarray(ids, dtype=np.int64), np.asarray(scores)
    by_id = np.argsort(ids, kind="stable")              # capped_walk breaks ties by POSITION descending: make position order id order
    if cat is not None and cap is not None and cap < k:
        took = capped_walk(scores[by_id], np.asarray(cat)[ids[by_id]], k, cap)
    else:
        took = capped_walk(scores[by_id], np.arange(len(ids)), k, 1)       # every entry its own category: the plain k best
    return by_id[np.asarray(took, dtype=np.int64)]


def fold_state(ids, scores, k, label=None, lab_score=None, pool=None, excl=(), cat=None, cap=None):
    """the state one fold of the items `ids` (global ids) with fp32 `scores` leaves.  pool: bool per item (None: all; the label of a
    labelled call is always in it); excl: ids that never enter the list; cat (indexed by global id) / cap: the capped walk."""
    ids, scores = np.asarray(ids, dtype=np.int64), np.asarray(scores, dtype=np.float32)
    pool = np.ones(len(ids), bool) if pool is None else np.asarray(pool, dtype=bool).copy()
    if lab_score is not None:
        pool |= ids == label
    x = scores[pool].astype(np.float64)
    count = int(((scores > np.float32(lab_score)) & pool & (ids != label)).sum()) if lab_score is not None else 0
    m = float(x.max()) if x.size else -np.inf
    s = float(np.exp(x - m).sum()) if x.size else 0.0
    ok = np.where(pool & ~np.isin(ids, np.asarray(list(excl), dtype=np.int64)))[0]
    took = ok[_walk(ids[ok], scores[ok], k, cat, cap)] if ok.size else np.zeros(0, np.int64)
    return {"ids": ids[took].tolist(), "scores": scores[took].copy(), "count": count, "m": m, "s": s}


def merge_states(states, k, cat=None, cap=None):
    """tcar_select_merge: the walk over the union of the lists, the summed count, the softmax pair in shard order"""
    ids = np.concatenate([np.asarray(st["ids"], dtype=np.int64) for st in states])
    scores = np.concatenate([np.asarray(st["scores"], dtype=np.float32) for st in states])
    took = _walk(ids, scores, k, cat, cap) if ids.size else np.zeros(0, np.int64)
    M = max(st["m"] for st in states)
    s = 0.0
    for st in states:                                   # ascending shard order; a state that folded nothing adds nothing
        if st["m"] > -np.inf:
            s += st["s"] * np.exp(st["m"] - M)
    return {"ids": ids[took].tolist(), "scores": scores[took].copy(), "count": sum(st["count"] for st in states), "m": M, "s": s}


def finish(st, k, lab_score=None):
    """tcar_select_finish: (topk padded with -1, rank, ce)"""
    topk = st["ids"] + [-1] * (k - len(st["ids"]))
    if lab_score is None:
        return topk, None, None
    return topk, 1 + st["count"], st["m"] + np.log(st["s"]) - float(lab_score)


def pack_states(states, k):
    """states of B sessions -> the int32 words [B, 2k + 4] of tcar_serve.h (softmax pair rounded to fp32)"""
    out = np.zeros((len(states), 2 * k + 4), np.int32)
    f = out.view(np.float32)
    for b, st in enumerate(states):
        n = len(st["ids"])
        f[b, :k] = -np.inf
        f[b, :n] = st["scores"]
        out[b, k:2 * k] = -1
        out[b, k:k + n] = st["ids"]
        out[b, 2 * k] = st["count"]
        f[b, 2 * k + 1], f[b, 2 * k + 2] = st["m"], st["s"]
    return out
