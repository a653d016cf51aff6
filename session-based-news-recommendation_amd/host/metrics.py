"""Ranking / diversity metrics of the evaluation loop (util.py:8-18, model_combine.py:174-194,301-313).

The GPU path returns, per session, the label's rank and the top-k indices (kernel `tcar_rank_topk`), so the
host never sees the [B,N] score matrix; the functions here turn ranks / top-k lists into the numbers the
reference prints.  `cau_metrics` keeps the reference signature for callers that do hold score rows.
"""
from __future__ import annotations

import numpy as np


def metrics_from_ranks(ranks: np.ndarray, cutoff: int = 20):
    """ranks are 1-based.  Returns (hit, mrr, ndcg) arrays, element-wise as util.py:15-17."""
    ranks = np.asarray(ranks, dtype=np.int64)
    hit = ranks <= cutoff
    mrr = np.where(hit, 1.0 / ranks, 0.0)
    ndcg = np.where(hit, 1.0 / np.log2(ranks + 1.0), 0.0)
    return hit, mrr, ndcg


def list_ranks(topk, labels, cutoff: int = 20) -> np.ndarray:
    """The 1-based place of every label in its OWN list (topk [B, k], 0-based ids, -1 = no entry), cutoff + 1 where the list's first
    `cutoff` entries do not hold it: what metrics_from_ranks turns into the accuracy of the lists themselves."""
    topk = np.asarray(topk)[:, :cutoff]
    eq = topk == np.asarray(labels, dtype=np.int64)[:, None]
    return np.where(eq.any(1), eq.argmax(1) + 1, cutoff + 1).astype(np.int64)


def largest_categories(cat, G: int) -> np.ndarray:
    """The G category codes that the most items of the table `cat` [N] carry, the largest first; of two categories of one size the
    smaller code comes first.  Fewer than G codes in the table: all of them.  What test() lists as sections (eval_sections)."""
    codes, counts = np.unique(np.asarray(cat).reshape(-1), return_counts=True)        # codes ascending
    order = np.argsort(-counts, kind="stable")                                        # stable: ties keep the ascending codes
    return codes[order][:G].astype(np.int64)


def section_hits(topk, labels, cat, sections):
    """Sectioned lists topk [B, G, k] (0-based ids, -1 = no entry; list g holds items of category sections[g]) against the labels
    [B] -> (hit [B] bool: the label is in the list of ITS OWN section, covered [B] bool: the label's category is a listed section).
    Recall in the label's section = hit.sum() / covered.sum()."""
    topk, labels = np.asarray(topk), np.asarray(labels, dtype=np.int64).reshape(-1)
    mine = np.asarray(cat)[labels][:, None] == np.asarray(sections, dtype=np.int64)[None, :]       # [B, G], at most one per row
    covered = mine.any(1)
    own = topk[np.arange(len(labels)), mine.argmax(1)]                                             # [B, k] (row 0's where uncovered)
    return covered & (own == labels[:, None]).any(1), covered


def related_sums(topk, sims, ids, cat):
    """Related lists topk [Q, k] (0-based ids, -1 = no entry) with their cosines sims [Q, k] of the articles ids [Q] -> (the sum
    of the listed cosines in double precision, the number of listed items of their article's own category).  Divide both by
    (topk >= 0).sum(): mean cosine, same-category share."""
    topk, cat = np.asarray(topk), np.asarray(cat)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    listed = topk >= 0
    same = listed & (cat[np.where(listed, topk, 0)] == cat[ids][:, None])
    return float(np.asarray(sims, dtype=np.float64)[listed].sum()), float(same.sum())


def duplicate_groups(partner):
    """The partner array of a duplicate audit (engine.TcarEngine.find_duplicates: partner[i] = the item most similar to i among those
    at or above the threshold, -1 = none) -> the groups of size >= 2, each a sorted list of ids, ordered by their first id: a
    union-find over the edges i -- partner[i].  These are BEST-PARTNER clusters: every item is joined to its one best partner only,
    so a group is a subset of a connected component of the threshold graph (two items above the threshold of each other whose best
    partners lie elsewhere may fall into different groups).  similar_items(ids of a group) lists every partner."""
    partner = np.asarray(partner, dtype=np.int64).reshape(-1)
    root = np.arange(partner.size)

    def find(i):
        while root[i] != i:
            root[i] = root[root[i]]
            i = root[i]
        return i

    for i in np.flatnonzero(partner >= 0).tolist():
        a, b = find(i), find(int(partner[i]))
        if a != b:
            root[max(a, b)] = min(a, b)
    groups = {}
    for i in np.flatnonzero(partner >= 0).tolist():
        for j in (i, int(partner[i])):
            groups.setdefault(find(j), set()).add(j)
    return [sorted(g) for _, g in sorted(groups.items())]


def cau_metrics(preds, labels, cutoff=20):
    """Same contract as util.py:8-18: rank = 1 + #{j: preds[j] > preds[label]} (strict)."""
    preds = np.asarray(preds)
    labels = np.asarray(labels, dtype=np.int64)
    if preds.ndim == 1:
        preds = preds[None, :]
    lab = preds[np.arange(len(labels)), labels]
    ranks = (preds > lab[:, None]).sum(1) + 1
    hit, mrr, ndcg = metrics_from_ranks(ranks, cutoff)
    return hit.tolist(), mrr.tolist(), ndcg.tolist()


def ild_batch(topk: np.ndarray, cat_of_item: np.ndarray) -> np.ndarray:
    """model_combine.py:174-182 for a [B,k] array of 0-based item ids: share of ordered pairs (i != j) whose
    categories differ."""
    c = cat_of_item[topk]                                     # [B,k]
    k = c.shape[1]
    diff = (c[:, :, None] != c[:, None, :]).sum((1, 2))       # the diagonal never differs
    return diff / float(k * (k - 1))


def content_ild_batch(topk, content) -> np.ndarray:
    """Intra-list distance over CONTENT: for every list of topk [B, k] (0-based ids, -1 = no entry) the mean of 1 - cos(x_i, x_j) over
    the ordered pairs (i != j) of its entries, x_n = content[n] (float [N, H]); an all-zero row has cosine 0 with everything.  NaN
    for a list of fewer than 2 entries.  float64 [B].  The content twin of ild_batch, which compares category labels."""
    topk = np.asarray(topk)
    x = np.asarray(content, dtype=np.float64)
    norm = np.sqrt((x * x).sum(1))
    x = x * np.where(norm > 0, 1.0 / np.where(norm > 0, norm, 1.0), 0.0)[:, None]
    out = np.full(topk.shape[0], np.nan)
    for b, row in enumerate(topk):
        ids = row[row >= 0]
        n = len(ids)
        if n >= 2:
            cos = x[ids] @ x[ids].T
            out[b] = ((n * (n - 1)) - (cos.sum() - np.trace(cos))) / float(n * (n - 1))
    return out


def unexp_batch(seq: np.ndarray, topk: np.ndarray, cat_of_item: np.ndarray) -> np.ndarray:
    """model_combine.py:184-194: share of (recommended, input) pairs with different category; `seq` holds
    1-based ids."""
    cr = cat_of_item[topk]                                    # [B,k]
    ci = cat_of_item[np.asarray(seq) - 1]                     # [B,T]
    diff = (cr[:, :, None] != ci[:, None, :]).sum((1, 2))
    return diff / float(cr.shape[1] * ci.shape[1])


def diversity_from_counts(ild_cnt, unexp_cnt, n_rec, T: int):
    """The divisions of getILD / getUnexp (model_combine.py:182,194) on the integer pair counts the device kernel
    tcar_eval_diversity returns: score / (n (n - 1)) and score / (n len(inSeq)) — Python int / int, i.e. double precision."""
    ild_cnt = np.asarray(ild_cnt, dtype=np.int64)
    unexp_cnt = np.asarray(unexp_cnt, dtype=np.int64)
    n = np.asarray(n_rec, dtype=np.int64)
    if n.size and int(n.min()) <= 1:
        # getILD divides by n (n - 1) unguarded (model_combine.py:182): a recommendation list of 0 or 1 items raises there, and here
        raise ZeroDivisionError("getILD: a recommendation list of %d item(s) (model_combine.py:182 divides by n (n - 1))" % int(n.min()))
    ild = ild_cnt / (n * (n - 1)).astype(np.float64)
    unexp = np.where(n > 0, unexp_cnt / np.maximum(n * int(T), 1).astype(np.float64), 0.0)      # getUnexp returns 0 for n == 0
    return ild, unexp


def impression_metrics(counts, metrics):
    """Per-session impression metrics from what TcarEngine.score_candidates returns with `clicked`: counts [B, 3] int = (npos, nneg,
    auc2) and metrics [B, 3] = (mrr, ndcg5, ndcg10) -> (auc, mrr, ndcg5, ndcg10), float64 arrays [B].  auc = auc2 / (2 npos nneg), the
    ROC AUC with ties at one half; it is NaN where a session has no positive or no negative — the usual rule for impressions without
    both classes — and `impression_means` drops such sessions from every mean."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1, 3)
    metrics = np.asarray(metrics, dtype=np.float64).reshape(-1, 3)
    pairs = counts[:, 0] * counts[:, 1]
    auc = np.where(pairs > 0, counts[:, 2] / np.maximum(2 * pairs, 1).astype(np.float64), np.nan)
    return auc, metrics[:, 0], metrics[:, 1], metrics[:, 2]


def impression_means(counts, metrics):
    """The four means of impression_metrics over the sessions that hold both classes -> {"auc", "mrr", "ndcg5", "ndcg10", "sessions"};
    NaN means when no session qualifies."""
    auc, mrr, n5, n10 = impression_metrics(counts, metrics)
    keep = ~np.isnan(auc)
    mean = lambda x: float(x[keep].mean()) if keep.any() else float("nan")
    return {"auc": mean(auc), "mrr": mean(mrr), "ndcg5": mean(n5), "ndcg10": mean(n10), "sessions": int(keep.sum())}


def category_table(reverse_item: dict, category_id, n_items: int) -> np.ndarray:
    """int table cat[item0] = code of category_id[reverse_item[item0]] (the double lookup of model_combine.py:180).
    The reference only ever compares categories with `!=`, so any label type works (MIND's categories are strings): the
    labels are factorised to integer codes.  Items without a category (the reference raises KeyError lazily, when such an
    item is first recommended) get one code of their own each, i.e. they differ from everything else."""
    labels, missing = [], []
    for i in range(n_items):
        orig = reverse_item.get(i) if hasattr(reverse_item, "get") else reverse_item[i]
        if orig is not None and orig in category_id:
            labels.append(category_id[orig])
        else:
            labels.append(None)
            missing.append(i)
    if missing:
        # the reference would raise KeyError the first time one of these is recommended (model_combine.py:180): say once that
        # ILD / unexp are computed on a fold where the reference's evaluation could fail
        import sys
        print("[tcar] %d of %d catalog items have no category: each counts as a category of its own in ILD / unexp "
              "(the reference raises KeyError when one is recommended)" % (len(missing), n_items), file=sys.stderr)
    out = np.empty(n_items, dtype=np.int64)
    known = [l for l in labels if l is not None]
    codes = {}
    for l in known:
        if l not in codes:
            codes[l] = len(codes)
    nxt = len(codes)
    for i, l in enumerate(labels):
        if l is None:
            out[i] = nxt
            nxt += 1
        else:
            out[i] = codes[l]
    return out
