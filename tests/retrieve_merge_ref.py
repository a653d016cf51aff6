"""The numpy restatement of the shortlist merge (include/tcar_retrieve_shard.h: tcar_retrieve_merge) that the host and GPU tests share.

A shortlist is (ids [B, C'] int32, scores [B, C'] fp32) in the list order of tests/retrieve_ref.py — score descending, then item id
descending; -0.0 and +0.0 are equal scores — with -1 / -inf behind its last entry.  The merge of several lists over DISJOINT items is
the first C entries of their union under the same order; scores keep their own bits."""
import numpy as np


def merge_shortlists(lists, C):
    """lists: a sequence of (ids [B, C_s], scores [B, C_s]) -> (ids [B, C] int32, scores [B, C] fp32)"""
    lists = [(np.asarray(i, np.int32), np.asarray(s, np.float32)) for i, s in lists]
    B = lists[0][0].shape[0]
    ids = np.full((B, C), -1, np.int32)
    scores = np.full((B, C), -np.inf, np.float32)
    for b in range(B):
        i = np.concatenate([l[0][b] for l in lists])
        s = np.concatenate([l[1][b] for l in lists])
        live = i >= 0
        i, s = i[live], s[live]
        assert len(set(i.tolist())) == len(i), "the lists of one session name disjoint items"
        order = np.lexsort((i, s))[::-1][:C]            # (lexsort compares floats: the two zeros tie and the id decides)
        ids[b, :len(order)] = i[order]
        scores[b, :len(order)] = s[order]
    return ids, scores
