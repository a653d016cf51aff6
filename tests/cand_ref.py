"""The numpy model of candidate-list scoring (include/tcar_cand.h) that the host and GPU tests share: the list order through
np.lexsort, the metrics through plain loops in fp64, and the KB32 image of a bf16 plane (csrc/tcar_bf16_layout.h)."""
import numpy as np


def rank_model(score, cand, clicked=None):
    """score [B, C] float, cand [B, C] int, clicked [B, C] 0 / 1 or None -> (rank_of [B, C] int32, order [B, C] int32, counts [B, 3]
    int64, metrics [B, 3] float64); counts and metrics are None without clicked.  A slot is empty iff its id is negative or its score
    is -inf.  Order: score descending, item id descending, slot ascending."""
    score, cand = np.asarray(score), np.asarray(cand)
    B, C = cand.shape
    rank_of, order = np.zeros((B, C), np.int32), np.full((B, C), -1, np.int32)
    counts, metrics = np.zeros((B, 3), np.int64), np.zeros((B, 3), np.float64)
    for b in range(B):
        slots = np.where((cand[b] >= 0) & (score[b] != -np.inf))[0]
        s, ids = score[b][slots].astype(np.float64), cand[b][slots].astype(np.int64)
        by = slots[np.lexsort((slots, -ids, -s))]                # the LAST key is the primary one
        for r, slot in enumerate(by):
            rank_of[b, slot], order[b, r] = r + 1, slot
        if clicked is None:
            continue
        pos = [int(x) for x in slots if clicked[b, x]]
        neg = np.sort(np.asarray([score[b, x] for x in slots if not clicked[b, x]], dtype=np.float64))
        auc2 = 0
        for p in pos:                                            # negatives strictly below count 2, ties 1
            below, upto = np.searchsorted(neg, score[b, p], "left"), np.searchsorted(neg, score[b, p], "right")
            auc2 += 2 * int(below) + int(upto - below)
        counts[b] = len(pos), len(neg), auc2
        if pos:
            metrics[b, 0] = sum(1.0 / rank_of[b, p] for p in pos) / len(pos)
            for col, k in ((1, 5), (2, 10)):
                dcg = sum(1.0 / np.log2(1.0 + rank_of[b, p]) for p in pos if rank_of[b, p] <= k)
                metrics[b, col] = dcg / sum(1.0 / np.log2(1.0 + i) for i in range(1, min(len(pos), k) + 1))
    return (rank_of, order, counts, metrics) if clicked is not None else (rank_of, order, None, None)


def auc2_brute(score, cand, clicked):
    """the pair loop: sum over (positive, negative) of 2 [s_p > s_n] + [s_p == s_n] among the non-empty slots of every row"""
    out = []
    for b in range(len(cand)):
        live = [c for c in range(cand.shape[1]) if cand[b, c] >= 0 and score[b, c] != -np.inf]
        out.append(sum(2 * (score[b, p] > score[b, n]) + (score[b, p] == score[b, n])
                       for p in live if clicked[b, p] for n in live if not clicked[b, n]))
    return np.asarray(out, dtype=np.int64)


def bf16_values(rng, shape, scale):
    """random floats that a bf16 holds exactly (fp32 with the low 16 bits cleared)"""
    x = (rng.standard_normal(shape) * scale).astype(np.float32)
    return (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def kb32_plane(x, fill_from=None):
    """The KB32 image of x [rows, inner] (fp32 values a bf16 holds exactly; inner % 32 == 0): uint16 [ceil128(rows) * inner], padding rows
    zero.  Columns >= fill_from hold a bf16 NaN (what a kernel must never read as a score)."""
    rows, inner = x.shape
    assert inner % 32 == 0
    bits = (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)
    if fill_from is not None:
        bits[:, fill_from:] = 0x7FC0
    out = np.zeros((rows + 127) // 128 * 128 * inner, np.uint16)
    r, k = np.meshgrid(np.arange(rows), np.arange(inner), indexing="ij")
    rr, kk = r & 127, k & 31
    off = ((r >> 7) * (inner // 32) + (k >> 5)) * 4096 + rr * 32 + ((((kk >> 3) ^ ((rr >> 2) & 3)) << 3) | (kk & 7))
    out[off] = bits
    return out
