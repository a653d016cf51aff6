"""What the tests of ragged batches (include/tcar_ragged.h) share: the two length mixes, a mixed batch at the shape of
serve_case.reference() as a ragged feed, and the fp64 oracle's scores of it — eval_batch per length group, the rows put back in
session order.  Computed once, shared, never written."""
import numpy as np

from serve_case import B, N, reference

SET = (1, 2, 3, 4, 5, 7, 8, 40)
# 41 sessions: T = 1; below, at and above the four register-cached positions; odd lengths against the 2- and 4-position trips; the
# whole 40-row position table.  The first and the last session differ, and the waves of EVERY workgroup (sessions 4 i .. 4 i + 3)
# hold four different lengths.  R = 353 <= 1,024: the projections run in their slab form.
MIX_SMALL = np.array(list(SET) * 5 + [3], np.int32)
# 26 sessions of length 40 among 15 short ones: R = 1,101 > 1,024, the projections run un-split
MIX_LONG = np.array([1, 40, 2, 40, 3, 40, 4, 40, 5, 40, 7, 40, 8, 40, 1, 40, 2, 40, 3, 40, 4, 40, 5, 40, 7, 40, 8, 40, 1, 40] + [40] * 11,
                    np.int32)
assert len(MIX_SMALL) == B and len(MIX_LONG) == B and (MIX_LONG == 40).sum() == 26
assert MIX_SMALL.sum() <= 1024 < MIX_LONG.sum() and set(MIX_SMALL.tolist()) == set(SET)

PER_ROW = ("seq", "pm", "pd", "pw", "ph", "pmi", "gap")


def offsets(lens):
    """off [B + 1] and pos [R] by a plain loop"""
    off, pos = [0], []
    for n in lens:
        off.append(off[-1] + int(n))
        pos += list(range(int(n)))
    return np.array(off, np.int32), np.array(pos, np.int32)


def random_ragged(lens, seed):
    """a labelled ragged feed of random ids in the reference's ranges"""
    rng = np.random.RandomState(seed)
    b, r = len(lens), int(np.sum(lens))
    f = {"seq": rng.randint(1, N + 1, r), "label": rng.randint(0, N, b), "pm": rng.randint(1, 13, r), "pd": rng.randint(1, 32, r),
         "pw": rng.randint(1, 8, r), "ph": rng.randint(1, 25, r), "pmi": rng.randint(1, 61, r), "cw": rng.randint(0, 7, b),
         "ch": rng.randint(0, 24, b), "gap": rng.randint(0, 12, r)}
    f = {k: v.astype(np.int32) for k, v in f.items()}
    f["len"] = np.asarray(lens, np.int32).copy()
    return f


def group(feed, length):
    """(the sessions of `feed` with this length, their rectangular feed [B_L, L])"""
    lens = feed["len"]
    off, _ = offsets(lens)
    idx = np.where(lens == length)[0]
    rows = (off[idx][:, None] + np.arange(length)[None, :]).astype(np.int64)
    sub = {k: feed[k][rows] for k in PER_ROW}
    sub.update({k: feed[k][idx] for k in ("cw", "ch", "label") if k in feed})
    return idx, sub


def permuted(feed, perm):
    """the ragged feed with its sessions in the order `perm`"""
    off, _ = offsets(feed["len"])
    rows = np.concatenate([np.arange(off[b], off[b + 1]) for b in perm]).astype(np.int64)
    out = {k: feed[k][rows] for k in PER_ROW}
    out.update({k: feed[k][perm] for k in ("cw", "ch", "label", "len") if k in feed})
    return out


def own_items(feed):
    """[B, max len]: the 0-based items of every session, -1 behind them"""
    off, _ = offsets(feed["len"])
    own = np.full((len(feed["len"]), int(feed["len"].max())), -1, np.int64)
    for b, n in enumerate(feed["len"]):
        own[b, :n] = feed["seq"][off[b]:off[b + 1]] - 1
    return own


_MIXED = {}


def mixed_reference(name):
    """the mixed batch `name` ("small" | "long") and the oracle's fp64 scores / CE of its sessions"""
    if name not in _MIXED:
        from oracle.tcar_oracle import TcarOracle
        r = reference()
        oracle = TcarOracle(r["params"], r["content"], r["mw"])
        lens = {"small": MIX_SMALL, "long": MIX_LONG}[name]
        feed = random_ragged(lens, 41 if name == "small" else 43)
        off, _ = offsets(lens)

        def scores():
            s, ce = np.zeros((B, N)), np.zeros(B)
            for length in sorted(set(lens.tolist())):
                idx, sub = group(feed, length)
                lg, c = oracle.eval_batch(sub)
                s[idx], ce[idx] = lg.numpy().astype(np.float64), c.numpy().astype(np.float64)
            return s, ce
        # Session 0 is the shortest (one item) and session 1 is longer: session 0's best item is put into session 1's LAST position, a
        # column of the [B, max len] exclusion lists that session 0 does not own.  Exclusion rows that are not -1 behind a session's own
        # items would drop it from session 0's list.  (Session 0's scores do not depend on session 1's items.)
        assert lens[0] == 1 and lens[1] > 1
        s, _ = scores()
        best = int(np.argsort(s[0])[-1])
        if best == feed["seq"][0] - 1:
            best = int(np.argsort(s[0])[-2])
        feed["seq"][off[2] - 1] = best + 1
        s, ce = scores()
        for a in list(feed.values()) + [s, ce]:
            a.setflags(write=False)
        _MIXED[name] = dict(feed=feed, s=s, ce=ce, delta=1e-3 * np.abs(s).max(1), best0=best)
    return _MIXED[name]
