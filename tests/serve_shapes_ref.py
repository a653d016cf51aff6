"""The serving calls at edge shapes (tests/test_gpu_serve_shapes.py, tests/test_serve_shapes_ref.py): the cases, the fp64 oracle's
references of them and the checkers that hold an engine's outputs against a reference.  Nothing here imports the GPU library: the
checkers take numpy arrays, so the CPU tests can hand them forged outputs and see them refused.

The gates are the project's, as tests/test_gpu_serve.py, test_gpu_cand_serve.py and test_gpu_retrieve_serve.py state them:
delta_b = 1e-3 * max_n |s[b, n]| (the logits gate) for lists, ranks and candidate ranks, `close` (1e-3 relative + 2e-5 of the scale)
for scores and cross entropies, and for a coarse score of a split-bf16 engine the band

    beta[b, n] = u * (|A| |E|^T)[b, n] + delta_b,        u = 2^-8,

with A the oracle's attout and E its candidate rows (item | content | clipped publish-time rows): the operands in fp64, so the band
owes nothing to the engine.  On an fp32 engine the coarse scores are its own scores and beta = delta_b.

Every checker notes its worst error / bound ratio in WORST before it asserts."""
from collections import OrderedDict, namedtuple

import numpy as np

from cand_ref import rank_model
from retrieve_ref import shortlist
from select_ref import finish, fold_state
from gpu_util import close

U = 2.0 ** -8
TOPK = 20
NEG = 3                                     # negatives per session: the training steps of phase B need some

Case = namedtuple("Case", "N H Ht B T panels seed emb_std w_std")
# panels: the `panel` arguments the streamed calls run with (None: the engine's default, one panel at these sizes)
CASES = OrderedDict([
    ("one",     Case(50, 12, 8, 1, 1, (None,), 71, 0.35, 0.12)),         # one session, one click, ek = 448, N < 128, k = 64 > N
    ("block+1", Case(129, 250, 64, 130, 3, (128,), 512, 0.35, 0.12)),    # the second panel holds ONE column; B = 128 + 2
    ("tile+1",  Case(1000, 250, 64, 513, 2, (128, None), 1765, 0.35, 0.12)),   # a one-row second M tile; eight panels, the last 104 wide
    ("long",    Case(1000, 40, 16, 3, 40, (256,), 1083, 0.35, 0.12)),    # T = 40; ek = 448 with plane offsets other than 0
    ("exact",   Case(768, 256, 64, 5, 3, (256,), 1032, 0.35, 0.12)),     # H = ldh, N = Npad = three whole panels
    ("wide",    Case(257, 300, 64, 33, 5, (256,), 595, 0.35, 0.12)),     # ldh = 320, ek = 960: H > 256; the last panel holds one column
])
SCORINGS = [(name, sc) for name in CASES for sc in (("f32", "bf16x3-mixed", "bf16x3") if name in ("block+1", "wide")
                                                    else ("f32", "bf16x3-mixed"))]
TRAINED = [(name, sc) for name in CASES for sc in ("f32", "bf16x3-mixed")]
PER_ROW = ("seq", "pm", "pd", "pw", "ph", "pmi", "gap")

WORST = {}


def note(what, ratio):
    WORST[what] = max(WORST.get(what, 0.0), float(ratio))


def shortlist_size(name):
    """C of retrieve / recommend_two_stage: min(128, Npad)"""
    return min(128, (CASES[name].N + 127) // 128 * 128)


# ------------------------------------------------------------------------------------------------------- inputs
_IN, _REF, _RAGGED, _TRAIN = {}, {}, {}, {}


def inputs(name):
    """(params, content, mw, batch) of a case: the content of `_case` of tests/step_cases.py.  Computed once, never written."""
    if name not in _IN:
        from oracle.tcar_oracle import init_params_numpy
        c = CASES[name]
        N, H, Ht, B, T = c.N, c.H, c.Ht, c.B, c.T
        rng = np.random.RandomState(c.seed)
        params = init_params_numpy(N, H, Ht, c.emb_std, c.w_std, rng)
        content = (rng.standard_normal((N + 1, H)) * 0.5).astype(np.float32)
        content[0] = 0
        mw = np.stack([rng.randint(1, 13, N), rng.randint(1, 32, N), rng.randint(1, 8, N), rng.randint(1, 25, N),
                       rng.randint(1, 61, N)], -1).astype(np.int32)
        b = {"seq": rng.randint(1, N + 1, (B, T)), "label": rng.randint(0, N, B), "pm": rng.randint(1, 13, (B, T)),
             "pd": rng.randint(1, 32, (B, T)), "pw": rng.randint(1, 8, (B, T)), "ph": rng.randint(1, 25, (B, T)),
             "pmi": rng.randint(1, 61, (B, T)), "cw": rng.randint(0, 7, B), "ch": rng.randint(0, 24, B),
             "gap": rng.randint(0, 12, (B, T)), "neg": rng.randint(0, N, (B, NEG))}
        b = {k: v.astype(np.int32) for k, v in b.items()}
        if T > 1:
            b["seq"][0, 1] = b["seq"][0, 0]            # a repeated item inside one session
        b["seq"][-1, 0] = b["seq"][0, 0]               # and across sessions
        for a in list(params.values()) + [content] + list(b.values()):
            a.setflags(write=False)
        _IN[name] = (params, content, mw, b)
    return _IN[name]


def unlabelled(feed):
    return {n: v for n, v in feed.items() if n not in ("label", "neg")}


def _forward(oracle, batch):
    """the oracle's fp64 scores of a rectangular batch and the operands of its scoring product"""
    import torch
    with torch.no_grad():
        out = oracle.forward(batch, with_neg=False)
        E = torch.cat([oracle.p["item_emb"][1:], oracle.content[1:], out["cand_pt"]], -1)
    s = out["logits"].numpy().astype(np.float64)
    A, E = out["attout"].numpy().astype(np.float64), E.numpy().astype(np.float64)
    return dict(s=s, ce=out["ce"].numpy().astype(np.float64), A=A, E=E, attout_t=out["attout"][:, -out["cand_pt"].shape[1]:].numpy())


def reference(name, params=None):
    """The oracle's view of a case: s [B, N] and ce [B] in fp64, delta [B], absdot = |A| |E|^T, the labels and the seen items.
    params None: the case's initial variables (computed once, shared); otherwise the variables given (phase B: the engine's own)."""
    if params is None and name in _REF:
        return _REF[name]
    from oracle.tcar_oracle import TcarOracle
    p0, content, mw, batch = inputs(name)
    r = _forward(TcarOracle(p0 if params is None else params, content, mw), batch)
    r.update(name=name, label=batch["label"], seen=(batch["seq"] - 1).astype(np.int64), delta=1e-3 * np.abs(r["s"]).max(1),
             absdot=np.abs(r["A"]) @ np.abs(r["E"]).T)
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    if params is None:
        _REF[name] = r
    return r


def lengths(name):
    """the lengths of the case's sessions in its ragged feed: 1, T, 2, 5, 8 in turn (those at most T), so 1 and T are always there"""
    c = CASES[name]
    cycle = [n for n in OrderedDict.fromkeys((1, c.T, 2, 5, 8)) if n <= c.T]
    return np.array([cycle[b % len(cycle)] for b in range(c.B)], np.int32)


def ragged_reference(name):
    """The case's sessions cut to lengths(name): `feeds`, one labelled rectangular feed [1, len] per session in session order (what
    pack_sessions takes), and the oracle's s / ce / delta / absdot of every session AT ITS OWN LENGTH — eval_batch per length group,
    the rows put back in session order, as tests/ragged_util.py builds them.  seen: [B, T], -1 behind a session's own items."""
    if name not in _RAGGED:
        from oracle.tcar_oracle import TcarOracle
        params, content, mw, batch = inputs(name)
        c, lens = CASES[name], lengths(name)
        oracle = TcarOracle(params, content, mw)
        s, ce, absdot = np.zeros((c.B, c.N)), np.zeros(c.B), np.zeros((c.B, c.N))
        for n in sorted(set(lens.tolist())):
            idx = np.where(lens == n)[0]
            sub = {k: batch[k][idx][:, :n] for k in PER_ROW}
            sub.update({k: batch[k][idx] for k in ("cw", "ch", "label")})
            r = _forward(oracle, sub)
            s[idx], ce[idx], absdot[idx] = r["s"], r["ce"], np.abs(r["A"]) @ np.abs(r["E"]).T
        feeds = []
        for b, n in enumerate(lens):
            f = {k: batch[k][b:b + 1, :n].copy() for k in PER_ROW}
            f.update({k: batch[k][b:b + 1].copy() for k in ("cw", "ch", "label")})
            feeds.append(f)
        seen = (batch["seq"] - 1).astype(np.int64)
        seen[np.arange(c.T)[None, :] >= lens[:, None]] = -1
        _RAGGED[name] = dict(name=name + ", ragged", lens=lens, feeds=feeds, s=s, ce=ce, delta=1e-3 * np.abs(s).max(1), absdot=absdot,
                             label=batch["label"], seen=seen)
        for a in (s, ce, absdot, seen, lens):
            a.setflags(write=False)
    return _RAGGED[name]


def trained_reference(name, steps=2):
    """The fp64 oracle trained `steps` steps on the case's batch from its initial variables, then a third step: `params` after
    `steps` steps (fp32, what an engine would export), `before` / `after` = reference(name) of the initial / trained variables,
    `stale` = the trained scores with the candidate-time part of E taken from the INITIAL variables (a time plane that was never
    rebuilt), and `loss3`, the per-session loss of the step after."""
    if name not in _TRAIN:
        from oracle.tcar_oracle import TcarOracle
        params, content, mw, batch = inputs(name)
        ora = TcarOracle(params, content, mw, max_grad=2.0)
        for _ in range(steps):
            ora.train_step(batch)
        trained = OrderedDict((k, v.astype(np.float32)) for k, v in ora.export().items())
        loss3 = ora.train_step(batch).numpy().astype(np.float64)
        before, after = reference(name), reference(name, trained)
        pt = before["E"].shape[1] - after["attout_t"].shape[1]
        stale = after["s"] + after["attout_t"].astype(np.float64) @ (before["E"][:, pt:] - after["E"][:, pt:]).T
        _TRAIN[name] = dict(params=trained, before=before, after=after, stale=stale, loss3=loss3)
    return _TRAIN[name]


def candidate_lists(name, C):
    """cand [B, C] int32: the session's label in slot 0 and, for C > 1, random ids of [0, N), three repeats of earlier slots and three
    empty slots (-1, N, -7), the slots behind the first shuffled row by row"""
    c = CASES[name]
    rng = np.random.RandomState(c.seed + C)
    cand = np.empty((c.B, C), np.int32)
    cand[:, 0] = inputs(name)[3]["label"]
    if C > 1:
        assert C >= 8
        cand[:, 1:C - 6] = rng.randint(0, c.N, (c.B, C - 7))
        cand[:, C - 6:C - 3] = np.take_along_axis(cand, rng.randint(0, C - 6, (c.B, 3)), 1)
        cand[:, C - 3:] = [-1, c.N, -7]
        for b in range(c.B):
            cand[b, 1:] = cand[b, 1:][rng.permutation(C - 1)]
    return cand


# ------------------------------------------------------------------------------------------------------ checkers
def check_band(s, delta, topk, k, gone=None, name="", short=False):
    """(a)-(d): k distinct in-range ids, sorted within 2 delta, everything clearly above the k-th score in, nothing clearly below.
    short=True: a session with fewer than k eligible items lists exactly those, in the same bands, and -1 behind them (a session
    with k or more is held exactly as without it)."""
    for b in range(s.shape[0]):
        row, d2 = s[b].copy(), 2 * delta[b]
        if gone is not None:
            row[gone[b][gone[b] >= 0]] = -np.inf
        n = k
        if short:
            n = min(k, int((row > -np.inf).sum()))
            assert (topk[b, n:] == -1).all(), (name, b, topk[b])
            if n == 0:
                continue
        t = topk[b, :n].astype(np.int64)
        assert len(set(t.tolist())) == n and t.min() >= 0 and t.max() < s.shape[1], (name, b, t)            # (a)
        assert (row[t[:-1]] >= row[t[1:]] - d2).all(), (name, b)                                            # (b)
        kth = np.sort(row)[-n]
        assert set(np.where(row > kth + d2)[0].tolist()) <= set(t.tolist()), (name, b)                      # (c)
        assert (row[t] >= kth - d2).all(), (name, b)                                                        # (d)


def _close(got, want, what, name, ref):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape == want.shape and got.size:
        tol = 1e-3 * np.abs(want) + 2e-5 * max(float(np.abs(want).max()), 1e-30) + 1e-9
        with np.errstate(invalid="ignore"):
            r = np.abs(got - want) / tol
        note("%s | %s" % (ref["name"], what), np.where(np.isnan(r), np.inf, r).max())
    close(got, want, name="%s: %s" % (name, what))


def _list_order(ids, sc, name, b):
    """scores descend, equal scores go by id descending"""
    assert (sc[:-1] >= sc[1:]).all(), (name, b)
    ties = sc[:-1] == sc[1:]
    assert (ids[:-1][ties] > ids[1:][ties]).all(), (name, b)


def check_eval(ref, rank, topk, ce, scores, k=TOPK, name=""):
    """eval_step_streamed against the oracle: (a)-(d) on the list, (e) the rank inside [lo, hi], (f) the list's scores, (g) ce"""
    s, delta, lab = ref["s"], ref["delta"], ref["label"]
    B, N = s.shape
    assert topk.shape == (B, k) and topk.dtype == np.int32 and rank.shape == (B,) and scores.shape == (B, k) and ce.shape == (B,), name
    assert np.isfinite(ce).all() and np.isfinite(scores).all(), name
    check_band(s, delta, topk, k, name=name)
    sl = s[np.arange(B), lab]
    others = np.arange(N)[None, :] != lab[:, None]
    lo = 1 + (s > (sl + 2 * delta)[:, None]).sum(1)
    hi = 1 + ((s > (sl - 2 * delta)[:, None]) & others).sum(1)
    assert ((lo <= rank) & (rank <= hi)).all(), (name, rank, lo, hi)                                        # (e)
    _close(scores, np.take_along_axis(s, topk.astype(np.int64), 1), "eval scores", name, ref)                    # (f)
    _close(ce, ref["ce"], "eval ce", name, ref)                                                                  # (g)


def check_recommend(ref, topk, scores, k=TOPK, short=False, name=""):
    """recommend(exclude_seen=True): no seen item listed, list order, the bands with the seen items gone, the list's scores"""
    s, delta, seen = ref["s"], ref["delta"], ref["seen"]
    B = s.shape[0]
    assert topk.shape == (B, k) and topk.dtype == np.int32 and scores.shape == (B, k), name
    for b in range(B):
        n = int((topk[b] >= 0).sum())
        assert (topk[b, :n] >= 0).all() and not set(topk[b, :n].tolist()) & set(seen[b][seen[b] >= 0].tolist()), (name, b)
        _list_order(topk[b, :n], scores[b, :n], name, b)
    check_band(s, delta, topk, k, gone=seen, name=name, short=short)
    live = topk >= 0
    _close(scores[live], np.take_along_axis(s, np.where(live, topk, 0).astype(np.int64), 1)[live], "recommend scores", name, ref)


def check_candidates(ref, cand, scores, rank_of, order, name=""):
    """score_candidates: the gates (a), (b) and the order of tests/test_gpu_cand_serve.py"""
    s, delta = ref["s"], ref["delta"]
    B, N = s.shape
    live = (cand >= 0) & (cand < N)
    assert scores.shape == cand.shape and rank_of.shape == cand.shape and order.shape == cand.shape and rank_of.dtype == np.int32, name
    want = np.take_along_axis(s, np.where(live, cand, 0).astype(np.int64), 1)
    assert (scores[~live] == -np.inf).all() and (rank_of[~live] == 0).all(), name
    _close(scores[live], want[live], "candidate scores", name, ref)
    for b in range(B):
        slots, d2 = np.where(live[b])[0], 2 * delta[b]
        sb = want[b, slots]
        lo = 1 + (sb[None, :] > sb[:, None] + d2).sum(1)
        hi = 1 + ((sb[None, :] > sb[:, None] - d2) & ~np.eye(len(slots), dtype=bool)).sum(1)
        rk = rank_of[b, slots]
        assert ((lo <= rk) & (rk <= hi)).all(), (name, b, rk, lo, hi)
        assert sorted(rk.tolist()) == list(range(1, len(slots) + 1)), (name, b)
        assert (rank_of[b, order[b, :len(slots)]] == np.arange(1, len(slots) + 1)).all() and (order[b, len(slots):] == -1).all(), (name, b)


def beta_of(ref, split):
    """the band of a coarse score: split-bf16 engines contract the hi planes alone; the fp32 engine's coarse scores are its own"""
    return U * ref["absdot"] + ref["delta"][:, None] if split else np.broadcast_to(ref["delta"][:, None], ref["s"].shape)


def check_coarse(ref, ids, coarse, C, split, name=""):
    """retrieve(exclude_seen=False): rule (b) of tests/test_gpu_retrieve_serve.py — min(C, N) distinct items in list order, every
    coarse score inside beta, everything the oracle puts clearly (2 beta) above its C-th best in, nothing clearly below it"""
    s, beta = ref["s"], beta_of(ref, split)
    B, N = s.shape
    n = min(C, N)
    assert ids.shape == (B, C) and ids.dtype == np.int32 and coarse.shape == (B, C) and coarse.dtype == np.float32, name
    assert (ids[:, n:] == -1).all() and (coarse[:, n:] == -np.inf).all(), name
    for b in range(B):
        t = ids[b, :n].astype(np.int64)
        assert len(set(t.tolist())) == n and t.min() >= 0 and t.max() < N, (name, b)
        err = np.abs(coarse[b, :n].astype(np.float64) - s[b, t])
        with np.errstate(invalid="ignore"):
            r = err / beta[b, t]
        note("%s | coarse score / beta" % ref["name"], np.where(np.isnan(r), np.inf, r).max())
        assert (err <= beta[b, t]).all(), (name, b, float((err / beta[b, t]).max()))
        cth = np.sort(s[b])[-C] if C <= N else -np.inf
        must = np.where(s[b] > cth + 2 * beta[b])[0]
        assert set(must.tolist()) <= set(t.tolist()), (name, b, sorted(set(must.tolist()) - set(t.tolist())))
        assert (s[b, t] >= cth - 2 * beta[b, t]).all(), (name, b)
        _list_order(t, coarse[b, :n], name, b)


def kept_sessions(ref, k, C, split):
    """Rule (e) of tests/test_gpu_retrieve_serve.py: the sessions whose oracle gap between the k-th and the C-th best score exceeds
    2 max_n beta[b, n] -> (keep [B] bool, margin [B] = gap / (2 max beta)).  A shortlist of C >= N items is the whole catalog:
    nothing can be missing from it and every session is kept."""
    s, beta = ref["s"], beta_of(ref, split)
    if C >= s.shape[1]:
        return np.ones(s.shape[0], bool), np.full(s.shape[0], np.inf)
    srt = -np.sort(-s, 1)
    margin = (srt[:, k - 1] - srt[:, C - 1]) / (2 * beta.max(1))
    return margin > 1, margin


def check_two_stage(ref, top, top_sc, rt_ids, rt_exact, k, C, split, name=""):
    """recommend_two_stage(exclude_seen=False): the list is exactly the top k of the call's own exact scores over its own shortlist,
    and (the sessions of kept_sessions, at least 90 % of them) it passes the bands of the streamed lists"""
    s, delta = ref["s"], ref["delta"]
    B = s.shape[0]
    assert top.shape == (B, k) and top.dtype == np.int32 and rt_ids.shape == (B, C) and rt_exact.shape == (B, C), name
    for b in range(B):
        o = np.lexsort((rt_ids[b], rt_exact[b]))[::-1][:k]
        assert (top[b] == rt_ids[b, o]).all() and top_sc[b].tobytes() == rt_exact[b, o].tobytes(), (name, b)
    keep, _ = kept_sessions(ref, k, C, split)
    assert (~keep).mean() <= 0.10, (name, (~keep).mean())
    check_band(s[keep], delta[keep], top[keep], k, name=name)
    _close(top_sc[keep], np.take_along_axis(s, top.astype(np.int64), 1)[keep], "two-stage scores", name, ref)


# ------------------------------------------------------------- what an engine with the scores x [B, N] (fp32) would return
def forge_eval(x, label, k=TOPK, lab_score=None):
    """(rank, topk, ce, scores) of eval_step_streamed by the numpy model of the select fold (tests/select_ref.py) over the scores x;
    lab_score: the label scores the step computed (None: x[b, label[b]])"""
    x = np.asarray(x, np.float32)
    B, N = x.shape
    rank, topk, ce, scores = np.zeros(B, np.int32), np.full((B, k), -1, np.int32), np.zeros(B, np.float32), np.zeros((B, k), np.float32)
    for b in range(B):
        ls = x[b, label[b]] if lab_score is None else np.float32(lab_score[b])
        st = fold_state(np.arange(N), x[b], k, label=int(label[b]), lab_score=ls)
        topk[b], rank[b], ce[b] = finish(st, k, ls)
        scores[b, :len(st["scores"])] = st["scores"]
    return rank, topk, ce, scores


def forge_recommend(x, excl, k=TOPK):
    """(topk, scores) of recommend with the exclusion lists excl [B, X] (-1: an empty slot; None: nothing excluded)"""
    x = np.asarray(x, np.float32)
    B, N = x.shape
    topk, scores = np.full((B, k), -1, np.int32), np.full((B, k), -np.inf, np.float32)
    for b in range(B):
        gone = () if excl is None else [int(i) for i in excl[b] if i >= 0]
        st = fold_state(np.arange(N), x[b], k, excl=gone)
        topk[b] = finish(st, k)[0]
        scores[b, :len(st["scores"])] = st["scores"]
    return topk, scores


def forge_candidates(x, cand):
    """(scores, rank_of, order) of score_candidates"""
    x = np.asarray(x, np.float32)
    live = (cand >= 0) & (cand < x.shape[1])
    scores = np.where(live, np.take_along_axis(x, np.where(live, cand, 0).astype(np.int64), 1), -np.inf).astype(np.float32)
    rank_of, order, _, _ = rank_model(scores, np.where(live, cand, -1))
    return scores, rank_of, order


def forge_retrieve(x, C):
    """(ids, coarse) of retrieve(exclude_seen=False) over the coarse scores x"""
    return shortlist(x, C)


def forge_two_stage(coarse, exact, k, C):
    """(top, top_sc, rt_ids, rt_exact) of recommend_two_stage(exclude_seen=False): shortlist from `coarse`, reranked by `exact`"""
    ids, _ = shortlist(coarse, C)
    live = ids >= 0
    ex = np.where(live, np.take_along_axis(np.asarray(exact, np.float32), np.where(live, ids, 0).astype(np.int64), 1), -np.inf).astype(np.float32)
    B = ids.shape[0]
    top, top_sc = np.zeros((B, k), np.int32), np.zeros((B, k), np.float32)
    for b in range(B):
        o = np.lexsort((ids[b], ex[b]))[::-1][:k]
        top[b], top_sc[b] = ids[b, o], ex[b, o]
    return top, top_sc, ids, ex
