"""Ragged batches at the engine level (include/tcar_ragged.h; TcarEngine.eval_step_streamed / recommend / retrieve /
recommend_two_stage / score_candidates on a feed with "len"), through Seq2SeqAttNN and through test() with --eval_mixed, at the
shape of serve_case.reference(): N = 700, H = 250, Ht = 64, B = 41, panel 256, k = 20.

Uniform lengths and permutations are held bit for bit; mixed lengths against the fp64 oracle (eval_batch per length group, rows put
back in session order) in exactly the bands the rectangular tests use — delta_b = 1e-3 * max_n |s[b, n]|, no session and no item
left out."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401

from ragged_util import mixed_reference, own_items, permuted, random_ragged
from gpu_util import _need_gpu, _np, close
from quota_case import CAT, K, M, walk_of_the_best_64
from serve_case import B, C_, N, PANEL, SHORT, TOPK, _lists, reference
from serve_case import beta_of_engine as _beta
from serve_shapes_ref import check_band
from window_case import check_band as check_pool
from window_case import check_eval
from window_case import reference as wref

pytestmark = pytest.mark.gpu


def _engine(scoring):
    from tcar_amd.engine import TcarEngine
    r = reference()
    return TcarEngine(r["params"], r["content"], r["mw"], max_grad=2.0, scoring=scoring)


def _unlabelled(feed):
    return {n: v for n, v in feed.items() if n not in ("label", "neg")}


def _five_calls(eng, feed, cand, clicked):
    """every output of the five serving calls on `feed` (rectangular or ragged), and attout behind the first: numpy copies"""
    nb = eng._sessions(feed)
    out = {}
    rank, topk, ce = eng.eval_step_streamed(feed, k=TOPK, panel=PANEL)
    out["eval"] = _np(rank, topk, ce, eng.last_scores)
    out["attout"] = _np(eng.attout[:nb])
    free = _unlabelled(feed)
    out["recommend"] = _np(*eng.recommend(free, k=TOPK, panel=PANEL, exclude_seen=True))
    out["retrieve"] = _np(*eng.retrieve(free, SHORT, panel=PANEL))
    out["two_stage"] = _np(*eng.recommend_two_stage(free, k=TOPK, shortlist=SHORT, panel=PANEL))
    out["cand"] = _np(*eng.score_candidates(free, cand, clicked))
    out["attout_last"] = _np(eng.attout[:nb])
    return out


def _same_bits(a, b, what):
    assert sorted(a) == sorted(b)
    for name in a:
        for i, (x, y) in enumerate(zip(a[name], b[name])):
            assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, name, i)


@pytest.mark.parametrize("scoring", ["f32", "bf16x3-mixed"])
def test_uniform_lengths_give_the_bits_of_the_rectangular_calls(scoring):
    _need_gpu()
    from tcar_amd.host.data import pack_sessions
    eng = _engine(scoring)
    cand, clicked = _lists()
    rect3 = {n: v for n, v in reference()["batch"].items() if n != "neg"}
    # a fresh T = 40 batch of 41 sessions: R = 1,640 rows, above TCAR_PROJ_SPLIT_ROWS — the projections run un-split
    flat = random_ragged(np.full(B, 40, np.int32), 29)
    rect40 = {n: (v.reshape(B, 40) if v.shape[0] == B * 40 else v) for n, v in flat.items() if n != "len"}
    for name, rect in (("T = 3", rect3), ("T = 40", rect40)):
        ragged = pack_sessions([rect])
        assert ragged["len"].tolist() == [rect["seq"].shape[1]] * B and ragged["seq"].ndim == 1
        want = _five_calls(eng, rect, cand, clicked)
        got = _five_calls(eng, ragged, cand, clicked)
        _same_bits(got, want, name)
        assert np.isfinite(want["attout"][0]).all() and (want["eval"][1] >= 0).all()
    eng.check_forks()


@pytest.mark.parametrize("mix", ["small", "long"])
@pytest.mark.parametrize("scoring", ["f32", "bf16x3-mixed"])
def test_mixed_lengths_match_the_oracle_in_the_bands_of_the_rectangular_tests(scoring, mix):
    _need_gpu()
    m = mixed_reference(mix)
    feed, s, delta, lab = m["feed"], m["s"], m["delta"], m["feed"]["label"]
    assert (feed["len"].sum() <= 1024) == (mix == "small")              # the slab form of the projections / the un-split one
    eng = _engine(scoring)
    eng.eval_step(reference()["batch"], k=TOPK)                          # (allocates the [B, N] matrix the streamed calls must not touch)
    eng.logits.fill_(float("nan"))
    # --- exactly the checks of test_streamed_evaluation_and_recommendation_match_the_oracle_in_bands
    rank, topk, ce = eng.eval_step_streamed(feed, k=TOPK, panel=PANEL)
    rank, topk, ce, scores = _np(rank, topk, ce, eng.last_scores)
    assert bool(torch.isnan(eng.logits).all())
    assert np.isfinite(ce).all() and np.isfinite(scores).all()
    assert topk.shape == (B, TOPK) and topk.dtype == np.int32 and rank.shape == (B,)
    check_band(s, delta, topk, TOPK, name="eval")
    sl = s[np.arange(B), lab]
    others = np.arange(N)[None, :] != lab[:, None]
    lo = 1 + (s > (sl + 2 * delta)[:, None]).sum(1)
    hi = 1 + ((s > (sl - 2 * delta)[:, None]) & others).sum(1)
    assert ((lo <= rank) & (rank <= hi)).all(), (rank, lo, hi)
    close(scores, np.take_along_axis(s, topk.astype(np.int64), 1), name="scores")
    close(ce, m["ce"], name="ce vs oracle")
    rank1, topk1, ce1 = _np(*eng.eval_step_streamed(feed, k=TOPK))                       # the default panel: one fold
    check_band(s, delta, topk1, TOPK, name="eval, default panel")
    assert ((lo <= rank1) & (rank1 <= hi)).all()
    close(ce1, m["ce"], name="ce vs oracle, default panel")
    # --- recommend: every session's own items are gone, and nothing of another session's
    free = _unlabelled(feed)
    tk, sc = _np(*eng.recommend(free, k=TOPK, exclude_seen=False, panel=PANEL))
    assert (tk == topk).all() and sc.tobytes() == scores.tobytes()
    seen = own_items(feed)
    assert seen.shape == (B, 40) and (seen[0, 1:] == -1).all() and m["best0"] in seen[1].tolist() and m["best0"] not in seen[0].tolist()
    tk, sc = _np(*eng.recommend(free, k=TOPK, panel=PANEL))
    for b in range(B):
        assert not set(tk[b].tolist()) & set(seen[b][seen[b] >= 0].tolist()), b
        assert (sc[b, :-1] >= sc[b, 1:]).all(), b
        ties = sc[b, :-1] == sc[b, 1:]
        assert (tk[b, :-1][ties] > tk[b, 1:][ties]).all(), b
    check_band(s, delta, tk, TOPK, gone=seen, name="recommend")
    # session 0's best item sits in session 1, in a column session 0 does not own: the -1 padding keeps it in session 0's list
    assert m["best0"] in tk[0].tolist()
    extra = np.full((B, 5), -1, np.int32)
    extra[:, 0], extra[:, 2], extra[:, 3] = tk[:, 0], tk[:, 7], tk[:, 0]
    tk2, sc2 = _np(*eng.recommend(free, k=TOPK, exclude=extra, panel=PANEL))
    gone = np.concatenate([seen, extra.astype(np.int64)], 1)
    for b in range(B):
        assert not set(tk2[b].tolist()) & set(gone[b][gone[b] >= 0].tolist()), b
    check_band(s, delta, tk2, TOPK, gone=gone, name="recommend + exclude")
    assert np.isfinite(sc2).all()
    # --- score_candidates: the bands of test_gpu_cand_serve (the label column of its lists is this batch's)
    cand, clicked = _lists()
    cand = cand.copy()
    cand[:, 0] = lab
    live = (cand >= 0) & (cand < N)
    cscore, rank_of, order, counts, _ = _np(*eng.score_candidates(free, cand, clicked))
    want = np.take_along_axis(s, np.where(live, cand, 0).astype(np.int64), 1)
    assert cscore.shape == (B, C_) and (cscore[~live] == -np.inf).all() and (rank_of[~live] == 0).all()
    close(cscore[live], want[live], name="candidate scores")
    for b in range(B):
        slots, d2 = np.where(live[b])[0], 2 * delta[b]
        sb = want[b, slots]
        lo_ = 1 + (sb[None, :] > sb[:, None] + d2).sum(1)
        hi_ = 1 + ((sb[None, :] > sb[:, None] - d2) & ~np.eye(len(slots), dtype=bool)).sum(1)
        rk = rank_of[b, slots]
        assert ((lo_ <= rk) & (rk <= hi_)).all(), (b, rk, lo_, hi_)
        assert (rank_of[b, order[b, :len(slots)]] == np.arange(1, len(slots) + 1)).all() and (order[b, len(slots):] == -1).all()
        pos, neg = want[b, slots[clicked[b, slots] != 0]], want[b, slots[clicked[b, slots] == 0]]
        assert counts[b, 0] == len(pos) and counts[b, 1] == len(neg)
        lo2, hi2 = 2 * (pos[:, None] > neg[None, :] + d2).sum(), 2 * (pos[:, None] > neg[None, :] - d2).sum()
        assert lo2 <= counts[b, 2] <= hi2, (b, lo2, counts[b, 2], hi2)
    # --- retrieve and the two-stage call: the bands of test_gpu_retrieve_serve
    ids, coarse = _np(*eng.retrieve(free, SHORT, exclude_seen=False, panel=PANEL))
    assert ids.shape == (B, SHORT) and (ids >= 0).all() and (ids < N).all()
    if scoring == "f32":                     # the coarse precision is the engine's own: the streamed selection over the same GEMM
        want_ids, want_sc = _np(*eng.recommend(free, k=64, exclude_seen=False, panel=PANEL))
        assert (ids[:, :64] == want_ids).all() and coarse[:, :64].tobytes() == want_sc.tobytes()
        beta = np.broadcast_to(delta[:, None], s.shape)
    else:
        beta = _beta(eng, delta)
    for b in range(B):
        t = ids[b].astype(np.int64)
        assert len(set(t.tolist())) == SHORT, b
        cth = np.sort(s[b])[-SHORT]
        must = np.where(s[b] > cth + 2 * beta[b])[0]
        assert set(must.tolist()) <= set(t.tolist()), b
        assert (s[b, t] >= cth - 2 * beta[b, t]).all(), b
        assert (np.abs(coarse[b].astype(np.float64) - s[b, t]) <= beta[b, t]).all(), b
        assert (coarse[b, :-1] >= coarse[b, 1:]).all(), b
    top, top_sc = _np(*eng.recommend_two_stage(free, k=TOPK, shortlist=SHORT, exclude_seen=False, panel=PANEL))
    sid, exact = _np(eng.rt_ids[:B], eng.rt_exact[:B])
    assert (sid == ids).all()
    for b in range(B):                       # the list is the top k of the exact scores over the call's own shortlist
        o = np.lexsort((sid[b], exact[b]))[::-1][:TOPK]
        assert (top[b] == sid[b, o]).all() and top_sc[b].tobytes() == exact[b, o].tobytes(), b
    srt = -np.sort(-s, 1)
    keep = srt[:, TOPK - 1] - srt[:, SHORT - 1] > 2 * beta.max(1)
    assert (~keep).mean() <= 0.10, (~keep).mean()
    check_band(s[keep], delta[keep], top[keep], TOPK, name="two-stage")
    close(top_sc[keep], np.take_along_axis(s, top.astype(np.int64), 1)[keep], name="two-stage scores")
    assert bool(torch.isnan(eng.logits).all())
    eng.check_forks()


@pytest.mark.parametrize("scoring", ["f32", "bf16x3-mixed"])
def test_a_permutation_of_the_sessions_permutes_the_results_bit_for_bit(scoring):
    """the same R and B, so the same launches: no sum in the head depends on where a row sits — this pins off[]"""
    _need_gpu()
    feed = mixed_reference("small")["feed"]
    perm = np.random.RandomState(9).permutation(B)
    assert (feed["len"][perm] != feed["len"]).any()
    eng = _engine(scoring)
    cand, clicked = _lists()
    a = _five_calls(eng, feed, cand, clicked)
    b = _five_calls(eng, permuted(feed, perm), cand[perm], clicked[perm])
    _same_bits({n: [x[perm] for x in v] for n, v in a.items()}, b, "permuted")
    eng.check_forks()


def test_window_cap_and_exclusions_carry_over_to_a_mixed_batch():
    _need_gpu()
    m = mixed_reference("small")
    feed, s, delta, lab = m["feed"], m["s"], m["delta"], m["feed"]["label"]
    free = _unlabelled(feed)
    w = wref()                               # its item keys and per-session windows: everything | a third | seven items | none
    key, win = w["key"], w["win"]
    eng = _engine("bf16x3-mixed")
    eng.set_item_keys(key)
    eng.set_categories(CAT)
    # per-session windows, held against the oracle inside every session's pool as test_gpu_window_serve holds them
    tkw, _ = _np(*eng.recommend(free, k=TOPK, panel=PANEL, exclude_seen=False, window=(w["lo"], w["hi"])))
    assert ((tkw >= 0).sum(1) == np.minimum(win.sum(1), TOPK)).all() and (tkw[3::4] == -1).all()
    check_pool(s, delta, tkw, TOPK, win, name="recommend, window")
    seen = own_items(feed)
    unseen = win.copy()
    for b in range(B):
        unseen[b, seen[b][seen[b] >= 0]] = False
    tks, _ = _np(*eng.recommend(free, k=TOPK, panel=PANEL, window=(w["lo"], w["hi"])))
    check_pool(s, delta, tks, TOPK, unseen, name="recommend, window + seen")
    pool = win | (np.arange(N)[None, :] == lab[:, None])
    rank, topk, ce = eng.eval_step_streamed(feed, k=TOPK, panel=PANEL, window=(w["lo"], w["hi"]))
    rank, topk, ce, scores = _np(rank, topk, ce, eng.last_scores)
    check_eval(dict(s=s, delta=delta, batch={"label": lab}), pool, rank, topk, ce, scores, "eval, windows by session")
    # a cap: the walk over the uncapped best 64 (test_gpu_quota_serve: exact, no tolerance), the uncapped 64 held in the band
    tk64, sc64 = _np(*eng.recommend(free, k=64, panel=PANEL))
    check_band(s, delta, tk64, 64, gone=seen, name="recommend, k = 64")
    want_tk, want_sc = walk_of_the_best_64(tk64, sc64)
    got_tk, got_sc = _np(*eng.recommend(free, k=K, panel=PANEL, max_per_category=M))
    assert (got_tk == want_tk).all() and got_sc.tobytes() == want_sc.tobytes()
    assert all(np.unique(CAT[t], return_counts=True)[1].max() <= M for t in got_tk) and (got_tk != tk64[:, :K]).any()
    # exclusions on top of the sessions' own items
    extra = (np.arange(B * 3, dtype=np.int32).reshape(B, 3) * 7) % N
    tkx, _ = _np(*eng.recommend(free, k=TOPK, panel=PANEL, exclude=extra))
    gone = np.concatenate([seen, extra.astype(np.int64)], 1)
    for b in range(B):
        assert not set(tkx[b].tolist()) & set(gone[b][gone[b] >= 0].tolist()), b
    check_band(s, delta, tkx, TOPK, gone=gone, name="recommend + exclude")
    eng.check_forks()


def test_training_the_materialised_evaluation_and_the_sharded_engine_refuse_a_ragged_feed():
    _need_gpu()
    from tcar_amd.sharded import ShardedEngine
    feed = mixed_reference("small")["feed"]
    eng = _engine("bf16x3-mixed")
    for call in (lambda: eng.train_step(feed), lambda: eng.eval_step(feed), lambda: eng.loss_and_grads(feed),
                 lambda: eng.train_step(None, bt=eng.upload(feed))):
        with pytest.raises(ValueError, match="rectangular feed"):
            call()
    r = reference()
    sh = ShardedEngine(r["params"], r["content"], r["mw"], max_grad=2.0, scoring="bf16x3-mixed", world=1, rank=0)
    for call in (lambda: sh.eval_step_streamed(feed, k=TOPK, panel=PANEL), lambda: sh.recommend(_unlabelled(feed), k=TOPK, panel=PANEL)):
        with pytest.raises(ValueError, match="rectangular feeds"):
            call()
    rank, _, _ = eng.eval_step_streamed(feed, k=TOPK, panel=PANEL)          # the engine is as usable as before
    assert rank.shape == (B,)


def test_the_model_takes_a_list_of_feeds():
    _need_gpu()
    from tcar_amd.host.data import pack_sessions
    from tcar_amd.host.model import Seq2SeqAttNN, initial_variables
    from tcar_amd.host.synth import SynthFold
    fold = SynthFold(n_items=400, dim=32, n_train=300, n_test=200, seed=17, active_t=True)
    np.random.seed(3)
    args = fold.model_args(batch_size=64, epoch=1, neg_num=8, hidden_size=32, time_hidden_size=16, lr=0.003,
                           initial_variables=initial_variables(400, 32, 16, 0.3, 0.1), emb_stddev=0.3, stddev=0.1, scoring="bf16x3")
    with redirect_stdout(io.StringIO()):
        model = Seq2SeqAttNN(args)
    lens = np.unique(fold.test.in_len)[:3]
    assert len(lens) == 3
    feeds = [_unlabelled(fold.test.batch_arrays(np.where(fold.test.in_len == n)[0][:b], "active_t")) for n, b in zip(lens, (4, 1, 3))]
    nb = sum(f["seq"].shape[0] for f in feeds)
    packed = pack_sessions(feeds)
    top, sc = _np(*model.recommend(feeds, k=5))
    want, want_sc = _np(*model.engine.recommend(packed, k=5))
    assert top.shape == (nb, 5) and (top == want).all() and sc.tobytes() == want_sc.tobytes()
    # ... and session by session it is what the rectangular call of the session's own feed gives, in the band of equal scores
    s0 = 0
    for f in feeds:
        one, one_sc = _np(*model.recommend(f, k=5))
        close(sc[s0:s0 + len(one)], one_sc, name="list of feeds vs one feed")
        s0 += len(one)
    ids, _ = _np(*model.retrieve(feeds, 70))
    want_ids, _ = _np(*model.engine.retrieve(packed, 70))
    assert ids.shape == (nb, 70) and (ids == want_ids).all()
    cand = np.tile(np.arange(6, dtype=np.int32), (nb, 1))
    res = model.score_candidates(feeds, cand)
    assert res.scores.cpu().numpy().tobytes() == model.engine.score_candidates(packed, cand).scores.cpu().numpy().tobytes()
    res = model.score_candidates(fold.test.ragged_arrays(np.arange(7), "active_t"), np.tile(np.arange(6, dtype=np.int32), (7, 1)))
    assert tuple(res.scores.shape) == (7, 6) and bool(torch.isfinite(res.scores).all())


def _prefix(line):
    return line.split(":")[0] if ":" in line else line.split(" ")[0]


def test_eval_mixed_streams_the_catalog_less_often_and_reports_the_same_metrics():
    _need_gpu()
    from tcar_amd.host.cli import main
    common = ["--synthetic", "400", "--synthetic_train", "1500", "--synthetic_test", "200", "--epoch", "1", "--hidden_size", "48",
              "--time_hidden_size", "16", "--batch_size", "64", "--eval_panel", "256"]
    out = {}
    for flag in ((), ("--eval_mixed", "1")):
        buf = io.StringIO()
        with redirect_stdout(buf):
            model = main(common + list(flag))
        out[bool(flag)] = (buf.getvalue().splitlines(), dict(model.last_metrics))
    (plain, m0), (lines, m1) = out[False], out[True]
    print(m0, m1)
    assert [_prefix(l) for l in lines] == [_prefix(l) for l in plain]               # the same lines in the same order
    assert any(l.startswith("MRR@20: ") for l in lines) and sum(l.startswith("batch_in:") for l in lines) == 2
    assert 0 < m1["eval_calls"] < m0["eval_calls"], (m0["eval_calls"], m1["eval_calls"])
    assert m1["sessions"] == m0["sessions"] == 200
    assert abs(m1["loss"] - m0["loss"]) <= 1e-3 * abs(m0["loss"]), (m0, m1)              # the project's loss gate
    for name in ("recall", "mrr", "ndcg"):                                              # +-0.002, as tests/test_gpu_e2e.py allows a trained run
        assert abs(m1[name] - m0[name]) <= 0.002 + 1e-12, (name, m0, m1)
