"""The diversified two-stage call through the engine (TcarEngine.recommend_two_stage(diversity=...), TcarEngine.diversify,
Seq2SeqAttNN.recommend, test() with --eval_diversity; tcar_mmr_rerank_step and its ragged twin) on the first 16 sessions of the
setup of tests/serve_case.py: N = 700, H = 250, shortlist 128, panel 256, k = 20.

The fp64 checks are those of tests/test_gpu_mmr_walk.py (b), on what the call itself left on the engine: its shortlist (rt_ids), the
exact scores (rt_exact) and the content columns of E.  TOL_SIM = (H + 8) 2^-24 and tau = mu TOL_SIM + 2^-23 max(max |s|, mu) as derived
there.  Sessions whose fp64 walk has a step decided by at most 2 tau are left out of the comparison of whole lists; from the oracle's
scores alone (the 128 best per session as the shortlist, mu = 2) that leaves out 0 of 16 with the smallest gap at 8.4e-4 = 13 x 2 tau,
so at most 2 of 16 may be left out here."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest

import tcar_amd  # noqa: F401

from cand_ref import rank_model
from gpu_util import _need_gpu, _np
from mmr_ref import tau_greedy, walk_f64
from ragged_util import group, random_ragged
from serve_case import H, N, PANEL, SHORT, TOPK, _feed, _keys_and_windows, reference

pytestmark = pytest.mark.gpu

NB = 16
TOL_SIM = (H + 8) * 2.0 ** -24
KW = dict(k=TOPK, shortlist=SHORT, panel=PANEL)


def _feed16():
    return {n: v[:NB] for n, v in _feed().items()}


def _engine(scoring="bf16x3-mixed", content=None):
    from tcar_amd.engine import TcarEngine
    r = reference()
    return TcarEngine(r["params"], r["content"] if content is None else content, r["mw"], max_grad=2.0, scoring=scoring)


def _call(eng, feed, mu, **kw):
    """(topk, scores, msim) of one diversified call: numpy copies"""
    top, sc = eng.recommend_two_stage(feed, diversity=mu, **dict(KW, **kw))
    return _np(top, sc, eng.rt_msim[:top.shape[0]])


def _same(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, i)


@pytest.mark.parametrize("scoring", ["bf16x3-mixed", "f32"])
def test_diversity_zero_returns_the_bytes_of_the_plain_call_fresh_and_trained(scoring):
    _need_gpu()
    eng, feed = _engine(scoring), _feed16()
    for state in ("fresh", "trained"):
        for kw in (dict(), dict(exclude_seen=False)):
            want = _np(*eng.recommend_two_stage(feed, **dict(KW, **kw)))
            got = _call(eng, feed, 0.0, **kw)
            _same(got[:2], want, (scoring, state, sorted(kw)))
            assert (got[0] >= 0).all() and (got[2][:, 0] == 0).all() and (got[2] >= 0).all()      # (m is kept at mu = 0 too; it costs nothing)
            _same(_np(*eng.recommend_two_stage(feed, **dict(KW, **kw))), want, "the plain call behind the diversified one")
        for _ in range(3):
            eng.train_step(reference()["batch"])
    eng.check_forks()


def test_diversified_lists_pass_the_fp64_checks_and_diversify_returns_the_same_bytes():
    _need_gpu()
    eng, feed, mu = _engine(), _feed16(), 2.0
    topk, sc, msim = _call(eng, feed, mu, exclude_seen=False)
    g = eng.geo
    ids, exact, content = _np(eng.rt_ids[:NB], eng.rt_exact[:NB], eng.E[:N, g.ldh:g.ldh + g.H])
    assert content.shape == (N, H) and (content == reference()["content"][1:]).all()
    assert (ids >= 0).all() and all(len(set(r.tolist())) == SHORT for r in ids)
    order = rank_model(exact, ids)[1]
    tau = mu * TOL_SIM + 2.0 ** -23 * max(float(np.abs(exact).max()), mu)
    short, m64, count = tau_greedy(ids, exact, order, content, mu, topk)
    print("tau %.3e, largest shortfall of a pick %.3e, largest msim error %.3e (TOL_SIM %.3e)"
          % (tau, short.max(), np.abs(msim - m64).max(), TOL_SIM))
    assert (count == TOPK).all() and (short <= 2 * tau).all() and (np.abs(msim.astype(np.float64) - m64) <= TOL_SIM).all()
    want, _, _, gap = walk_f64(ids, exact, order, content, mu, TOPK)
    sure = gap > 2 * tau
    print("sessions left out of the comparison with walk_f64: %d of %d" % (int((~sure).sum()), NB))
    assert (~sure).sum() <= 2 and (topk[sure] == want[sure]).all()
    slot = [[int(np.where(ids[b] == i)[0][0]) for i in topk[b]] for b in range(NB)]
    assert sc.tobytes() == np.take_along_axis(exact, np.asarray(slot), 1).tobytes()            # the exact score of each pick, bit for bit
    plain = _np(*eng.recommend_two_stage(feed, exclude_seen=False, **KW))[0]
    assert (plain != topk).any()                                                              # the penalty moved something
    # the op-level form on the lists the call left: the same bytes, from host arrays and from the device views
    _same(_np(*eng.diversify(ids, exact, TOPK, mu)), (topk, sc, msim), "diversify (host arrays)")
    _call(eng, feed, mu, exclude_seen=False)
    _same(_np(*eng.diversify(eng.rt_ids[:NB], eng.rt_exact[:NB], k=TOPK, diversity=mu)), (topk, sc, msim), "diversify (device views)")
    eng.check_forks()


def test_no_list_holds_two_copies_of_one_story_once_the_penalty_exceeds_the_score_spread():
    """content in groups of 8 identical rows (one-hot: norm exactly 1), the groups on disjoint columns: cosines are exactly 1 and 0"""
    _need_gpu()
    content = np.zeros((N + 1, H), np.float32)
    content[1 + np.arange(N), np.arange(N) // 8] = 1.0
    eng, feed = _engine(content=content), _feed16()
    plain = _call(eng, feed, 0.0)[0]
    exact = _np(eng.rt_exact[:NB])[0]
    spread = float((exact.max(1) - exact.min(1)).max())
    mu = 1.01 * spread + 1e-3
    topk, _, msim = _call(eng, feed, mu)
    assert (topk >= 0).all() and (plain >= 0).all()
    pairs = lambda lists: [len(r) - len(set((r // 8).tolist())) for r in lists]      # noqa: E731
    assert sum(pairs(plain)) > 0, "no plain list holds two items of one group: the inputs show nothing"
    assert pairs(topk) == [0] * NB, pairs(topk)
    assert (msim == 0).all()                                                          # nothing listed had met a copy of itself
    eng.check_forks()


def test_a_live_content_update_gives_the_bytes_of_an_engine_built_from_the_final_tables():
    _need_gpu()
    r, feed, mu = reference(), _feed16(), 2.0
    eng = _engine()
    before = _call(eng, feed, mu)
    short = _np(eng.rt_ids[:NB])[0]
    # rows that ARE in the shortlists: the first picks of the first sessions become copies of the story session 0 lists first
    ids = np.unique(before[0][:8, :3].reshape(-1))
    ids = ids[ids != before[0][0, 0]].astype(np.int32)
    assert len(ids) >= 4 and all((short == i).any() for i in ids)
    new = np.repeat(r["content"][1 + before[0][0, 0]][None, :], len(ids), 0)
    eng.update_items(ids, content=new)
    after = _call(eng, feed, mu)
    final = r["content"].copy()
    final[1 + ids] = new
    _same(after, _call(_engine(content=final), feed, mu), "updated engine against one built from the final tables")
    assert (after[0] != before[0]).any()
    eng.check_forks()


@pytest.mark.parametrize("scoring", ["bf16x3-mixed", "f32"])
def test_ragged_feeds_return_the_bytes_of_the_rectangular_calls(scoring):
    _need_gpu()
    from tcar_amd.host.data import pack_sessions
    eng, mu = _engine(scoring), 2.0
    feed = {n: v for n, v in random_ragged(np.asarray([1, 2, 3, 4, 5] * 3, np.int32), 61).items() if n != "label"}
    got = _call(eng, feed, mu)
    assert got[0].shape == (15, TOPK) and (got[0] >= 0).all()
    for length in (1, 2, 3, 4, 5):
        idx, sub = group(feed, length)
        assert sub["seq"].shape == (3, length)
        _same([x[idx] for x in got], _call(eng, sub, mu), (scoring, "length", length))
    rect = _feed16()
    uniform = pack_sessions([rect])
    assert uniform["seq"].ndim == 1 and uniform["len"].tolist() == [3] * NB
    _same(_call(eng, uniform, mu), _call(eng, rect, mu), (scoring, "uniform"))
    eng.check_forks()


def test_window_and_exclusions_compose_with_the_walk():
    _need_gpu()
    eng, feed, mu = _engine(), _feed16(), 2.0
    keys, lo, hi = _keys_and_windows()
    lo, hi = lo[:NB], hi[:NB]
    eng.set_item_keys(keys)
    free = _call(eng, feed, mu, exclude_seen=False)[0]
    extra = np.full((NB, 4), -1, np.int32)
    extra[:, 0], extra[:, 2] = free[:, 0], free[:, 5]
    topk = _call(eng, feed, mu, exclude=extra, window=(lo, hi))[0]
    seen = reference()["batch"]["seq"][:NB].astype(np.int64) - 1
    for b in range(NB):
        t = topk[b][topk[b] >= 0]
        assert len(t) > 0 and len(set(t.tolist())) == len(t)
        assert not set(t.tolist()) & (set(extra[b].tolist()) | set(seen[b].tolist())), b
        assert ((lo[b] <= keys[t]) & (keys[t] < hi[b])).all(), b
        assert (topk[b][len(t):] == -1).all()
    # the same request through diversify on what it left: the same lists
    again = _np(*eng.diversify(eng.rt_ids[:NB], eng.rt_exact[:NB], TOPK, mu))[0]
    assert (again == topk).all()
    eng.check_forks()


def test_the_sharded_engine_refuses_the_keyword():
    _need_gpu()
    from tcar_amd import _lib
    from tcar_amd.sharded import ShardedEngine
    r = reference()
    eng = ShardedEngine(r["params"], r["content"], r["mw"], max_grad=2.0, scoring="bf16x3-mixed", world=1, rank=0)
    with pytest.raises(_lib.TcarError, match="diversity.*does not take the keyword"):
        eng.shard_recommend_two_stage(_feed16(), k=TOPK, shortlist=SHORT, diversity=1.0)
    with pytest.raises(_lib.TcarError, match="diversity.*does not take the keyword"):
        eng.recommend_two_stage(_feed16(), diversity=1.0)
    with pytest.raises(_lib.TcarError, match="diversify"):
        eng.diversify(np.zeros((2, 30), np.int32), np.zeros((2, 30), np.float32), 20, 1.0)


def test_the_model_reaches_the_diversified_call():
    _need_gpu()
    from tcar_amd.host.model import Seq2SeqAttNN, initial_variables
    from tcar_amd.host.synth import SynthFold
    fold = SynthFold(n_items=400, dim=32, n_train=300, n_test=200, seed=17, active_t=True)
    np.random.seed(3)
    args = fold.model_args(batch_size=64, epoch=1, neg_num=8, hidden_size=32, time_hidden_size=16, lr=0.003,
                           initial_variables=initial_variables(400, 32, 16, 0.3, 0.1), emb_stddev=0.3, stddev=0.1, scoring="bf16x3")
    with redirect_stdout(io.StringIO()):
        model = Seq2SeqAttNN(args)
    idx = np.where(fold.test.in_len == 3)[0][:4]
    assert len(idx) > 0
    feed = {n: v for n, v in fold.test.batch_arrays(idx, "active_t").items() if n not in ("label", "neg")}
    top, sc = _np(*model.recommend(feed, k=5, shortlist=128, diversity=1.0))
    want, want_sc = _np(*model.engine.recommend_two_stage(feed, k=5, shortlist=128, diversity=1.0))
    assert top.shape == (len(idx), 5) and (top == want).all() and sc.tobytes() == want_sc.tobytes()
    with pytest.raises(ValueError, match="diversity re-ranks the shortlist"):
        model.recommend(feed, k=5, diversity=1.0)


def test_eval_diversity_adds_one_line_to_the_test_loop_and_moves_nothing_else():
    _need_gpu()
    from tcar_amd.host.cli import main
    common = ["--synthetic", "400", "--synthetic_train", "1500", "--synthetic_test", "200", "--epoch", "1", "--hidden_size", "48",
              "--time_hidden_size", "16", "--batch_size", "64", "--eval_panel", "256", "--eval_shortlist", "80"]
    out = {}
    for flag in ((), ("--eval_diversity", "1.5")):
        buf = io.StringIO()
        with redirect_stdout(buf):
            model = main(common + list(flag))
        out[bool(flag)] = (buf.getvalue().splitlines(), dict(model.last_metrics))
    (plain, m0), (lines, m1) = out[False], out[True]
    new = [i for i, l in enumerate(lines) if l.startswith("diversified lists (shortlist 80, penalty 1.5): Recall@20: ")]
    assert len(new) == 1 and lines[new[0] - 1].startswith("two-stage lists (shortlist 80): Recall@20: ")
    assert lines[:new[0]] + lines[new[0] + 1:] == plain                    # every other line of the run, byte for byte
    d = m1.pop("diversified")
    assert m1 == m0 and d["shortlist"] == 80 and d["penalty"] == 1.5
    assert sorted(d) == ["content_ild", "ild", "penalty", "recall", "shortlist", "two_stage_content_ild", "two_stage_ild"]
    assert 0.0 <= d["recall"] <= 1.0 and 0.0 <= d["ild"] <= 1.0 and 0.0 <= d["two_stage_ild"] <= 1.0
    assert 0.0 < d["content_ild"] <= 2.0 and 0.0 < d["two_stage_content_ild"] <= 2.0
    assert lines[new[0]] == ("diversified lists (shortlist 80, penalty 1.5): Recall@20: {}, ILD: {}, content ILD: {} (two-stage lists: "
                             "ILD {}, content ILD {})").format(d["recall"], d["ild"], d["content_ild"], d["two_stage_ild"],
                                                               d["two_stage_content_ild"])
