"""Retrieval and the two-stage call at the engine level (TcarEngine.retrieve / recommend_two_stage; tcar_retrieve_step /
tcar_retrieve_rerank_step) on the reference setup of tests/serve_case.py: N = 700, B = 41, PANEL = 256.

Where the coarse precision is the engine's own (scoring "bf16": the hi planes; "f32") the panel GEMM is the one recommend() runs and
only the selector differs: the lists must be equal bit for bit.  On "bf16x3-mixed" the coarse scores come from the hi planes alone and
are held to the fp64 oracle in a BAND per entry,

    beta[b, n] = u * (|A| |E|^T)[b, n] + delta_b,        u = 2^-8,    delta_b = 1e-3 * max_n |s[b, n]|  (the project's logits gate),

with A the engine's fp32 attout and E its candidate rows, read back (E as hi + lo of its planes: on a split-bf16 engine the planes are
the candidate rows, the fp32 matrix's time block is not kept).  u: every pack kernel forms the hi plane as `(__bf16)x` (embed.hip,
gemm_bf16.hip, optim.hip, score.hip), a conversion that ROUNDS TO NEAREST even: each operand is off by at most 2^-9 relative, a
product of two by 2^-8 (1 + 2^-10) — the 2^-18 term and the fp32 accumulation are what delta_b is for.

(e) leaves out the sessions whose oracle gap between the k-th and the C-th best score is at most 2 max_n beta[b, n]; measured on
the CPU from the oracle alone (u = 2^-8, shortlist = 128): 0 of 41 sessions, the smallest margin 1.33 — the cap of 10 % holds."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401

from gpu_util import _kb32_index, _need_gpu, _np, close
from serve_case import B, N, PANEL, SHORT, TOPK, _feed, _keys_and_windows, reference
from serve_case import beta_of_operands as _beta
from serve_shapes_ref import check_band

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("scoring", ["bf16", "f32"])
def test_retrieve_equals_recommend_where_the_coarse_precision_is_the_engines_own(scoring):                   # (a)
    _need_gpu()
    from tcar_amd.engine import TcarEngine
    r = reference()
    feed = _feed()
    eng = TcarEngine(r["params"], r["content"], r["mw"], max_grad=2.0, scoring=scoring)
    keys, lo, hi = _keys_and_windows()
    eng.set_item_keys(keys)
    top = _np(*eng.recommend(feed, k=20, panel=PANEL))[0]
    extra = np.full((B, 5), -1, np.int32)
    extra[:, 0], extra[:, 2], extra[:, 3] = top[:, 0], top[:, 7], top[:, 0]
    for name, kw in (("plain", dict(exclude_seen=False)), ("exclude", dict(exclude_seen=True, exclude=extra)),
                     ("window", dict(exclude_seen=False, window=(lo, hi))), ("window + exclude", dict(exclude=extra, window=(lo, hi)))):
        want_ids, want_sc = _np(*eng.recommend(feed, k=64, panel=PANEL, **kw))
        ids, sc = _np(*eng.retrieve(feed, 64, panel=PANEL, **kw))
        assert ids.dtype == np.int32 and ids.shape == (B, 64) and sc.dtype == np.float32
        assert (ids == want_ids).all(), (scoring, name)
        live = ids >= 0
        assert sc[live].tobytes() == want_sc[live].tobytes(), (scoring, name)
        assert (sc[~live] == -np.inf).all()
        if "window" in name:
            assert (~live).any() and live.any()
    eng.check_forks()


_MIXED = {}


@pytest.fixture(scope="module")
def mixed():
    """every call of the bf16x3-mixed engine, once: numpy copies of what came back"""
    _need_gpu()
    if _MIXED:
        return _MIXED
    from tcar_amd.engine import TcarEngine
    r = reference()
    feed = _feed()
    eng = TcarEngine(r["params"], r["content"], r["mw"], max_grad=2.0, scoring="bf16x3-mixed")
    eng.eval_step_streamed(r["batch"], k=TOPK)
    eng.logits.fill_(float("nan"))
    m = _MIXED
    m["ids"], m["coarse"] = _np(*eng.retrieve(feed, SHORT, exclude_seen=False, panel=PANEL))
    g = eng.geo
    m["A"] = eng.attout[:B].cpu().numpy().astype(np.float64)
    idx = torch.tensor(_kb32_index(eng.e16h.shape[0], g.ek)[:N], device=eng.dev)
    m["E"] = (eng.e16h.flatten()[idx].double() + eng.e16l.flatten()[idx].double()).cpu().numpy()
    m["ids_again"], m["coarse_again"] = _np(*eng.retrieve(feed, SHORT, exclude_seen=False, panel=PANEL))
    m["ids_1panel"], m["coarse_1panel"] = _np(*eng.retrieve(feed, SHORT, exclude_seen=False))
    m["seen_ids"], m["seen_coarse"] = _np(*eng.retrieve(feed, 1024, panel=PANEL))                      # (c): C > N, seen items excluded
    m["exact"] = _np(eng.score_candidates(feed, m["ids"]).scores)[0]
    m["top"], m["top_sc"] = _np(*eng.recommend_two_stage(feed, k=TOPK, shortlist=SHORT, exclude_seen=False, panel=PANEL))
    m["short_of_two"] = _np(eng.rt_ids[:B], eng.rt_exact[:B])
    m["top_again"], m["top_sc_again"] = _np(*eng.recommend_two_stage(feed, k=TOPK, shortlist=SHORT, exclude_seen=False, panel=PANEL))
    m["logits_nan"] = bool(torch.isnan(eng.logits).all())
    eng.check_forks()                                                                                     # (g)
    return m


def test_the_read_back_operands_are_the_oracles(mixed):
    """A E^T is the oracle's score matrix to the logits gate: the band below is built from the operands the engine scored"""
    close(mixed["A"] @ mixed["E"].T, reference()["s"], name="A E^T")


def test_the_coarse_shortlist_holds_what_the_oracle_puts_clearly_inside(mixed):                          # (b)
    s, beta = reference()["s"], _beta(mixed)
    ids, coarse = mixed["ids"], mixed["coarse"]
    assert ids.shape == (B, SHORT) and (ids >= 0).all() and (ids < N).all()
    for b in range(B):
        t = ids[b].astype(np.int64)
        assert len(set(t.tolist())) == SHORT, b                                        # distinct
        cth = np.sort(s[b])[-SHORT]
        must = np.where(s[b] > cth + 2 * beta[b])[0]
        assert set(must.tolist()) <= set(t.tolist()), (b, sorted(set(must.tolist()) - set(t.tolist())))
        assert (s[b, t] >= cth - 2 * beta[b, t]).all(), b                              # nothing clearly below the C-th best
        err = np.abs(coarse[b].astype(np.float64) - s[b, t])
        assert (err <= beta[b, t]).all(), (b, float((err / beta[b, t]).max()))
        assert (coarse[b, :-1] >= coarse[b, 1:]).all(), b
        ties = coarse[b, :-1] == coarse[b, 1:]
        assert (t[:-1][ties] > t[1:][ties]).all(), b
    # the coarse scores are NOT the exact ones: the hi planes alone were contracted
    assert np.abs(coarse - mixed["exact"]).max() > 0


def test_a_shortlist_longer_than_the_pool_lists_every_eligible_item_once(mixed):                        # (c)
    ids, coarse = mixed["seen_ids"], mixed["seen_coarse"]
    seen = reference()["batch"]["seq"].astype(np.int64) - 1
    assert ids.shape == (B, 1024)
    for b in range(B):
        pool = np.setdiff1d(np.arange(N), seen[b])
        n = len(pool)
        assert sorted(ids[b, :n].tolist()) == pool.tolist(), b
        assert (ids[b, n:] == -1).all() and (coarse[b, n:] == -np.inf).all() and np.isfinite(coarse[b, :n]).all(), b
        assert (coarse[b, :n - 1] >= coarse[b, 1:n]).all(), b
        ties = coarse[b, :n - 1] == coarse[b, 1:n]
        assert (ids[b, :n - 1][ties] > ids[b, 1:n][ties]).all(), b


def test_the_two_stage_list_is_the_top_k_of_the_exact_scores_over_the_shortlist(mixed):                 # (d)
    ids, exact = mixed["ids"], mixed["exact"]
    sid, sexact = mixed["short_of_two"]
    assert (sid == ids).all() and sexact.tobytes() == exact.tobytes()                 # the call's own shortlist and exact scores
    top, top_sc = mixed["top"], mixed["top_sc"]
    assert top.shape == (B, TOPK) and top.dtype == np.int32
    for b in range(B):
        order = np.lexsort((ids[b], exact[b]))[::-1][:TOPK]                            # score, then id, descending
        assert (top[b] == ids[b, order]).all(), b
        assert top_sc[b].tobytes() == exact[b, order].tobytes(), b


def test_the_two_stage_list_passes_the_band_of_the_streamed_lists(mixed):                               # (e)
    r = reference()
    s, beta = r["s"], _beta(mixed)
    srt = -np.sort(-s, 1)
    keep = srt[:, TOPK - 1] - srt[:, SHORT - 1] > 2 * beta.max(1)
    assert (~keep).mean() <= 0.10, (~keep).mean()
    check_band(s[keep], r["delta"][keep], mixed["top"][keep], TOPK, name="two-stage")
    close(mixed["top_sc"][keep], np.take_along_axis(s, mixed["top"].astype(np.int64), 1)[keep], name="two-stage scores")


def test_logits_stay_untouched_and_two_calls_give_equal_bits(mixed):                                     # (f), (g)
    assert mixed["logits_nan"]
    assert mixed["ids_again"].tobytes() == mixed["ids"].tobytes() and mixed["coarse_again"].tobytes() == mixed["coarse"].tobytes()
    assert mixed["top_again"].tobytes() == mixed["top"].tobytes() and mixed["top_sc_again"].tobytes() == mixed["top_sc"].tobytes()
    # one panel instead of three is another launch geometry of the GEMM: the same band, not the same bits
    s, beta = reference()["s"], _beta(mixed)
    t = mixed["ids_1panel"].astype(np.int64)
    assert (np.abs(mixed["coarse_1panel"] - np.take_along_axis(s, t, 1)) <= np.take_along_axis(beta, t, 1)).all()


def test_a_sharded_engine_refuses_both_calls():
    _need_gpu()
    from tcar_amd import _lib
    from tcar_amd.sharded import ShardedEngine
    r = reference()
    eng = ShardedEngine(r["params"], r["content"], r["mw"], max_grad=2.0, scoring="bf16x3-mixed", world=1, rank=0)
    with pytest.raises(_lib.TcarError, match="whole catalog on one engine"):
        eng.retrieve(_feed(), 64)
    with pytest.raises(_lib.TcarError, match="whole catalog on one engine"):
        eng.recommend_two_stage(_feed())


def test_the_model_reaches_both_calls_and_leaves_recommend_without_a_shortlist_alone():
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
    ids, coarse = _np(*model.retrieve(feed, 70))
    assert ids.shape == coarse.shape == (len(idx), 70) and all(len(set(r.tolist())) == 70 for r in ids) and ids.min() >= 0
    top, sc = _np(*model.recommend(feed, k=5, shortlist=70))
    want, want_sc = _np(*model.engine.recommend_two_stage(feed, k=5, shortlist=70))
    assert top.shape == (len(idx), 5) and (top == want).all() and sc.tobytes() == want_sc.tobytes()
    assert all(set(t.tolist()) <= set(r.tolist()) for t, r in zip(top, ids))
    plain, plain_sc = _np(*model.recommend(feed, k=5))                         # no shortlist: the streamed selection, as before
    eng_top, eng_sc = _np(*model.engine.recommend(feed, k=5))
    assert (plain == eng_top).all() and plain_sc.tobytes() == eng_sc.tobytes()


def test_eval_shortlist_adds_one_line_to_the_test_loop_and_moves_nothing_else():                         # (h)
    _need_gpu()
    from tcar_amd.host.cli import main
    common = ["--synthetic", "400", "--synthetic_train", "1500", "--synthetic_test", "200", "--epoch", "1", "--hidden_size", "48",
              "--time_hidden_size", "16", "--batch_size", "64", "--eval_panel", "256"]
    out = {}
    for flag in ((), ("--eval_shortlist", "80")):
        buf = io.StringIO()
        with redirect_stdout(buf):
            model = main(common + list(flag))
        out[bool(flag)] = (buf.getvalue().splitlines(), dict(model.last_metrics))
    (plain, m0), (lines, m1) = out[False], out[True]
    new = [i for i, l in enumerate(lines) if l.startswith("two-stage lists (shortlist 80): Recall@20: ")]
    assert len(new) == 1 and lines[new[0] - 1].startswith("MRR@20: ")
    assert lines[:new[0]] + lines[new[0] + 1:] == plain                    # every earlier (and later) line, byte for byte
    t = m1.pop("two_stage")
    assert m1 == m0 and sorted(t) == ["agreement", "recall", "shortlist"] and t["shortlist"] == 80
    assert 0.0 <= t["recall"] <= 1.0 and 0.0 <= t["agreement"] <= 1.0
    assert lines[new[0]] == "two-stage lists (shortlist 80): Recall@20: {}, agreement with the streamed lists: {}".format(
        t["recall"], t["agreement"])
