"""Every serving call — eval_step_streamed, recommend, score_candidates, retrieve, recommend_two_stage and the ragged forms —
against the fp64 oracle at the edge shapes of tests/serve_shapes_ref.py (CASES), on a fresh engine (phase A) and on an engine that
has just trained (phase B).  Cases, references, gates and checkers are that module's; tests/test_serve_shapes_ref.py shows on the
CPU that the checkers refuse the mistakes this file is after.

Phase A, one engine per (case, scoring): every call at every panel width of the case against the oracle of the initial variables;
where a case has two panel widths, topk, scores and rank of both partitions are equal bit for bit (include/tcar_serve.h).
Phase B: two train_step(batch, defer_update=True) on a TcarEngine in its default form, then — no materialised eval_step in between,
the candidate-time planes still stale — the serving calls against a TcarOracle built from the engine's own export_params(), and a
third training step whose loss is held to the oracle trained from the initial variables (1e-3 in f32, 1e-2 in bf16x3-mixed, the gates
of tests/test_gpu_parity.py::test_step_matches_oracle).

Rule (e) of the two-stage check (kept_sessions) leaves out NO session of any case, measured on the CPU from the oracle alone and
pinned in tests/test_serve_shapes_ref.py: the smallest margins gap / (2 max beta), split-bf16 band / fp32 band, are one inf / inf
(C = 128 > N: the shortlist is the catalog), block+1 18.1 / 416, tile+1 4.61 / 90.4, long 10.3 / 140, exact 5.84 / 127,
wide 7.81 / 168.

Measured on an MI355X: every test passes, the two partitions of `tile+1` (panel 128 and one panel of 1,024) included, and the
whole file takes 4.5 s in one process, the slowest test 0.5 s (a test alone in a fresh process: 2 to 3 s, the imports).  Worst error / bound per call and
case, fp32 engine / split-bf16 engines (the larger of bf16x3-mixed and bf16x3 where both run); the band rules (a)-(e) and the bit
equalities have no ratio, they hold or they do not:

    phase A      eval scores      eval ce          recommend        candidates       coarse / beta    two-stage
    one          0.0005 / 0.026   0.0000 / 0.0014  0.0040 / 0.073   0.0019 / 0.058   0.0002 / 0.26    0.0004 / 0.027
    block+1      0.0026 / 0.022   0.0016 / 0.0064  0.0026 / 0.022   0.0098 / 0.22    0.0024 / 0.14    0.0011 / 0.022
    tile+1       0.0022 / 0.0094  0.0006 / 0.0083  0.0022 / 0.0094  0.015  / 0.22    0.0019 / 0.17    0.0007 / 0.0093
    long         0.0007 / 0.0038  0.0001 / 0.0006  0.0007 / 0.0038  0.0032 / 0.071   0.0006 / 0.21    0.0001 / 0.0038
    exact        0.0012 / 0.0070  0.0001 / 0.0009  0.0012 / 0.0070  0.0099 / 0.071   0.0009 / 0.11    0.0004 / 0.0074
    wide         0.0022 / 0.011   0.0006 / 0.0056  0.0022 / 0.011   0.0094 / 0.10    0.0018 / 0.12    0.0009 / 0.011
    ragged       eval scores      eval ce          recommend
    one          0.0005 / 0.026   0.0000 / 0.0014  0.0040 / 0.073
    block+1      0.0026 / 0.021   0.0012 / 0.0093  0.0026 / 0.021
    tile+1       0.0024 / 0.011   0.0011 / 0.0086  0.0024 / 0.011
    long         0.0007 / 0.0044  0.0001 / 0.0005  0.0007 / 0.0044
    exact        0.0012 / 0.0064  0.0003 / 0.0014  0.0012 / 0.0064
    wide         0.0021 / 0.011   0.0007 / 0.0075  0.0021 / 0.011
    phase B      eval scores      eval ce          recommend        candidates       coarse / beta      (f32 / bf16x3-mixed)
    one          0.0009 / 0.032   0.0000 / 0.0003  0.0015 / 0.078   0.0008 / 0.071   0.0001 / 0.23
    block+1      0.0025 / 0.021   0.0017 / 0.011   0.0025 / 0.021   0.0094 / 0.21    0.0020 / 0.15
    tile+1       0.0021 / 0.011   0.0009 / 0.013   0.0021 / 0.011   0.014  / 0.24    0.0019 / 0.16
    long         0.0005 / 0.0045  0.0001 / 0.0003  0.0005 / 0.0045  0.0030 / 0.14    0.0005 / 0.18
    exact        0.0019 / 0.0087  0.0006 / 0.0027  0.0019 / 0.0087  0.0069 / 0.17    0.0013 / 0.12
    wide         0.0020 / 0.011   0.0046 / 0.0078  0.0020 / 0.011   0.012  / 0.14    0.0014 / 0.11

Every test prints its worst ratios (pytest -s)."""
import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401

import serve_shapes_ref as R
from gpu_util import _need_gpu, _np, close

pytestmark = pytest.mark.gpu

K = R.TOPK


def _engine(name, scoring):
    from tcar_amd.engine import TcarEngine
    params, content, mw, _ = R.inputs(name)
    return TcarEngine(params, content, mw, max_grad=2.0, scoring=scoring)


def _same_bits(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, i)


def _streamed_eval(eng, feed, panel):
    rank, topk, ce = eng.eval_step_streamed(feed, k=K, panel=panel)
    return _np(rank, topk, ce, eng.last_scores)


def _rectangular_calls(eng, name, ref, scoring):
    """items 1-4: eval_step_streamed, recommend, score_candidates and retrieve of the case's batch against `ref`"""
    c = R.CASES[name]
    batch = R.inputs(name)[3]
    feed = R.unlabelled(batch)
    split = scoring != "f32"
    C = R.shortlist_size(name)
    eng._ensure_work(c.B, c.T)                         # (allocates the [B, N] matrix the serving calls must not touch)
    eng.logits.fill_(float("nan"))
    ev = {}
    for panel in c.panels:
        tag = "%s %s panel %s" % (ref["name"], scoring, panel)
        ev[panel] = rank, topk, ce, scores = _streamed_eval(eng, batch, panel)
        R.check_eval(ref, rank, topk, ce, scores, k=K, name="eval " + tag)
        tk, sc = _np(*eng.recommend(feed, k=K, panel=panel))
        R.check_recommend(ref, tk, sc, k=K, name="recommend " + tag)
        ids, coarse = _np(*eng.retrieve(feed, C, panel=panel, exclude_seen=False))
        R.check_coarse(ref, ids, coarse, C, split, name="retrieve " + tag)
        if not split:                  # the coarse precision is the engine's own: the streamed selection over the same panel GEMM
            kk = min(64, C)
            want_ids, want_sc = _np(*eng.recommend(feed, k=kk, panel=panel, exclude_seen=False))
            live = want_ids >= 0
            assert (ids[:, :kk] == want_ids).all() and coarse[:, :kk][live].tobytes() == want_sc[live].tobytes(), tag
    if len(c.panels) == 2:             # a total order: the same lists, scores and ranks from every partition of the catalog
        a, b = (ev[p] for p in c.panels)
        _same_bits((a[1], a[3], a[0]), (b[1], b[3], b[0]), "%s %s: topk, scores, rank of two partitions" % (ref["name"], scoring))
    if name == "one":                  # k = 64 > N: every unseen item, then -1
        tk, sc = _np(*eng.recommend(feed, k=64, panel=c.panels[0]))
        n = c.N - len(set(batch["seq"][0].tolist()))
        assert (tk[0, :n] >= 0).all() and (tk[0, n:] == -1).all(), tk
        R.check_recommend(ref, tk, sc, k=64, short=True, name="recommend, k = 64")
    for width in (1, 65):
        cand = R.candidate_lists(name, width)
        res = eng.score_candidates(feed, cand)
        R.check_candidates(ref, cand, *_np(res.scores, res.rank_of, res.order), name="candidates %s %s C = %d" % (ref["name"], scoring, width))
    assert bool(torch.isnan(eng.logits).all())


@pytest.mark.parametrize("name,scoring", R.SCORINGS)
def test_a_fresh_engine_serves_every_call_as_the_oracle_scores_it(name, scoring):
    _need_gpu()
    from tcar_amd.host.data import pack_sessions
    c = R.CASES[name]
    ref = R.reference(name)
    eng = _engine(name, scoring)
    assert eng.geo.ek == 2 * ((c.H + 63) // 64 * 64) + 320 and eng.default_panel() == eng.geo.Npad
    _rectangular_calls(eng, name, ref, scoring)
    batch = R.inputs(name)[3]
    feed = R.unlabelled(batch)
    split = scoring != "f32"
    C = R.shortlist_size(name)
    for panel in c.panels:                                                                       # item 5
        top, top_sc = _np(*eng.recommend_two_stage(feed, k=K, shortlist=C, panel=panel, exclude_seen=False))
        rt_ids, rt_exact = _np(eng.rt_ids[:c.B], eng.rt_exact[:c.B])
        R.check_two_stage(ref, top, top_sc, rt_ids, rt_exact, K, C, split, name="two-stage %s %s panel %s" % (name, scoring, panel))
    rr = R.ragged_reference(name)                                                                # item 6
    ragged = pack_sessions(rr["feeds"])
    assert ragged["len"].tolist() == rr["lens"].tolist() and ragged["seq"].ndim == 1
    for panel in c.panels:
        rank, topk, ce, scores = got = _streamed_eval(eng, ragged, panel)
        R.check_eval(rr, rank, topk, ce, scores, k=K, name="ragged eval %s %s panel %s" % (name, scoring, panel))
        tk, sc = rec = _np(*eng.recommend(R.unlabelled(ragged), k=K, panel=panel))
        R.check_recommend(rr, tk, sc, k=K, name="ragged recommend %s %s panel %s" % (name, scoring, panel))
        if c.B == 1:                   # a single length: the rectangular call's bits
            _same_bits(got, _streamed_eval(eng, batch, panel), "ragged eval, one length")
            _same_bits(rec, _np(*eng.recommend(feed, k=K, panel=panel)), "ragged recommend, one length")
    assert bool(torch.isnan(eng.logits).all())
    eng.check_forks()
    print({k: round(v, 4) for k, v in R.WORST.items() if k.startswith(name)})


@pytest.mark.parametrize("name,scoring", R.TRAINED)
def test_an_engine_that_has_just_trained_serves_from_the_planes_of_its_own_variables(name, scoring):
    _need_gpu()
    batch = R.inputs(name)[3]
    eng = _engine(name, scoring)
    for _ in range(2):
        loss = eng.train_step(batch, defer_update=True)
    assert bool(torch.isfinite(loss).all())
    assert eng._time_dirty and eng._pending_lr is not None          # the candidate-time planes are stale, the second update is owed
    params = eng.export_params()                                    # (flushes the owed update)
    assert eng._time_dirty
    ref = dict(R.reference(name, params), name=name + ", trained")
    untrained = R.reference(name)
    assert np.abs(ref["s"] - untrained["s"]).max() > 4 * ref["delta"].max()      # training moved the scores out of the bands
    _rectangular_calls(eng, name, ref, scoring)
    assert not eng._time_dirty
    # serving left the training state intact: the third step follows the oracle trained from the initial variables
    loss3 = eng.train_step(batch, defer_update=True).cpu().numpy().copy()
    assert np.isfinite(loss3).all()
    close(loss3, R.trained_reference(name)["loss3"], rtol=1e-2 if scoring == "bf16x3-mixed" else 1e-3, name="the third step's loss")
    eng.flush()
    eng.check_forks()
    print({k: round(v, 4) for k, v in R.WORST.items() if k.startswith(name + ", trained")})
