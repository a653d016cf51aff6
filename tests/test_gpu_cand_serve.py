"""Candidate-list scoring at the engine level (TcarEngine.score_candidates, tcar_cand_step) against the fp64 oracle, on the reference
setup of tests/serve_case.py.  The engine's scores differ from the oracle's by rounding, so ranks and pair counts are checked in
BANDS of delta_b = 1e-3 * max_n |s[b, n]| — the project's logits gate — in which no session and no slot is left out."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401

from gpu_util import _need_gpu, close
from serve_case import B, C_, N, TOPK, _lists, reference

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("scoring", ["f32", "bf16x3-mixed"])
def test_candidate_scores_ranks_and_pair_counts_match_the_oracle_in_bands(scoring):
    _need_gpu()
    from tcar_amd.engine import TcarEngine
    from tcar_amd.host import metrics as M
    r = reference()
    s, delta, batch = r["s"], r["delta"], r["batch"]
    cand, clicked = _lists()
    live = (cand >= 0) & (cand < N)
    assert (~live).sum() == 3 * B
    eng = TcarEngine(r["params"], r["content"], r["mw"], max_grad=2.0, scoring=scoring)
    _, topk, _ = eng.eval_step_streamed(batch, k=TOPK)
    topk, top_scores = topk.cpu().numpy().copy(), eng.last_scores.cpu().numpy().copy()
    eng.logits.fill_(float("nan"))
    feed = {n: v for n, v in batch.items() if n not in ("label", "neg")}           # no label, no negatives in the feed
    res = eng.score_candidates(feed, cand, clicked)
    got = [t.cpu().numpy().copy() for t in res]
    scores, rank_of, order, counts, metrics = got
    assert bool(torch.isnan(eng.logits).all())                                                              # (e)
    assert scores.shape == (B, C_) and rank_of.dtype == np.int32 and counts.shape == (B, 3) and metrics.shape == (B, 3)
    want = np.take_along_axis(s, np.where(live, cand, 0).astype(np.int64), 1)
    assert (scores[~live] == -np.inf).all() and (rank_of[~live] == 0).all()
    close(scores[live], want[live], name="scores")                                                          # (a)
    for b in range(B):
        slots, d2 = np.where(live[b])[0], 2 * delta[b]
        sb = want[b, slots]
        lo = 1 + (sb[None, :] > sb[:, None] + d2).sum(1)
        hi = 1 + ((sb[None, :] > sb[:, None] - d2) & ~np.eye(len(slots), dtype=bool)).sum(1)
        rk = rank_of[b, slots]
        assert ((lo <= rk) & (rk <= hi)).all(), (b, rk, lo, hi)                                             # (b)
        assert sorted(rk.tolist()) == list(range(1, len(slots) + 1))
        assert (rank_of[b, order[b, :len(slots)]] == np.arange(1, len(slots) + 1)).all() and (order[b, len(slots):] == -1).all()
        pos, neg = want[b, slots[clicked[b, slots] != 0]], want[b, slots[clicked[b, slots] == 0]]
        assert counts[b, 0] == len(pos) and counts[b, 1] == len(neg)
        lo2, hi2 = 2 * (pos[:, None] > neg[None, :] + d2).sum(), 2 * (pos[:, None] > neg[None, :] - d2).sum()
        assert lo2 <= counts[b, 2] <= hi2, (b, lo2, counts[b, 2], hi2)                                      # (c)
    auc, mrr, n5, n10 = M.impression_metrics(counts, metrics)
    for x in (auc, mrr, n5, n10):
        assert np.isfinite(x).all() and ((0 <= x) & (x <= 1)).all()
    # (d) the streamed step's own lists, scored again as candidates: the same items, another kernel
    again = eng.score_candidates(feed, topk).scores.cpu().numpy()
    close(again, top_scores, name="top-20 scored as candidates")
    # (f) two calls give equal bits (bt= a resident batch this time)
    bt = eng.upload(batch)
    for a, t in zip(got, eng.score_candidates(None, cand, clicked, bt=bt)):
        assert a.tobytes() == t.cpu().numpy().tobytes()
    unlabelled = eng.score_candidates(feed, cand)
    assert unlabelled.counts is None and unlabelled.metrics is None
    assert unlabelled.rank_of.cpu().numpy().tobytes() == rank_of.tobytes() and unlabelled.scores.cpu().numpy().tobytes() == scores.tobytes()
    eng.check_forks()


def test_a_sharded_engine_refuses_candidate_scoring():                                                      # (g)
    _need_gpu()
    from tcar_amd import _lib
    from tcar_amd.sharded import ShardedEngine
    r = reference()
    eng = ShardedEngine(r["params"], r["content"], r["mw"], max_grad=2.0, scoring="bf16x3-mixed", world=1, rank=0)
    with pytest.raises(_lib.TcarError, match="whole catalog on one engine"):
        eng.score_candidates(r["batch"], np.zeros((B, 4), np.int32))


def test_eval_candidates_adds_one_line_to_the_test_loop_and_moves_nothing_else():
    _need_gpu()
    from tcar_amd.host.cli import main
    common = ["--synthetic", "400", "--synthetic_train", "1500", "--synthetic_test", "200", "--epoch", "1", "--hidden_size", "48",
              "--time_hidden_size", "16", "--batch_size", "64"]
    out = {}
    for flag in ((), ("--eval_candidates", "16")):
        buf = io.StringIO()
        with redirect_stdout(buf):
            model = main(common + list(flag))
        out[bool(flag)] = (buf.getvalue().splitlines(), dict(model.last_metrics))
    (plain, m0), (lines, m1) = out[False], out[True]
    new = [i for i, l in enumerate(lines) if l.startswith("candidates (16 per session): AUC: ")]
    assert len(new) == 1 and lines[new[0] - 1].startswith("MRR@20: ")
    assert lines[:new[0]] + lines[new[0] + 1:] == plain                    # every earlier (and later) line, byte for byte
    c = m1.pop("candidates")
    assert m1 == m0 and sorted(c) == ["auc", "mrr", "ndcg10", "ndcg5"]
    assert all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in c.values())
    assert lines[new[0]] == "candidates (16 per session): AUC: {}, MRR: {}, nDCG@5: {}, nDCG@10: {}".format(c["auc"], c["mrr"], c["ndcg5"], c["ndcg10"])
