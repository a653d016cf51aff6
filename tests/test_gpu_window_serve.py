"""Publish-time windows at the engine level (TcarEngine.eval_step_streamed / recommend with window=, tcar_serve_step_window) against
the fp64 oracle, and through Seq2SeqAttNN.test() with fresh_hours.  Shape, reference and bands are those of
test_gpu_serve.py, kept in tests/window_case.py: delta_b = 1e-3 * max_n |s[b, n]|, every check restricted to the session's POOL — the
items whose key lies in its window, and its label."""
import copy
import random

import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401

from gpu_util import _need_gpu
from window_case import B, I32_MAX, I32_MIN, N, PANEL, TOPK, check_band, check_eval, reference, run_test, trained

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("scoring", ["f32", "bf16x3-mixed"])
def test_windowed_evaluation_and_recommendation_match_the_oracle_in_bands(scoring):
    _need_gpu()
    from tcar_amd.engine import TcarEngine
    r = reference()
    batch, lab, key, win = r["batch"], r["batch"]["label"], r["key"], r["win"]
    eng = TcarEngine(r["params"], r["content"], r["mw"], max_grad=2.0, scoring=scoring)
    feed = {n: v for n, v in batch.items() if n not in ("label", "neg")}
    with pytest.raises(ValueError, match="set_item_keys"):
        eng.recommend(feed, k=TOPK, panel=PANEL, window=(0, 10))             # a window without keys
    with pytest.raises(ValueError):
        eng.set_item_keys(key[:-1])
    eng.set_item_keys(key)
    with pytest.raises(ValueError, match="window"):
        eng.recommend(feed, k=TOPK, panel=PANEL, window=(np.zeros(B + 1, np.int32), 10))
    eng.eval_step(batch, k=TOPK)
    eng.logits.fill_(float("nan"))

    # recommendation: a window that holds everything changes no bit
    tk0, sc0 = (x.cpu().numpy().copy() for x in eng.recommend(feed, k=TOPK, panel=PANEL))
    tk1, sc1 = (x.cpu().numpy().copy() for x in eng.recommend(feed, k=TOPK, panel=PANEL, window=(I32_MIN, I32_MAX)))
    assert (tk0 == tk1).all() and sc0.tobytes() == sc1.tobytes()
    # ... and a window is the exclusion of every item outside it
    X = int((~win).sum(1).max())
    out = np.full((B, X), -1, np.int32)
    for b in range(B):
        ids = np.where(~win[b])[0]
        out[b, :len(ids)] = ids
    tkw, scw = (x.cpu().numpy().copy() for x in eng.recommend(feed, k=TOPK, panel=PANEL, exclude_seen=False, window=(r["lo"], r["hi"])))
    tkx, scx = (x.cpu().numpy().copy() for x in eng.recommend(feed, k=TOPK, panel=PANEL, exclude_seen=False, exclude=out))
    assert (tkw == tkx).all() and (scw.view(np.int32)[tkw >= 0] == scx.view(np.int32)[tkx >= 0]).all()
    assert ((tkw >= 0).sum(1) == np.minimum(win.sum(1), TOPK)).all() and (tkw[3::4] == -1).all()
    check_band(r["s"], r["delta"], tkw, TOPK, win, name="recommend, window")
    # exclusions on top: the session's own items leave the windowed list
    tks, _ = eng.recommend(feed, k=TOPK, panel=PANEL, window=(r["lo"], r["hi"]))
    tks = tks.cpu().numpy().copy()
    seen = (batch["seq"] - 1).astype(np.int64)
    unseen = win.copy()
    for b in range(B):
        unseen[b, seen[b]] = False
        assert not set(tks[b].tolist()) & set(seen[b].tolist()), b
    check_band(r["s"], r["delta"], tks, TOPK, unseen, name="recommend, window + seen")

    # evaluation inside the pools (the window or the label), per-session windows and a scalar one
    pool = win | (np.arange(N)[None, :] == lab[:, None])
    rank, topk, ce = eng.eval_step_streamed(batch, k=TOPK, panel=PANEL, window=(r["lo"], r["hi"]))
    rank, topk, ce, scores = rank.cpu().numpy().copy(), topk.cpu().numpy().copy(), ce.cpu().numpy().copy(), eng.last_scores.cpu().numpy().copy()
    check_eval(r, pool, rank, topk, ce, scores, "eval, windows by session")
    none = np.arange(B) % 4 == 3
    assert (rank[none] == 1).all() and (topk[none, 0] == lab[none]).all() and (topk[none, 1:] == -1).all()
    assert (np.abs(ce[none]) <= 2 * r["delta"][none]).all()                  # the label alone: its two scores agree within the band
    third = (int(r["lo"][1]), int(r["hi"][1]))
    pool3 = np.broadcast_to(win[1], (B, N)) | (np.arange(N)[None, :] == lab[:, None])
    rank, topk, ce = eng.eval_step_streamed(batch, k=TOPK, panel=PANEL, window=third)
    check_eval(r, pool3, rank.cpu().numpy().copy(), topk.cpu().numpy().copy(), ce.cpu().numpy().copy(), eng.last_scores.cpu().numpy().copy(),
               "eval, one window for all")
    rank, topk, ce = eng.eval_step_streamed(batch, k=TOPK, window=third)      # the default panel: one fold
    check_eval(r, pool3, rank.cpu().numpy().copy(), topk.cpu().numpy().copy(), ce.cpu().numpy().copy(), eng.last_scores.cpu().numpy().copy(),
               "eval, one window for all, default panel")
    assert bool(torch.isnan(eng.logits).all())                    # no call above needs or writes the [B, N] matrix
    eng.set_item_keys(None)
    with pytest.raises(ValueError, match="set_item_keys"):
        eng.eval_step_streamed(batch, k=TOPK, panel=PANEL, window=third)
    eng.check_forks()


def test_fresh_hours_that_hold_every_item_reproduce_the_unwindowed_metrics():
    _need_gpu()
    t = trained()
    model, args = t["models"]["early"]
    plain, text0 = run_test(model, t["te"], args)
    fresh, text1 = run_test(model, t["te"], dict(args, fresh_hours=1e6))
    assert fresh.pop("labels_outside") == 0.0 and "labels outside their window: 0.0" in text1
    assert fresh == plain and "labels outside" not in text0          # exactly: every metric, the coverage included
    assert text1.replace("labels outside their window: 0.0\n", "") == text0


def test_narrow_fresh_hours_against_a_host_recomputation_from_the_datetimes():
    _need_gpu()
    from tcar_amd.host import metrics as M
    t = trained()
    fold, te, own = t["fold"], t["te"], t["own"]
    model, args = t["models"]["own"]
    hours = 120
    got, text = run_test(model, te, dict(args, fresh_hours=hours))
    # the windows again, in Python datetimes: minutes since the earliest publish time, [click + 1 - 60 hours, click + 1)
    t0 = min(own)
    minute = lambda when: int((when - t0).total_seconds() // 60)
    keys = np.array([minute(p) for p in own], np.int64)
    random.seed(11)
    sampler = model._sampler((copy.deepcopy(te[0]), te[1], te[2]))
    hits, mrrs, ndcgs, losses, outside = [], [], [], [], []
    while sampler.has_next():
        feed = sampler.next_batch_arrays()
        Tn = feed["seq"].shape[1]
        hi = np.array([minute(te[2][key][Tn]["click_t"]) + 1 for key in feed["keys"]], np.int64)
        lo = hi - 60 * hours
        kl = keys[feed["label"]]
        outside += (~((lo <= kl) & (kl < hi))).tolist()
        rank, topk, ce = model.engine.eval_step_streamed(feed, k=20, panel=128, window=(lo, hi))
        h, m, n = M.metrics_from_ranks(rank.cpu().numpy(), 20)
        hits += h.tolist()
        mrrs += m.tolist()
        ndcgs += n.tolist()
        losses += ce.cpu().numpy().tolist()
        tk = topk.cpu().numpy()
        pool = ((lo[:, None] <= keys[None, :]) & (keys[None, :] < hi[:, None])) | (np.arange(400)[None, :] == feed["label"][:, None])
        assert ((tk >= 0).sum(1) == np.minimum(pool.sum(1), 20)).all()
        assert all(pool[b][tk[b][tk[b] >= 0]].all() for b in range(len(tk)))          # nothing from outside a pool is recommended
    n = len(hits)
    assert n == fold.test.n and 0 < sum(outside) < n
    assert got["labels_outside"] == sum(outside) / n
    assert "labels outside their window: {}".format(sum(outside) / n) in text
    assert got["recall"] == float(np.sum(hits)) / n and got["mrr"] == float(np.sum(mrrs)) / n and got["ndcg"] == float(np.sum(ndcgs)) / n
    assert got["loss"] == float(np.sum(losses)) / n
    assert all(np.isfinite(got[m]) for m in ("recall", "mrr", "ndcg", "loss", "ild", "unexp")) and got["coverage"] > 0
    # a pool is a fraction of the catalog, so the label ranks higher in it than in the whole catalog
    whole, _ = run_test(model, te, args)
    assert got["recall"] >= whole["recall"] and got["mrr"] >= whole["mrr"] and got["loss"] < whole["loss"]
