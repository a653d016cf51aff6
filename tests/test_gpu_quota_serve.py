"""Per-category caps at the engine level (TcarEngine.eval_step_streamed / recommend with max_per_category=, tcar_serve_step_quota) and
through Seq2SeqAttNN.test() with cat_cap, on the small engine and fold of tests/window_case.py.

The engine check needs no tolerance: recommend(k=64) returns the 64 best items of a session and their score bits; every other item
scores lower, so the capped walk over those 64 — as long as it yields k items — is the capped list of the whole catalog."""
import numpy as np
import pytest

import tcar_amd  # noqa: F401

from gpu_util import _need_gpu
from quota_case import CAT, K, M, walk_of_the_best_64
from window_case import B, N, PANEL, reference, run_test, trained

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("scoring", ["f32", "bf16x3-mixed"])
def test_capped_lists_are_the_walk_over_the_uncapped_best_64(scoring):
    _need_gpu()
    from tcar_amd.engine import TcarEngine
    r = reference()
    batch = r["batch"]
    eng = TcarEngine(r["params"], r["content"], r["mw"], max_grad=2.0, scoring=scoring)
    feed = {n: v for n, v in batch.items() if n not in ("label", "neg")}
    with pytest.raises(ValueError, match="set_categories"):
        eng.recommend(feed, k=K, panel=PANEL, max_per_category=M)                    # a cap without a category table
    with pytest.raises(ValueError, match="set_categories"):
        eng.eval_step_streamed(batch, k=K, panel=PANEL, max_per_category=M)
    eng.set_categories(CAT)
    eng.set_item_keys(r["key"])
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="max_per_category"):
            eng.recommend(feed, k=K, panel=PANEL, max_per_category=bad)
    with pytest.raises(ValueError, match="max_per_category"):
        eng.eval_step_streamed(batch, k=K, panel=PANEL, max_per_category=0)
    third = (int(r["lo"][1]), int(r["hi"][1]))                       # 233 items in the pool of every session
    seen = (batch["seq"] - 1).astype(np.int64)
    for kw in (dict(exclude_seen=False), dict(exclude_seen=True), dict(exclude_seen=True, window=third),
               dict(exclude_seen=False, exclude=np.arange(B * 3, dtype=np.int32).reshape(B, 3) % N)):
        tk64, sc64 = (x.cpu().numpy().copy() for x in eng.recommend(feed, k=64, panel=PANEL, **kw))
        want_tk, want_sc = walk_of_the_best_64(tk64, sc64)
        got_tk, got_sc = (x.cpu().numpy().copy() for x in eng.recommend(feed, k=K, panel=PANEL, max_per_category=M, **kw))
        assert (got_tk == want_tk).all(), (kw, np.where(got_tk != want_tk))
        assert got_sc.tobytes() == want_sc.tobytes(), kw                            # the score bits
        assert all(np.unique(CAT[t], return_counts=True)[1].max() <= M for t in got_tk)
        assert (got_tk != tk64[:, :K]).any()                                        # the cap changed something
        if kw["exclude_seen"]:
            assert all(not set(got_tk[b].tolist()) & set(seen[b].tolist()) for b in range(B))
        if "window" in kw:
            assert ((third[0] <= r["key"][got_tk]) & (r["key"][got_tk] < third[1])).all()
        # one fold (the default panel) and another partition: the same bits
        for panel in (None, 128):
            tk2, sc2 = (x.cpu().numpy().copy() for x in eng.recommend(feed, k=K, panel=panel, max_per_category=M, **kw))
            assert (tk2 == got_tk).all(), (kw, panel)
    # a cap of k or more is the uncapped call
    tk0, sc0 = (x.cpu().numpy().copy() for x in eng.recommend(feed, k=K, panel=PANEL))
    tk1, sc1 = (x.cpu().numpy().copy() for x in eng.recommend(feed, k=K, panel=PANEL, max_per_category=K))
    assert tk0.tobytes() == tk1.tobytes() and sc0.tobytes() == sc1.tobytes()

    # evaluation: the cap shapes the list and leaves rank and ce alone, bit for bit
    for kw in (dict(), dict(window=third)):
        rank0, topk0, ce0 = (x.cpu().numpy().copy() for x in eng.eval_step_streamed(batch, k=K, panel=PANEL, **kw))
        rank1, topk1, ce1 = (x.cpu().numpy().copy() for x in eng.eval_step_streamed(batch, k=K, panel=PANEL, max_per_category=M, **kw))
        assert (rank0 == rank1).all() and ce0.tobytes() == ce1.tobytes(), kw
        assert (topk1 >= 0).all() and all(np.unique(CAT[t], return_counts=True)[1].max() <= M for t in topk1)
        assert (topk0 != topk1).any()
        _, tk64, _ = eng.eval_step_streamed(batch, k=64, panel=PANEL, **kw)
        want_tk, want_sc = walk_of_the_best_64(tk64.cpu().numpy().copy(), eng.last_scores.cpu().numpy().copy())
        assert (topk1 == want_tk).all(), kw
    eng.check_forks()


def test_a_cat_cap_of_20_reproduces_the_uncapped_streamed_test():
    _need_gpu()
    t = trained()
    model, args = t["models"]["early"]
    plain, text0 = run_test(model, t["te"], args)
    capped, text1 = run_test(model, t["te"], dict(args, cat_cap=20))
    lists = capped.pop("capped")
    assert capped == plain and "capped" not in plain                 # exactly: every metric, the coverage included
    assert lists == {"mrr": plain["mrr"], "recall": plain["recall"], "ndcg": plain["ndcg"]}      # the label's place in the list is its rank
    line = "capped lists (<= 20 per category): MRR@20: {}, Recall@20: {}, nDCG@20: {}\n".format(lists["mrr"], lists["recall"], lists["ndcg"])
    assert line in text1 and text1.replace(line, "") == text0


def test_a_cat_cap_of_1_gives_lists_of_distinct_categories():
    _need_gpu()
    t = trained()
    model, args = t["models"]["early"]
    plain, _ = run_test(model, t["te"], args)
    eng, lists = model.engine, []
    inner = eng.eval_step_streamed

    def recording(*a, **kw):
        assert kw.get("max_per_category") == 1
        out = inner(*a, **kw)
        lists.append(out[1].cpu().numpy().copy())
        return out
    eng.eval_step_streamed = recording
    try:
        capped, text = run_test(model, t["te"], dict(args, cat_cap=1))
    finally:
        del eng.eval_step_streamed
    cat = model._category_table()
    tk = np.concatenate(lists)
    assert len(tk) == t["fold"].test.n and (tk >= 0).all()           # 300 categories over 400 items: every list is full
    assert all(len(set(cat[row].tolist())) == 20 for row in tk)      # recomputed on the host: twenty categories in twenty entries
    assert capped["ild"] == 1.0
    assert capped["capped"]["recall"] <= capped["recall"]
    assert (capped["mrr"], capped["recall"], capped["ndcg"], capped["loss"]) == (plain["mrr"], plain["recall"], plain["ndcg"], plain["loss"])
    assert capped["ild"] >= plain["ild"] and "capped lists (<= 1 per category): MRR@20: " in text
    # with a publish-time window on top: still distinct categories, and the windowed ranks
    fresh, _ = run_test(model, t["te"], dict(args, fresh_hours=1e6))
    both, _ = run_test(model, t["te"], dict(args, fresh_hours=1e6, cat_cap=1))
    assert both["ild"] == 1.0 and both["recall"] == fresh["recall"] and both["capped"] == capped["capped"]
