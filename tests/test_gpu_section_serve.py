"""Sectioned recommendation at the engine level (TcarEngine.recommend_sections, tcar_sections_step) and through Seq2SeqAttNN.test()
with eval_sections.

The oracle is in the code base and needs no tolerance: list g of recommend_sections(sections, k) must carry the bits of
recommend(k, window=(code, code + 1)) on the same engine once its item keys are the categories.  Two small engines per scoring mode:
N = 1,003 and N = 49,300 — above one default panel, so the default partition has two panels there."""
import numpy as np
import pytest

import tcar_amd  # noqa: F401

from gpu_util import _need_gpu, _np, close
from window_case import run_test, trained

pytestmark = pytest.mark.gpu

H, Ht, B, T, K = 250, 64, 13, 3, 10
SECTIONS = [3, -2 ** 31, 0, 2 ** 31 - 2, 7, 424242]          # the last code: no item carries it
_CASE = {}


def case(N):
    """parameters, a batch and a category table of one catalog size: computed once, shared, never written"""
    if N not in _CASE:
        from oracle.tcar_oracle import init_params_numpy
        rng = np.random.RandomState(N)
        params = init_params_numpy(N, H, Ht, 0.35, 0.12, rng)
        content = (rng.standard_normal((N + 1, H)) * 0.5).astype(np.float32)
        content[0] = 0
        mw = np.stack([rng.randint(1, 13, N), rng.randint(1, 32, N), rng.randint(1, 8, N), rng.randint(1, 25, N),
                       rng.randint(1, 61, N)], -1).astype(np.int32)
        b = {"seq": rng.randint(1, N + 1, (B, T)), "label": rng.randint(0, N, B), "pm": rng.randint(1, 13, (B, T)),
             "pd": rng.randint(1, 32, (B, T)), "pw": rng.randint(1, 8, (B, T)), "ph": rng.randint(1, 25, (B, T)),
             "pmi": rng.randint(1, 61, (B, T)), "cw": rng.randint(0, 7, B), "ch": rng.randint(0, 24, B),
             "gap": rng.randint(0, 12, (B, T)), "neg": rng.randint(0, N, (B, 5))}
        b = {k: v.astype(np.int32) for k, v in b.items()}
        # about N / 9 items per listed category, except code 7: five items (a list that ends early)
        cat = np.asarray([3, -2 ** 31, 0, 2 ** 31 - 2, 11, 12, 13, 14, 15], np.int64)[rng.randint(0, 9, N)].astype(np.int32)
        cat[rng.permutation(N)[:5]] = 7
        pub = rng.permutation(N).astype(np.int32)                     # publish keys, distinct
        for a in list(b.values()) + [cat, pub]:
            a.setflags(write=False)
        _CASE[N] = dict(params=params, content=content, mw=mw, batch=b, cat=cat, pub=pub)
    return _CASE[N]


def engine(N, scoring):
    from tcar_amd.engine import TcarEngine
    c = case(N)
    eng = TcarEngine(c["params"], c["content"], c["mw"], max_grad=2.0, scoring=scoring)
    eng.set_categories(c["cat"])
    return eng


def free(batch):
    return {n: v for n, v in batch.items() if n not in ("label", "neg")}


def by_windows(eng, feed, cat, k, sections=SECTIONS, **kw):
    """the oracle: one windowed recommend() per section on the engine whose item keys are the categories -> [B, G, k] ids and scores"""
    eng.set_item_keys(cat)
    tk, sc = [], []
    for code in sections:
        t, s = _np(*eng.recommend(feed, k=k, window=(code, code + 1), **kw))
        s[t < 0] = -7.0                                              # (behind a list's end the scores are whatever the buffer held)
        tk.append(t)
        sc.append(s)
    eng.set_item_keys(None)
    return np.stack(tk, 1), np.stack(sc, 1)


def sectioned(eng, feed, k, sections=SECTIONS, **kw):
    res = eng.recommend_sections(feed, sections, k=k, **kw)
    tk, sc = _np(res.topk, res.scores)
    sc[tk < 0] = -7.0
    return tk, sc, res


def same(a, b, what):
    assert a[0].shape == b[0].shape and a[0].tobytes() == b[0].tobytes(), (what, np.where(a[0] != b[0]))
    assert a[1].tobytes() == b[1].tobytes(), what


@pytest.mark.parametrize("scoring", ["f32", "bf16x3-mixed"])
@pytest.mark.parametrize("N", [1003, 49300])
def test_every_section_list_carries_the_bits_of_the_windowed_recommend(N, scoring):
    _need_gpu()
    c = case(N)
    eng = engine(N, scoring)
    feed, cat = free(c["batch"]), c["cat"]
    assert eng.default_panel() < N or N == 1003
    extra = (np.arange(B * 3, dtype=np.int32).reshape(B, 3) * 7) % N
    for trained_steps in (0, 2):
        for _ in range(trained_steps):
            eng.train_step(c["batch"])
        for kw in (dict(exclude_seen=False), dict(exclude_seen=True), dict(exclude_seen=True, exclude=extra)):
            want = by_windows(eng, feed, cat, K, **kw)
            got = sectioned(eng, feed, K, **kw)[:2]
            same(got, want, (trained_steps, kw))
            same(sectioned(eng, feed, K, panel=128 if N == 1003 else 8192, **kw)[:2], want, (trained_steps, kw, "small panels"))
            tk = got[0]
            assert (tk[:, -1] == -1).all() and (tk[:, 4, 5:] == -1).all() and (tk[:, 4, 0] >= 0).all()       # no item / five items
            assert (tk[:, :4] >= 0).all()
            for g, code in enumerate(SECTIONS):
                assert (cat[tk[:, g][tk[:, g] >= 0]] == code).all(), code
            if kw["exclude_seen"]:
                seen = c["batch"]["seq"] - 1
                assert all(not set(tk[b].ravel().tolist()) & set(seen[b].tolist()) for b in range(B))
    eng.check_forks()


@pytest.mark.parametrize("scoring", ["f32", "bf16x3-mixed"])
def test_a_publish_window_and_the_overall_list_ride_on_the_same_panels(scoring):
    _need_gpu()
    N = 1003
    c = case(N)
    eng = engine(N, scoring)
    feed, cat, pub = free(c["batch"]), c["cat"], c["pub"]
    lo = np.full(B, 100, np.int64)
    hi = np.where(np.arange(B) % 2 == 0, 600, 900).astype(np.int64)
    # the oracle of "fresh sport": windowed by category, with the items outside the publish window passed as exclusions
    outside = [np.where(~((lo[b] <= pub) & (pub < hi[b])))[0] for b in range(B)]
    excl = np.full((B, max(len(o) for o in outside)), -1, np.int32)
    for b, o in enumerate(outside):
        excl[b, :len(o)] = o
    want = by_windows(eng, feed, cat, K, exclude_seen=True, exclude=excl)
    eng.set_item_keys(pub)
    got = sectioned(eng, feed, K, window=(lo, hi))
    same(got[:2], want, "publish window + sections")
    listed = [got[0][b][got[0][b] >= 0] for b in range(B)]
    assert all(len(t) and ((lo[b] <= pub[t]) & (pub[t] < hi[b])).all() for b, t in enumerate(listed))
    # overall = k0: the bits of recommend(k0) with the same window and exclusions; the section lists do not move
    for kw in (dict(), dict(window=(lo, hi))):
        plain = sectioned(eng, feed, K, **kw)[:2]
        for k0 in (1, 20, 64):
            tk, sc, res = sectioned(eng, feed, K, overall=k0, **kw)
            same((tk, sc), plain, ("sections with overall", k0))
            otk, osc = _np(res.overall_topk, res.overall_scores)
            rtk, rsc = _np(*eng.recommend(feed, k=k0, **kw))
            assert otk.shape == (B, k0) and otk.tobytes() == rtk.tobytes(), (k0, kw)
            assert osc[otk >= 0].tobytes() == rsc[rtk >= 0].tobytes(), (k0, kw)
    assert sectioned(eng, feed, K)[2].overall_topk is None
    eng.check_forks()


def test_ragged_feeds_give_the_rectangular_bits_and_mixed_lengths_their_own_lists():
    _need_gpu()
    from tcar_amd.host.data import pack_sessions
    N = 1003
    c = case(N)
    eng = engine(N, "bf16x3-mixed")
    rect = free(c["batch"])
    same(sectioned(eng, pack_sessions([rect]), K)[:2], sectioned(eng, rect, K)[:2], "uniform lengths")
    # mixed lengths: the sessions of the batch cut to 1, 2 and 3 clicks, one ragged call
    per_row = ("seq", "pm", "pd", "pw", "ph", "pmi", "gap")
    feeds = []
    for length, rows in ((1, slice(0, 4)), (2, slice(4, 9)), (3, slice(9, B))):
        feeds.append({n: (v[rows, :length] if n in per_row else v[rows]) for n, v in rect.items()})
    mixed = pack_sessions(feeds)
    tk, sc, _ = sectioned(eng, mixed, K)
    same((tk, sc), by_windows(eng, mixed, c["cat"], K), "mixed lengths vs the windowed recommend of the same feed")
    s0 = 0
    for f in feeds:                      # the rule of test_gpu_ragged_serve for recommend(): each length's rectangular call, scores close
        one_tk, one_sc, _ = sectioned(eng, f, K)
        n = one_tk.shape[0]
        assert ((tk[s0:s0 + n] >= 0) == (one_tk >= 0)).all()
        close(sc[s0:s0 + n], one_sc, name="mixed feed vs the feed of one length")
        s0 += n
    eng.check_forks()


def test_an_item_moves_between_sections_with_update_items():
    _need_gpu()
    from tcar_amd.engine import TcarEngine
    N = 1003
    c = case(N)
    eng = engine(N, "bf16x3-mixed")
    feed = free(c["batch"])
    before = sectioned(eng, feed, K, exclude_seen=False)[0]
    movers = np.unique(before[:, 0, :3])                             # the best three of section 3 of every session ...
    movers = movers[movers >= 0][:40].astype(np.int64)
    final = np.array(c["cat"])
    final[movers] = 0                                                # ... move to section 0
    eng.update_items(movers, categories=final[movers])
    after = sectioned(eng, feed, K, exclude_seen=False)
    fresh = TcarEngine(c["params"], c["content"], c["mw"], max_grad=2.0, scoring="bf16x3-mixed")
    fresh.set_categories(final)
    same(after[:2], sectioned(fresh, feed, K, exclude_seen=False)[:2], "updated engine vs an engine built from the final table")
    assert not set(after[0][:, 0].ravel().tolist()) & set(movers.tolist())                   # gone from the old section
    assert set(after[0][:, 2].ravel().tolist()) & set(movers.tolist())                       # and in the new one where the score earns it
    assert (final[after[0][:, 2][after[0][:, 2] >= 0]] == 0).all()


def test_eval_sections_adds_its_line_and_lists_what_the_evaluation_lists():
    _need_gpu()
    from tcar_amd.host import metrics as M
    t = trained()
    model, args = t["models"]["early"]
    plain, text0 = run_test(model, t["te"], args)
    G = 4
    eng, calls = model.engine, []
    inner_sec, inner_eval = eng.recommend_sections, eng.eval_step_streamed

    def rec_sections(batch, sections, **kw):
        assert kw["k"] == 20 and kw["exclude_seen"] is False and kw.get("window") is None
        res = inner_sec(batch, sections, **kw)
        calls[-1] += (list(sections), res.topk.cpu().numpy().copy())
        return res

    def rec_eval(*a, **kw):
        out = inner_eval(*a, **kw)
        calls.append((out[1].cpu().numpy().copy(),))
        return out
    eng.recommend_sections, eng.eval_step_streamed = rec_sections, rec_eval
    try:
        got, text1 = run_test(model, t["te"], dict(args, eval_sections=G))
    finally:
        del eng.recommend_sections, eng.eval_step_streamed
    sec = got.pop("sections")
    assert got == plain and "sections" not in plain
    cat = model._category_table()
    want_sections = M.largest_categories(cat, G).tolist()
    line = "sections ({} categories, 20 per section): Recall@20 in the label's section: {}, labels in a listed section: {}\n".format(
        G, sec["recall"], sec["covered"])
    assert line in text1 and text1.replace(line, "") == text0
    assert sec["G"] == G and 0.0 <= sec["recall"] <= 1.0 and 0.0 < sec["covered"] <= 1.0
    # an item of a listed category inside the evaluation's own top 20 is inside that section's list
    n = 0
    for topk, sections, stk in calls:
        assert sections == want_sections
        for b in range(topk.shape[0]):
            for i in topk[b][topk[b] >= 0]:
                if cat[i] in sections:
                    assert i in stk[b, sections.index(cat[i])], (b, i)
                    n += 1
    assert n > 0
    # with a publish-time window (one that holds every item) and the batches packed into ragged ones: the flag combines with both; the
    # labels are the same, so the covered share is, and the line is there (a ragged call's scores are close, not the same bits)
    both, text2 = run_test(model, t["te"], dict(args, eval_sections=G, fresh_hours=1e6, eval_mixed=1))
    assert both["sections"]["covered"] == sec["covered"] and both["sections"]["G"] == G
    assert "sections ({} categories, 20 per section): Recall@20 in the label's section: ".format(G) in text2
