"""Related items through the engine (TcarEngine.similar_items, Seq2SeqAttNN.related_articles / similar_to_content, test() with
eval_related; tcar_similar_step) on the N = 700, H = 250 setup of tests/serve_case.py, k = 20.

What is compared with what:
  partition   panels of 128, of 256 (three, the last one 188 wide) and the default panel: equal bytes.
  list logic  the [Q, 700] block of ONE tcar_sim_panel call, turned into lists by the numpy model (select_ref through
              similar_ref.lists), against similar_items byte for byte — plain, exclude_self, exclude, a window per query, a cap of 2 per
              category, all at once.  The fold is existing code and the scores are checked at the op level (test_gpu_similar_panel.py),
              so nothing here is compared with itself.
  fp64        TOL_SIM = (H + 8) 2^-24 bounds one similarity (derived in tests/test_gpu_mmr_walk.py).  On the fixture content many
              queries are NOT decisive (of the 32 queries used here 6 have a neighbouring gap <= 2 TOL_SIM inside their fp64 top 21, the
              smallest 4.0e-6), so whole lists are not compared
              there: every listed item is within 2 TOL_SIM of the fp64 k-th best, no unlisted eligible item beats a listed one by more
              than 2 TOL_SIM, every reported sim is within TOL_SIM.  No query is left out.
  planted     similar_case.planted(): N = 3,000, 32 queries with 24 planted neighbours at cosines 0.95 - 0.02 j.  Checked here in
              fp64: the smallest gap inside a top-21 is 0.02 = 650 x 2 TOL_SIM, the 20th best is 0.57, the best unplanted item is
              <= 0.29 — so the lists must EQUAL the fp64 lists for all 32 queries.  Through tcar_similar_step on a plain table (a
              context that holds the dimensions and E alone): no 3,000-row engine is built."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401

from gpu_util import _need_gpu, _np, ptr
from serve_case import H, N, TOPK, _keys_and_windows, reference
from similar_case import P_H, P_N, P_NEIGH, P_Q, planted
from similar_ref import lists, sims_f64, tol_sim
from window_case import run_test, trained

pytestmark = pytest.mark.gpu

TOL_SIM = tol_sim(H)
NQ = 16
_ENG = {}


def _engine(content=None):
    from tcar_amd.engine import TcarEngine
    r = reference()
    return TcarEngine(r["params"], r["content"] if content is None else content, r["mw"], max_grad=2.0, scoring="bf16x3-mixed")


def _shared():
    """one engine for the tests that only read it, with item keys and categories installed"""
    if not _ENG:
        eng = _engine()
        keys, lo, hi = _keys_and_windows()
        cat = np.random.RandomState(9).randint(0, 9, N).astype(np.int32)
        eng.set_item_keys(keys)
        eng.set_categories(cat)
        _ENG.update(eng=eng, keys=keys, lo=lo, hi=hi, cat=cat)
    return _ENG


def _ids(n, seed=2):
    return np.random.RandomState(seed).choice(N, n, replace=False).astype(np.int32)


def _same(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, i, np.argwhere(x != y)[:5])


def _block(eng, ids):
    """the [Q, N] similarities of the catalog rows `ids` from one tcar_sim_queries and ONE tcar_sim_panel over E's content columns"""
    g, lib, Q = eng.geo, eng.lib, len(ids)
    qid = torch.from_numpy(np.asarray(ids, np.int32)).cuda()
    xq, rq = torch.zeros(Q, g.ldh, device="cuda"), torch.zeros(Q, device="cuda")
    out = torch.full((Q, N), float("nan"), device="cuda")
    cp = C.c_void_p(eng.E.data_ptr() + 4 * g.ldh)
    torch.cuda.synchronize()
    assert lib.tcar_sim_queries(Q, g.N, g.H, cp, g.ek, ptr(qid), None, 0, ptr(xq), g.ldh, ptr(rq), None) == 0
    assert lib.tcar_sim_panel(Q, 0, g.N, g.H, cp, g.ek, ptr(xq), g.ldh, ptr(rq), ptr(out), N, None) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_every_partition_into_panels_returns_the_same_bytes():
    _need_gpu()
    eng, ids = _shared()["eng"], _ids(NQ)
    want = _np(*eng.similar_items(ids, k=TOPK, panel=128))
    assert want[0].shape == (NQ, TOPK) and want[0].dtype == np.int32 and want[1].dtype == np.float32 and (want[0] >= 0).all()
    assert not (want[0] == ids[:, None]).any()                                  # exclude_self is the default
    _same(_np(*eng.similar_items(ids, k=TOPK, panel=256)), want, "panel 256: three panels, the last one 188 wide")
    _same(_np(*eng.similar_items(ids, k=TOPK)), want, "the default panel")
    _same(_np(*eng.similar_items(torch.from_numpy(ids.astype(np.int64)).cuda(), k=TOPK, panel=256)), want, "ids as a device tensor")


def test_the_lists_are_the_model_s_lists_of_one_panel_call_s_block():
    _need_gpu()
    s = _shared()
    eng, keys, cat, ids = s["eng"], s["keys"], s["cat"], _ids(NQ)
    lo, hi = s["lo"][:NQ], s["hi"][:NQ].copy()
    hi[::4] = lo[::4] + 12                                                      # (the keys are a permutation: twelve items)
    block = _block(eng, ids)
    assert np.isfinite(block).all() and (np.abs(block[np.arange(NQ), ids] - 1) <= TOL_SIM).all()
    rng = np.random.RandomState(4)
    extra = rng.randint(-1, N, (NQ, 5)).astype(np.int32)
    extra[:, 0] = np.argsort(block, 1)[:, -2]                                   # the best item that is not the query itself
    own = [[int(i)] for i in ids]
    pool = (lo[:, None] <= keys[None, :]) & (keys[None, :] < hi[:, None])
    assert pool.sum(1).min() < TOPK < pool.sum(1).max()                          # some windows hold fewer than k items
    both = [o + e.tolist() for o, e in zip(own, extra)]
    for what, kw, model in (("plain", dict(exclude_self=False), dict()),
                            ("exclude_self", dict(), dict(excl=own)),
                            ("exclude", dict(exclude_self=False, exclude=extra), dict(excl=extra.tolist())),
                            ("window", dict(exclude_self=False, window=(lo, hi)), dict(pool=pool)),
                            ("cap", dict(exclude_self=False, max_per_category=2), dict(cat=cat, cap=2)),
                            ("all", dict(exclude=extra, window=(lo, hi), max_per_category=2), dict(excl=both, pool=pool, cat=cat, cap=2))):
        got = _np(*eng.similar_items(ids, k=TOPK, panel=256, **kw))
        _same(got, lists(block, TOPK, **model), what)
        if "cap" in model:
            assert all(np.bincount(cat[t[t >= 0]], minlength=9).max() <= 2 for t in got[0]), what
    assert (_np(*eng.similar_items(ids, k=TOPK, exclude_self=False))[0][:, 0] == ids).all()


def test_every_list_lies_in_the_fp64_band():
    _need_gpu()
    eng, ids = _shared()["eng"], _ids(32, seed=6)
    content = reference()["content"][1:]
    s64 = sims_f64(content[ids], content)
    topk, sims = _np(*eng.similar_items(ids, k=TOPK, panel=256))
    assert (topk >= 0).all() and all(len(set(t.tolist())) == TOPK for t in topk)
    worst = [0.0, 0.0, 0.0]
    for q in range(32):
        ok = np.ones(N, bool)
        ok[ids[q]] = False
        assert ok[topk[q]].all()
        kth = np.sort(s64[q][ok])[-TOPK]
        listed = s64[q][topk[q]]
        ok[topk[q]] = False
        worst = [max(worst[0], float(kth - listed.min())), max(worst[1], float(s64[q][ok].max() - listed.min())),
                 max(worst[2], float(np.abs(sims[q] - listed).max()))]
        assert (listed >= kth - 2 * TOL_SIM).all(), q
        assert s64[q][ok].max() <= listed.min() + 2 * TOL_SIM, q
        assert (np.abs(sims[q].astype(np.float64) - listed) <= TOL_SIM).all(), q
    print("below the fp64 k-th best by at most %.3e, an unlisted item above a listed one by at most %.3e (2 TOL_SIM %.3e); "
          "largest error of a reported sim %.3e (TOL_SIM %.3e)" % (worst[0], worst[1], 2 * TOL_SIM, worst[2], TOL_SIM))


def test_planted_neighbours_come_back_as_the_fp64_lists_for_every_query():
    _need_gpu()
    from tcar_amd import _lib
    lib = _lib.load()
    content, ids = planted()
    s64 = sims_f64(content[ids], content)
    s64[np.arange(P_Q), ids] = -np.inf                                          # the query itself is excluded
    order = np.argsort(s64, 1)[:, ::-1]
    top21 = np.take_along_axis(s64, order[:, :TOPK + 1], 1)
    planted_rows = 100 + P_NEIGH * np.arange(P_Q)[:, None] + np.arange(P_NEIGH)[None, :]
    assert (order[:, :TOPK] == planted_rows[:, :TOPK]).all()
    rest = s64.copy()
    np.put_along_axis(rest, planted_rows, -np.inf, 1)
    assert (top21[:, :-1] - top21[:, 1:]).min() >= 0.0199 and top21[:, TOPK - 1].min() >= 0.5699 and rest.max() <= 0.29
    assert 0.0199 > 600 * 2 * TOL_SIM
    # a plain table in the layout of a context: ek = 2 ldh + 5 ldt floats per row, the content columns at ldh
    ldh, ldt = 256, 64
    ek = 2 * ldh + 5 * ldt
    E = torch.zeros(P_N, ek)
    E[:, ldh:ldh + P_H] = torch.from_numpy(np.array(content))
    E = E.cuda()
    ctx, q, s = _lib.Ctx(), _lib.Similar(), _lib.Serve()
    ctx.d.n_items, ctx.d.H, ctx.d.Ht, ctx.d.ldh, ctx.d.ldt = P_N, P_H, ldt, ldh, ldt
    ctx.E = E.data_ptr()
    panel = 1024
    qid = torch.from_numpy(ids).cuda()
    xq, rq = torch.zeros(P_Q, ldh, device="cuda"), torch.zeros(P_Q, device="cuda")
    buf = torch.zeros(P_Q, panel, device="cuda")
    words = int(lib.tcar_select_state_bytes(1, TOPK)) // 4
    state = torch.zeros(P_Q, words, dtype=torch.int32, device="cuda")
    topk = torch.full((P_Q, TOPK), -7, dtype=torch.int32, device="cuda")
    score = torch.zeros(P_Q, TOPK, device="cuda")
    excl = qid.clone().view(P_Q, 1).contiguous()
    q.qid, q.xq, q.rq = qid.data_ptr(), xq.data_ptr(), rq.data_ptr()
    s.k, s.panel, s.panel_buf, s.state, s.state_bytes = TOPK, panel, buf.data_ptr(), state.data_ptr(), state.numel() * 4
    s.excl, s.X, s.topk, s.score = excl.data_ptr(), 1, topk.data_ptr(), score.data_ptr()
    torch.cuda.synchronize()
    assert lib.tcar_similar_step(C.byref(ctx), P_Q, C.byref(q), C.byref(s), None, None, None) == 0
    torch.cuda.synchronize()
    got, sims = _np(topk, score)
    assert (got == order[:, :TOPK]).all(), np.argwhere(got != order[:, :TOPK])[:5]
    assert np.abs(sims - top21[:, :TOPK]).max() <= TOL_SIM


def test_a_live_content_update_is_found_by_the_next_call():
    _need_gpu()
    r = reference()
    eng, rng = _engine(), np.random.RandomState(8)
    i, j = 17, 403
    others = _ids(6, seed=12)
    before = _np(*eng.similar_items([j], k=TOPK))
    assert i not in before[0][0]
    row = r["content"][1 + j]
    eng.update_items([i], content=row[None, :])
    topk, sims = _np(*eng.similar_items([j], k=TOPK))
    assert topk[0, 0] == i and abs(float(sims[0, 0]) - 1.0) <= TOL_SIM
    assert topk[0, 1:].tolist() == before[0][0, :TOPK - 1].tolist() and sims[0, 1:].tobytes() == before[1][0, :TOPK - 1].tobytes()
    final = r["content"].copy()
    final[1 + i] = row
    ids = np.concatenate([[j, i], others]).astype(np.int32)
    _same(_np(*eng.similar_items(ids, k=TOPK, panel=256)), _np(*_engine(content=final).similar_items(ids, k=TOPK, panel=256)),
          "updated engine against one built from the final tables")
    del rng


def test_drafts_score_the_bits_of_the_rows_they_copy():
    _need_gpu()
    eng, ids = _shared()["eng"], _ids(NQ, seed=3)
    rows = reference()["content"][1 + ids]
    want = _np(*eng.similar_items(ids, k=TOPK, exclude_self=False, panel=256))
    _same(_np(*eng.similar_items(content=rows, k=TOPK, panel=256)), want, "content= against ids")
    _same(_np(*eng.similar_items(content=torch.from_numpy(rows.astype(np.float64)).cuda(), k=TOPK)), want, "a float64 device tensor")


def test_empty_and_degenerate_queries():
    _need_gpu()
    s = _shared()
    eng, keys = s["eng"], s["keys"]
    ids = np.asarray([5, -1, 300, N + 3], np.int32)
    topk, sims = _np(*eng.similar_items(ids, k=TOPK, panel=256))
    assert (topk[[1, 3]] == -1).all() and (sims[[1, 3]] == 0).all()             # an empty query lists nothing
    one = _np(*eng.similar_items(ids[[0, 2]], k=TOPK, panel=256))
    _same((topk[[0, 2]], sims[[0, 2]]), one, "the neighbours of an empty query are not moved by it")
    # an all-zero row is similar to nothing: every sim is +0 and the list order falls back to the item id, descending
    topk, sims = _np(*eng.similar_items(content=np.zeros((2, H), np.float32), k=TOPK))
    assert (topk == np.arange(N - 1, N - 1 - TOPK, -1)[None, :]).all() and not sims.any() and not np.signbit(sims).any()
    topk, _ = _np(*eng.similar_items(content=np.zeros((1, H), np.float32), k=TOPK, exclude=[[N - 1, N - 3]]))
    assert topk[0].tolist() == [n for n in range(N - 1, N - 30, -1) if n not in (N - 1, N - 3)][:TOPK]
    # a window that holds seven items: seven entries, then -1
    topk, sims = _np(*eng.similar_items([5, 9], k=TOPK, window=(0, 7)))
    inside = set(np.where((keys >= 0) & (keys < 7))[0].tolist())
    for q, me in enumerate((5, 9)):
        want = inside - {me}
        assert set(topk[q, :len(want)].tolist()) == want and (topk[q, len(want):] == -1).all() and (sims[q, len(want):] == 0).all()
        assert (np.diff(sims[q, :len(want)]) <= 0).all()


def test_eval_related_adds_its_line_and_the_model_reaches_the_call():
    _need_gpu()
    from tcar_amd import _lib
    t = trained()
    model, args = t["models"]["early"]
    plain, text0 = run_test(model, t["te"], args)
    K = 5
    got, text1 = run_test(model, t["te"], dict(args, eval_related=K))
    rel = got.pop("related")
    assert got == plain and "related" not in plain
    line = "related articles ({} per article): mean cosine: {}, same category: {}\n".format(K, rel["mean_cosine"], rel["same_category"])
    assert line in text1 and text1.replace(line, "") == text0
    # the figures from the content table in fp64: the K best cosines of every distinct label article
    eng = model.engine
    content, cat = np.asarray(eng._content)[1:], model._category_table()
    labels = _labels(model, t["te"])
    assert rel["k"] == K and rel["articles"] == len(labels) > 10
    s64 = sims_f64(content[labels], content)
    s64[np.arange(len(labels)), labels] = -np.inf
    best = np.sort(s64, 1)[:, -K:]
    # (a listed item is within 2 TOL_SIM of the fp64 one of its place and its reported cosine within TOL_SIM of its own)
    assert abs(rel["mean_cosine"] - best.mean()) <= 3 * tol_sim(content.shape[1])
    assert 0.0 <= rel["same_category"] <= 1.0
    # the model's calls are the engine's
    ids = labels[:6]
    want = _np(*eng.similar_items(ids, k=4))
    _same(_np(*model.related_articles(ids, k=4)), want, "related_articles")
    _same(_np(*model.similar_to_content(content[ids], k=4, exclude=ids[:, None])), want, "similar_to_content")
    lim = _np(*model.related_articles(ids, k=4, max_per_category=1))[0]
    assert all(len(set(cat[r[r >= 0]].tolist())) == (r >= 0).sum() for r in lim)
    with pytest.raises(ValueError, match="k must be"):
        model.related_articles(ids, k=65)
    assert isinstance(_lib.TcarError("x"), RuntimeError)


def _labels(model, te):
    """the distinct labels of the feeds the model's own sampler builds from the test data (0-based, as test() reads them)"""
    sampler, out = model._sampler((copy.deepcopy(te[0]), te[1], te[2])), []
    while sampler.has_next():
        out.append(np.asarray(sampler.next_batch_arrays()["label"]).reshape(-1))
    return np.unique(np.concatenate(out))
