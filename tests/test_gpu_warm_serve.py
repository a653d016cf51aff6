"""The warm start through the engine (TcarEngine.warm_start_items, tcar_warm_step; include/tcar_warm.h) on the shape of
tests/catalog_case.py — N = 700 (the last 50 rows spare: their keys lie above every window), H = 250 at ldh 256, B = 8, T = 5 — on an
fp32 and a split-bf16 engine, fresh and after two training steps.

  lists     donors / sims are, bit for bit, similar_items(ids, k, exclude = ids + exclude, window): no named id ever donates; the
            same bits for panel = 128 and the default.
  rows      within (2 k + 2) 2^-24 max|x| of the fp64 statement of the rule (tests/warm_ref.py) fed the engine's own item table.
  contract  the live engine answers recommend, eval_step_streamed and score_candidates with the bits of an engine BUILT from its
            exported state (the comparison of tests/test_gpu_catalog_update.py, restated); the Adam moments of the named rows are
            zero, every other moment keeps its bytes.
  pool      emptied by a window, every row is +0 with support 0.
  after     a following update_items(item_rows = array) behaves as ever.
  planted   content in well-separated clusters, item rows a cluster centroid plus noise of a fixed radius: on the CPU first — the
            reference lists hold same-cluster donors only and every blended row lies closer to its centroid than the noise radius,
            because a convex combination of same-cluster rows does — then the same two statements of the engine's rows."""
import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401

import serve_shapes_ref as R
import warm_ref
from catalog_case import B, FAR, H, N, SPARE, tables
from gpu_util import _need_gpu, _np
from similar_ref import lists, sims_f32

pytestmark = pytest.mark.gpu

K = 16
WINDOW = (0, 10 ** 6)                            # every live key; the spare rows (FAR) are outside
_rs = np.random.RandomState(17)
IDS = np.concatenate([[0, 127, 128, N - SPARE - 1], _rs.choice(np.arange(1, N - SPARE - 1), 7, replace=False),
                      [N - 1, N - 2]]).astype(np.int64)                # live rows, a block seam, and two spare rows being published
assert len(np.unique(IDS)) == len(IDS) == 13
EXTRA = _rs.randint(-1, N, (len(IDS), 3)).astype(np.int32)             # the caller's exclusion lists


def _engine(params, content, mw, keys, cat, scoring):
    from tcar_amd.engine import TcarEngine
    eng = TcarEngine(params, content, mw, max_grad=2.0, scoring=scoring)
    eng.set_item_keys(keys)
    eng.set_categories(cat)
    return eng


def _live_engine(scoring, state):
    t = tables()
    eng = _engine(t["params"], t["content"], t["mw"], t["keys"], t["cat"], scoring)
    if state == "trained":
        for _ in range(2):
            eng.train_step(t["batch"])
        eng.flush()
    return eng


def _rebuilt(eng, scoring):
    """a second engine from the host tables and the exported state of `eng`"""
    t = tables()
    st = eng.export_state()
    eng2 = _engine({k[4:]: v for k, v in st.items() if k.startswith("var/")}, t["content"], t["mw"], t["keys"], t["cat"], scoring)
    eng2.load_state(st)
    return eng2


def _calls(eng):
    batch = tables()["batch"]
    feed = R.unlabelled(batch)
    out = {"recommend": _np(*eng.recommend(feed)), "recommend window": _np(*eng.recommend(feed, window=WINDOW, panel=128))}
    out["streamed"] = _np(*eng.eval_step_streamed(batch, panel=256)) + _np(eng.last_scores)
    cand = np.concatenate([np.tile(IDS.astype(np.int32), (B, 1)), np.random.RandomState(5).randint(0, N, (B, 20)).astype(np.int32)], 1)
    res = eng.score_candidates(feed, cand)
    out["candidates"] = _np(res.scores, res.rank_of, res.order)
    return out


def _same_calls(a, b, what):
    assert list(a) == list(b)
    for name in a:
        for i, (x, y) in enumerate(zip(a[name], b[name])):
            assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, name, i)


def _item_table(eng):
    return eng.E[:N, :H].cpu().numpy().copy()


@pytest.mark.parametrize("state", ["fresh", "trained"])
@pytest.mark.parametrize("scoring", ["f32", "bf16x3-mixed"])
def test_lists_rows_and_the_rebuild_contract(scoring, state):
    _need_gpu()
    eng = _live_engine(scoring, state)
    what = "%s, %s" % (scoring, state)
    table = _item_table(eng)
    Mi, Vi = _np(eng.Mi, eng.Vi)
    if state == "trained":
        assert Mi.any() and Vi.any()                                   # there is optimizer history to keep
    U = len(IDS)
    # ---- the lists: similar_items with every named id excluded in every row, then the caller's lists
    excl = np.concatenate([np.tile(IDS.astype(np.int32), (U, 1)), EXTRA], 1)
    want = _np(*eng.similar_items(IDS, k=K, exclude=excl, window=WINDOW))
    ws = eng.warm_start_items(IDS, k=K, min_sim=0.0, exclude=EXTRA, window=WINDOW)
    rows, support, wsum, donors, sims = _np(*ws)
    assert rows.shape == (U, H) and donors.shape == sims.shape == (U, K) and support.shape == wsum.shape == (U,)
    assert donors.tobytes() == want[0].tobytes() and sims.tobytes() == want[1].tobytes(), what
    assert not np.isin(donors, IDS).any() and (donors >= 0).all() and (donors < N - SPARE).all()       # no named id, no spare row
    assert not (donors[:, :, None] == EXTRA[:, None, :]).any()
    # ---- the rows: the fp64 rule over the engine's own item table as it was
    _, (ref, ref_support, ref_wsum) = warm_ref.check_rows(rows, donors, sims, table, 0.0, name="rows " + what)
    assert np.array_equal(support, ref_support) and (np.abs(wsum - ref_wsum) <= K * warm_ref.EPS * ref_wsum).all()
    after = _item_table(eng)
    assert after[IDS].tobytes() == rows.tobytes()                       # installed: the fp32 image holds the rows ...
    keep = np.setdiff1d(np.arange(N), IDS)
    assert after[keep].tobytes() == table[keep].tobytes()               # ... and no other row moved
    assert not eng.E[:N, H:eng.geo.ldh].any()                          # the pad columns of the item block stay zero
    # ---- the moments: zero for the named rows, untouched elsewhere
    Mi2, Vi2 = _np(eng.Mi, eng.Vi)
    assert not Mi2[IDS].any() and not Vi2[IDS].any()
    assert Mi2[keep].tobytes() == Mi[keep].tobytes() and Vi2[keep].tobytes() == Vi[keep].tobytes()
    # ---- the contract of update_items(item_rows = rows): the bits of an engine built from the final tables
    eng2 = _rebuilt(eng, scoring)
    assert eng2.E[:N, :H].cpu().numpy()[IDS].tobytes() == rows.tobytes()
    _same_calls(_calls(eng), _calls(eng2), what)
    # ---- the same bits for another partition into panels (the donors' rows did not move: no named id is a donor)
    again = _np(*eng.warm_start_items(IDS, k=K, exclude=EXTRA, window=WINDOW, panel=128))
    for x, y in zip(again, (rows, support, wsum, donors, sims)):
        assert x.tobytes() == y.tobytes(), (what, "panel 128")
    # ---- a plain update afterwards behaves as before
    new = tables()["new"]["item"][IDS]
    eng.update_items(IDS, item_rows=new)
    assert _item_table(eng)[IDS].tobytes() == new.tobytes()
    _same_calls(_calls(eng), _calls(_rebuilt(eng, scoring)), what + ", update_items after")
    eng.check_forks()


@pytest.mark.parametrize("scoring", ["f32", "bf16x3-mixed"])
def test_an_empty_donor_pool_gives_zero_rows(scoring):
    _need_gpu()
    eng = _live_engine(scoring, "fresh")
    table = _item_table(eng)
    ids = IDS[:5]
    # one window for all rows that holds no key, then a window per row: the odd rows keep their pool
    ws = _np(*eng.warm_start_items(ids, k=K, window=(FAR - 5, FAR - 4)))
    rows, support, wsum, donors, sims = ws
    assert (donors == -1).all() and not sims.any() and not support.any()
    assert rows.tobytes() == np.zeros((5, H), np.float32).tobytes() and wsum.tobytes() == np.zeros(5, np.float32).tobytes()
    assert not _item_table(eng)[ids].any()
    eng.update_items(ids, item_rows=table[ids])
    lo, hi = np.zeros(5, np.int64), np.asarray([0, 10 ** 6, 0, 10 ** 6, 0])
    rows, support, _, donors, _ = _np(*eng.warm_start_items(ids, k=K, window=(lo, hi)))
    assert support.tolist() == [0, K, 0, K, 0] and not rows[::2].any() and rows[1].any() and rows[3].any()
    # min_sim above every cosine of random rows (about 1 / sqrt(250)): the lists are full and nobody donates
    rows, support, wsum, donors, sims = _np(*eng.warm_start_items(ids, k=K, min_sim=0.9, window=WINDOW))
    assert (donors >= 0).all() and (sims < 0.9).all() and not support.any() and not rows.any() and not wsum.any()
    _same_calls(_calls(eng), _calls(_rebuilt(eng, scoring)), scoring + ", zero rows")


def test_the_op_level_blend_is_the_kernel_of_the_call():
    _need_gpu()
    eng = _live_engine("f32", "fresh")
    table = eng.E[:N, :H]                                              # a view with the row stride of E
    ws = eng.warm_start_items(IDS, k=K, window=WINDOW)
    donors, sims, rows = ws.donors.clone(), ws.sims.clone(), ws.rows.clone()
    eng.update_items(IDS, item_rows=tables()["params"]["item_emb"][1 + IDS])       # (nothing named donates: the table is as it was for the blend)
    got, support, wsum = eng.rows_blend(donors, sims, table, 0.0)
    assert torch.equal(got, rows) and torch.equal(support, ws.support) and torch.equal(wsum, ws.wsum)


# ------------------------------------------------------------------------------------------------ planted structure
CLUSTERS, RADIUS, P_MIN_SIM = 8, 0.05, 0.5


def _planted():
    """content = unit centroid of the row's cluster + noise (cosines: about 0.94 inside a cluster, about 0.06 across), item row =
    item centroid of the cluster + a vector of norm exactly RADIUS (in fp64; the fp32 row is within 1e-7 of it)"""
    rng = np.random.RandomState(23)
    cluster = np.arange(N) % CLUSTERS
    cen = rng.standard_normal((CLUSTERS, H))
    cen /= np.linalg.norm(cen, axis=1, keepdims=True)
    content = (cen[cluster] + 0.35 / np.sqrt(H) * rng.standard_normal((N, H))).astype(np.float32)
    icen = 0.35 * rng.standard_normal((CLUSTERS, H))
    noise = rng.standard_normal((N, H))
    noise *= RADIUS / np.linalg.norm(noise, axis=1, keepdims=True)
    item = (icen[cluster] + noise).astype(np.float32)
    hidden = np.asarray([c + CLUSTERS * (3 + 5 * c) for c in range(CLUSTERS)], np.int64)      # one row of every cluster
    return cluster, content, item, icen, hidden


def test_hidden_rows_of_a_clustered_catalog_come_back_inside_the_noise_radius():
    _need_gpu()
    cluster, content, item, icen, hidden = _planted()
    # ---- on the CPU first: the reference lists and the reference rows
    S = sims_f32(content[hidden], content)
    topk, score = lists(S, K, excl=[hidden.tolist()] * CLUSTERS)
    assert (topk >= 0).all() and (cluster[topk] == cluster[hidden][:, None]).all()          # same-cluster donors only ...
    across = cluster[None, :] != cluster[hidden][:, None]
    assert score.min() > P_MIN_SIM + 0.2 and S[across].max() < P_MIN_SIM - 0.2              # ... clear of min_sim on both sides
    ref, support, _, _ = warm_ref.blend(topk, score, item, P_MIN_SIM)
    d_ref = np.linalg.norm(ref - icen[cluster[hidden]], axis=1)
    assert (support == K).all() and (d_ref < RADIUS).all(), d_ref
    # ---- the engine: the hidden rows are overwritten with garbage first, as a spare row's would be
    t = tables()
    params = {k: v.copy() for k, v in t["params"].items()}
    params["item_emb"][1:] = item
    params["item_emb"][1 + hidden] = 3.0
    full = np.concatenate([np.zeros((1, H), np.float32), content])
    for scoring in ("f32", "bf16x3-mixed"):
        eng = _engine(params, full, t["mw"], t["keys"], t["cat"], scoring)
        rows, sup, _, donors, sims = _np(*eng.warm_start_items(hidden, k=K, min_sim=P_MIN_SIM))
        assert (cluster[donors] == cluster[hidden][:, None]).all() and (sup == K).all() and not np.isin(donors, hidden).any()
        d = np.linalg.norm(rows.astype(np.float64) - icen[cluster[hidden]], axis=1)
        print(scoring, "distance to the centroid / noise radius:", np.round(d / RADIUS, 3))
        assert (d < RADIUS).all(), d
