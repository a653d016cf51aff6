"""In-place catalog updates on the GPU (include/tcar_catalog.h, TcarEngine.update_items).  The contract is the strongest this project
uses — THE SAME BITS as buffers, or an engine, built from scratch from the final tables — so almost every comparison here is
torch.equal / tobytes; the one tolerance (test 3) is the project's gate for scores against the fp64 oracle (tests/serve_shapes_ref.py).

Shapes: N = 700 (Npad = 768, the last 128-row block holds 60 live rows), H = 250 (ldh = 256: the pad columns 250 .. 255 of both blocks
are live hazards), Ht = 64, B = 8, T = 5.  Id sets: [0], [N - 1], [127, 128] (a block seam), one whole block, 37 scattered ids in
random order, all N rows in reversed order.

  1  tcar_catalog_update on raw buffers against tcar_split_bf16 / tcar_cand_time_fwd_bf16 / tcar_time_onehot over the final tables:
     every buffer, byte for byte, canary words behind each included; fp32 and plane contexts, refresh_time 0 and 1.
  2  an updated engine (fresh / trained with a dirty time block / trained with a clean one) against a second engine built from the final
     host tables and the first one's exported state: every serving call, then one training step and the whole exported state.
  3  the scores of the updated rows against an fp64 numpy dot of the final tables — and the same check refused over the old tables.
  4  the publishing idiom: spare rows outside every window, published into it, retired again.
  5  no whole-catalog refresh follows an update of a clean engine."""
import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401

import serve_shapes_ref as R
from catalog_case import (B, CANARY, EK, FAR, H, N, NPAD, SPARE, T, Raw, _bytes, _device_payload, _moments, _update, final_tables,
                          tables)
from gpu_util import _need_gpu, _np, lib  # noqa: F401  (lib: the module-scoped fixture)

pytestmark = pytest.mark.gpu

_rs = np.random.RandomState(7).permutation(N)
ID_SETS = {"first": [0], "last": [N - 1], "seam": [127, 128], "block": list(range(256, 384)),
           "scattered": _rs[:37].tolist(), "all-reversed": list(range(N - 1, -1, -1))}
ENGINE_IDS = ID_SETS["scattered"] + [i for i in (127, 128) if i not in ID_SETS["scattered"]]


# ----------------------------------------------------------------------------------- 1  the kernel, raw bytes
def _same_buffers(got, want, what):
    for name in got.names():
        g, w = got.whole[name], want.whole[name]
        assert torch.equal(_bytes(g), _bytes(w)), "%s: %s differs in %d words" % (what, name, int((g != w).sum()))
        assert bool((g[-CANARY:] == 0x5A5A5A5A).all()), (what, name, "canary")
    assert not bool(got.E.view(NPAD, EK)[N:].any()), (what, "padding rows of E")
    if got.planes:
        # rows [N, Npad) of the last block: the blocked layout keeps a row's pieces 64 bytes apart, so compare with a plane built from zeros
        for p in (got.eh, got.el):
            blk = p.view(NPAD // 128, EK // 32, 128, 32)[-1, :, N % 128:, :]
            assert not bool(blk.view(torch.int16).any()), (what, "padding rows of the planes")
    assert not bool(got.oh.view(NPAD // 128, 5, 128, 32)[-1, :, N % 128:, :].view(torch.int16).any()), (what, "padding rows of the one-hot plane")


@pytest.mark.parametrize("refresh", [0, 1])
@pytest.mark.parametrize("planes", [False, True], ids=["f32", "planes"])
@pytest.mark.parametrize("name", list(ID_SETS))
def test_the_kernel_leaves_the_bytes_of_buffers_built_from_the_final_tables(lib, name, planes, refresh):
    t, ids = tables(), ID_SETS[name]
    mom = _moments()
    got = Raw(lib, planes, t["params"]["item_emb"][1:], t["content"][1:], t["mw"], t["keys"], t["cat"], moments=mom)
    _update(lib, got, _device_payload(ids), refresh)
    params, content, mw, keys, cat = final_tables(ids, "mw_wild")
    m, v = mom[0].copy(), mom[1].copy()
    m[ids], v[ids] = 0, 0
    # refresh_time = 0: the time block keeps the OLD publish times (the caller owes a whole refresh), everything else is final
    want = Raw(lib, planes, params["item_emb"][1:], content[1:], mw, keys, cat, time_mw=None if refresh else t["mw"], moments=(m, v))
    _same_buffers(got, want, "%s planes=%s refresh=%d" % (name, planes, refresh))


@pytest.mark.parametrize("planes", [False, True], ids=["f32", "planes"])
def test_a_table_the_call_does_not_bring_keeps_every_byte(lib, planes):
    t, ids = tables(), ID_SETS["scattered"] + [127, 128, N - 1]
    mom = _moments()
    old = lambda: Raw(lib, planes, t["params"]["item_emb"][1:], t["content"][1:], t["mw"], t["keys"], t["cat"], moments=mom)
    params, content, mw, keys, cat = final_tables(ids, "mw_wild")
    pay = _device_payload(ids, ld=256)
    # content alone: the item block, the time block, the moments and the small tables are the old ones
    got = old()
    _update(lib, got, pay, 1, item=False, mw=False, keys=False, cat=False)
    _same_buffers(got, Raw(lib, planes, t["params"]["item_emb"][1:], content[1:], t["mw"], t["keys"], t["cat"], moments=mom), "content alone")
    # keys and categories alone
    got = old()
    _update(lib, got, pay, 0, item=False, content=False, mw=False)
    _same_buffers(got, Raw(lib, planes, t["params"]["item_emb"][1:], t["content"][1:], t["mw"], keys, cat, moments=mom), "keys and categories")
    # publish times alone, refreshed
    got = old()
    _update(lib, got, pay, 1, item=False, content=False, keys=False, cat=False)
    _same_buffers(got, Raw(lib, planes, t["params"]["item_emb"][1:], t["content"][1:], mw, t["keys"], t["cat"], moments=mom), "publish times")
    # an id outside the catalog names no row
    got = old()
    stray = dict(pay, ids=torch.tensor([N, -1, 2 ** 31 - 1] + [0] * (len(ids) - 3), dtype=torch.int32, device="cuda:0")[:3])
    _update(lib, got, stray, 1)
    _same_buffers(got, old(), "ids outside the catalog")


# ------------------------------------------------------------------------ 2  an updated engine against a fresh one
def _engine(params, content, mw, keys, cat, scoring):
    from tcar_amd.engine import TcarEngine
    eng = TcarEngine(params, content, mw, max_grad=2.0, scoring=scoring)
    eng.set_item_keys(keys)
    eng.set_categories(cat)
    return eng


def _updated_engine(scoring, state, ids=ENGINE_IDS):
    """an engine over the OLD tables brought into `state`, then updated to the final tables of `ids`"""
    t = tables()
    eng = _engine(t["params"], t["content"], t["mw"], t["keys"], t["cat"], scoring)
    if state != "fresh":
        for _ in range(2):
            eng.train_step(t["batch"])
        assert eng._time_dirty
        if state == "clean":
            eng.recommend(R.unlabelled(t["batch"]))
            assert not eng._time_dirty
    dirty = eng._time_dirty
    new, i = t["new"], np.asarray(ids)
    eng.update_items(ids, content=new["content"][i], item_rows=new["item"][i], mwdhm=new["mw"][i], keys=new["keys"][i], categories=new["cat"][i])
    assert eng._time_dirty == dirty                     # an update never dirties a clean time block (and cannot clean a dirty one)
    return eng


def _rebuilt_engine(eng, ids, scoring):
    """a second engine from the final host tables and the exported state of `eng`"""
    _, content, mw, keys, cat = final_tables(ids)
    st = eng.export_state()
    eng2 = _engine({k[4:]: v for k, v in st.items() if k.startswith("var/")}, content, mw, keys, cat, scoring)
    eng2.load_state(st)
    return eng2


def _calls(eng):
    """every serving call -> {name: [numpy arrays]}"""
    from tcar_amd.host.data import pack_sessions
    batch = tables()["batch"]
    feed = R.unlabelled(batch)
    out = {}
    out["eval_step"] = _np(*eng.eval_step(batch))
    for tag, kw in (("plain", {}), ("window", dict(window=(1000, 600000))), ("cap", dict(max_per_category=2)), ("panel", dict(panel=128))):
        out["streamed " + tag] = _np(*eng.eval_step_streamed(batch, **kw)) + _np(eng.last_scores)
    out["recommend"] = _np(*eng.recommend(feed))
    out["retrieve"] = _np(*eng.retrieve(feed, 64))
    out["two-stage"] = _np(*eng.recommend_two_stage(feed, shortlist=64))
    rng = np.random.RandomState(5)
    cand = np.concatenate([np.tile(np.asarray(ENGINE_IDS[:20], np.int32), (B, 1)), rng.randint(0, N, (B, 20)).astype(np.int32)], 1)
    res = eng.score_candidates(feed, cand)
    out["candidates"] = _np(res.scores, res.rank_of, res.order)
    cut = lambda lo, hi, n: dict({k: batch[k][lo:hi, :n] for k in R.PER_ROW}, **{k: batch[k][lo:hi] for k in ("cw", "ch", "label")})
    ragged = pack_sessions([cut(0, 3, T), cut(3, 6, 2), cut(6, 8, 1)])
    out["ragged recommend"] = _np(*eng.recommend(R.unlabelled(ragged)))
    return out


def _same_calls(a, b, what):
    assert list(a) == list(b)
    for name in a:
        for i, (x, y) in enumerate(zip(a[name], b[name])):
            assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, name, i)


@pytest.mark.parametrize("state", ["fresh", "dirty", "clean"])
@pytest.mark.parametrize("scoring", ["f32", "bf16x3-mixed"])
def test_an_updated_engine_is_the_engine_built_from_the_final_tables(scoring, state):
    _need_gpu()
    eng = _updated_engine(scoring, state)
    eng2 = _rebuilt_engine(eng, ENGINE_IDS, scoring)
    what = "%s, %s" % (scoring, state)
    _same_calls(_calls(eng), _calls(eng2), what)
    # one training step in both: the rebuilt index, the one-hot rows and the zeroed moments.  The split-bf16 step adds every gradient
    # in a fixed order and takes all eight sessions.  The fp32 step adds the residual-weight and bias gradients of the sessions with
    # float atomics (engine.ATOMIC_IN_F32): with three or more terms the order is the scheduler's, and two identical engines differ in
    # the last bits of exactly those variables (measured here with B = 8, and what tests/test_gpu_configs.py reports for one engine
    # run twice).  Its step takes the first two sessions: a sum of two terms has no order.
    batch = tables()["batch"]
    if scoring == "f32":
        batch = {k: v[:2] for k, v in batch.items()}
    assert eng._index_stale
    l1, l2 = _np(eng.train_step(batch))[0], _np(eng2.train_step(batch))[0]
    assert not eng._index_stale
    assert l1.tobytes() == l2.tobytes(), (what, "loss")
    s1, s2 = eng.export_state(), eng2.export_state()
    assert sorted(s1) == sorted(s2)
    differ = [k for k in s1 if np.asarray(s1[k]).tobytes() != np.asarray(s2[k]).tobytes()]
    print(what, "state arrays that differ:", differ)
    assert not differ, (what, differ)
    eng.check_forks()
    eng2.check_forks()


# ------------------------------------------------------------------- 3  independent of the code under test
@pytest.mark.parametrize("scoring", ["f32", "bf16x3-mixed"])
def test_the_updated_rows_score_as_an_fp64_dot_of_the_final_tables(scoring):
    _need_gpu()
    from oracle.tcar_oracle import TcarOracle
    t = tables()
    eng = _updated_engine(scoring, "fresh")
    feed = R.unlabelled(t["batch"])
    cand = np.tile(np.asarray(ENGINE_IDS, np.int32), (B, 1))
    res = eng.score_candidates(feed, cand)
    scores, rank_of, order = _np(res.scores, res.rank_of, res.order)

    def ref(params, content, mw, name):
        r = R._forward(TcarOracle(params, content, mw), t["batch"])           # the oracle's clip, its attout and its candidate rows
        s = r["A"] @ r["E"].T                                                  # the fp64 numpy dot
        assert np.abs(s - r["s"]).max() <= 1e-9 * np.abs(r["s"]).max()
        return dict(s=s, delta=1e-3 * np.abs(s).max(1), name=name)
    params, content, mw, _, _ = final_tables(ENGINE_IDS)
    final, old = ref(params, content, mw, "final tables"), ref(t["params"], t["content"], t["mw"], "old tables")
    R.check_candidates(final, cand, scores, rank_of, order, name="updated rows, %s" % scoring)
    print({k: round(v, 4) for k, v in R.WORST.items() if k.startswith("final tables")})
    # the rows moved by far more than the gate: the same scores are refused over the tables they replaced
    assert np.abs(final["s"][:, ENGINE_IDS] - old["s"][:, ENGINE_IDS]).max() > 100 * final["delta"].max()
    with pytest.raises(AssertionError):
        R.check_candidates(old, cand, scores, rank_of, order, name="updated rows against the OLD tables")


# ---------------------------------------------------------------------------------- 4  the publishing idiom
@pytest.mark.parametrize("scoring", ["f32", "bf16x3-mixed"])
def test_spare_rows_are_published_into_the_window_and_retired_again(scoring):
    _need_gpu()
    from oracle.tcar_oracle import TcarOracle
    t = tables()
    batch, feed = t["batch"], R.unlabelled(t["batch"])
    window, spare = (0, 10 ** 6), np.arange(N - SPARE, N)
    eng = _engine(t["params"], t["content"], t["mw"], t["keys"], t["cat"], scoring)
    listed = lambda: _np(eng.recommend(feed, window=window)[0])[0]
    assert not np.isin(listed(), spare).any()                     # a spare row is in no pool
    # the article a session likes best, by the fp64 oracle: its item | content part must be positive, so that 1.5 times it beats it
    r = R._forward(TcarOracle(t["params"], t["content"], t["mw"]), batch)
    s = r["s"].copy()
    s[:, spare] = -np.inf
    s[np.arange(B)[:, None], batch["seq"] - 1] = -np.inf           # exclude_seen
    top1 = s.argmax(1)
    part = np.einsum("bk,bk->b", r["A"][:, :2 * H], r["E"][top1][:, :2 * H])
    assert (part > 20 * 1e-3 * np.abs(r["s"]).max(1)).all()        # (clear of the logits gate: the engine cannot order them otherwise)
    pub = spare[:10]
    src = top1[np.arange(10) % B]
    params = t["params"]
    eng.update_items(pub, content=1.5 * t["content"][1 + src], item_rows=1.5 * params["item_emb"][1 + src], mwdhm=t["mw"][src],
                     keys=np.full(10, 500000), categories=t["cat"][src])
    now = listed()
    for j, row in enumerate(pub):
        assert row in now[j % B], (j, row, now[j % B])             # published: it beats the article it was copied from
    assert not np.isin(now, spare[10:]).any()
    eng.update_items(pub, keys=np.full(10, FAR))                   # retired: the key moves out of every window
    after = listed()
    assert not np.isin(after, spare).any()
    # and the engine is the one built from the final tables
    p2 = {k: v.copy() for k, v in params.items()}
    content, mw, cat = t["content"].copy(), t["mw"].copy(), t["cat"].copy()
    p2["item_emb"][1 + pub] = 1.5 * params["item_emb"][1 + src]
    content[1 + pub], mw[pub], cat[pub] = 1.5 * t["content"][1 + src], t["mw"][src], t["cat"][src]
    fresh = _engine(p2, content, mw, t["keys"], cat, scoring)
    for kw in (dict(window=window), dict(), dict(window=window, max_per_category=2)):
        a, b = _np(*eng.recommend(feed, **kw)), _np(*fresh.recommend(feed, **kw))
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), kw


# ------------------------------------------------------------------------------------- 5  no stray refresh
@pytest.mark.parametrize("scoring", ["f32", "bf16x3-mixed"])
def test_no_whole_catalog_refresh_follows_an_update_of_a_clean_engine(scoring):
    _need_gpu()
    t = tables()
    feed = R.unlabelled(t["batch"])
    eng = _updated_engine(scoring, "clean")
    assert not eng._time_dirty
    got = _np(*eng.recommend(feed))                                 # runs with refresh_time = 0: the row refresh made the time block right
    assert not eng._time_dirty
    _, content, mw, keys, cat = final_tables(ENGINE_IDS)
    fresh = _engine(eng.export_params(), content, mw, keys, cat, scoring)
    want = _np(*fresh.recommend(feed))
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    # had the rows kept their old time vectors they would score otherwise: an engine with the old publish times disagrees on them
    cand = np.tile(np.asarray(ENGINE_IDS, np.int32), (B, 1))
    stale = _engine(eng.export_params(), content, t["mw"], keys, cat, scoring)
    s_got, s_want, s_stale = (_np(e.score_candidates(feed, cand).scores)[0] for e in (eng, fresh, stale))
    assert s_got.tobytes() == s_want.tobytes() and (s_stale != s_want).mean() > 0.9
