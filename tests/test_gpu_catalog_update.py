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
import ctypes as C

import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401
from tcar_amd import _lib

import serve_shapes_ref as R
from select_util import _need_gpu

pytestmark = pytest.mark.gpu

N, H, HT, B, T = 700, 250, 64, 8, 5
LDH, LDT = 256, 64
EK, NPAD = 2 * LDH + 5 * LDT, 768
SPARE = 50                                   # the last rows of the catalog: no session has read them
VOCAB = (13, 32, 8, 25, 61)
CANARY = 64                                  # 4-byte words behind every raw buffer
FAR = 2 ** 31 - 2                            # a key above every window's hi

_rs = np.random.RandomState(7).permutation(N)
ID_SETS = {"first": [0], "last": [N - 1], "seam": [127, 128], "block": list(range(256, 384)),
           "scattered": _rs[:37].tolist(), "all-reversed": list(range(N - 1, -1, -1))}
ENGINE_IDS = ID_SETS["scattered"] + [i for i in (127, 128) if i not in ID_SETS["scattered"]]

_T = {}


def tables():
    """The OLD catalog — (params, content [N + 1, H], mw [N, 5], keys [N], cat [N], batch) — and, for every row, its replacement:
    new[...] indexed by 0-based id.  Computed once, never written."""
    if not _T:
        from oracle.tcar_oracle import init_params_numpy
        rng = np.random.RandomState(2024)
        params = init_params_numpy(N, H, HT, 0.35, 0.12, rng)
        for k, name in enumerate(("month", "day", "week", "hour", "minute")):      # some time rows inside the unit ball, some outside
            params[name + "_embedding"][::2] *= 0.05
        content = (rng.standard_normal((N + 1, H)) * 0.5).astype(np.float32)
        content[0] = 0
        draw_mw = lambda: np.stack([rng.randint(0, v, N) for v in VOCAB], -1).astype(np.int32)
        mw = draw_mw()
        keys = rng.randint(0, 10 ** 6, N).astype(np.int32)
        keys[N - SPARE:] = FAR
        cat = rng.randint(0, 9, N).astype(np.int32)
        live = N - SPARE
        b = {"seq": rng.randint(1, live + 1, (B, T)), "label": rng.randint(0, live, B), "pm": rng.randint(1, 13, (B, T)),
             "pd": rng.randint(1, 32, (B, T)), "pw": rng.randint(1, 8, (B, T)), "ph": rng.randint(1, 25, (B, T)),
             "pmi": rng.randint(1, 61, (B, T)), "cw": rng.randint(0, 7, B), "ch": rng.randint(0, 24, B),
             "gap": rng.randint(0, 12, (B, T)), "neg": rng.randint(0, live, (B, R.NEG))}
        b = {k: v.astype(np.int32) for k, v in b.items()}
        new = dict(content=(rng.standard_normal((N, H)) * 0.5).astype(np.float32),
                   item=(rng.standard_normal((N, H)) * 0.35).astype(np.float32), mw=draw_mw(),
                   keys=rng.randint(0, 10 ** 6, N).astype(np.int32), cat=rng.randint(0, 9, N).astype(np.int32))
        new["mw_wild"] = new["mw"].copy()                                     # (the raw-buffer tests: the oracle does not clamp)
        new["mw_wild"][::7] = [-3, 40, 8, 99, -1]                             # ids outside the vocabularies: clamped for the look-up
        # every replacement row is at distance >= 1 from the row it replaces (test 3 rests on it)
        assert np.linalg.norm(new["content"] - content[1:], axis=1).min() >= 1 and np.linalg.norm(new["item"] - params["item_emb"][1:], axis=1).min() >= 1
        for a in list(params.values()) + [content, mw, keys, cat] + list(b.values()) + list(new.values()):
            a.setflags(write=False)
        _T.update(params=params, content=content, mw=mw, keys=keys, cat=cat, batch=b, new=new)
    return _T


def final_tables(ids, mw_from="mw"):
    """the host tables after the rows `ids` took their replacements: (params, content, mw, keys, cat)"""
    t, ids = tables(), np.asarray(ids)
    params = {k: v.copy() for k, v in t["params"].items()}
    content, mw, keys, cat = t["content"].copy(), t["mw"].copy(), t["keys"].copy(), t["cat"].copy()
    params["item_emb"][1 + ids] = t["new"]["item"][ids]
    content[1 + ids], mw[ids], keys[ids], cat[ids] = t["new"]["content"][ids], t["new"][mw_from][ids], t["new"]["keys"][ids], t["new"]["cat"][ids]
    return params, content, mw, keys, cat


def _bytes(t):
    return t.contiguous().view(-1).view(torch.uint8)


# ----------------------------------------------------------------------------------- 1  the kernel, raw bytes
def _guarded(numel, dtype, dev):
    """a buffer of `numel` elements with CANARY 4-byte words behind it -> (whole allocation as int32 words, the buffer)"""
    nbytes = numel * torch.empty((), dtype=dtype).element_size()
    assert nbytes % 4 == 0
    whole = torch.full((nbytes // 4 + CANARY,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    buf = whole[:nbytes // 4].view(dtype)
    buf.zero_()
    return whole, buf


class Raw:
    """The catalog side of a context, built with the existing entry points alone from host tables: E, the planes (plane contexts),
    mwdhm, key / category tables, Mi / Vi, the one-hot plane — each with canary words behind it."""

    def __init__(self, lib, planes, item, content, mw, keys, cat, time_mw=None, moments=None):
        dev = torch.device("cuda:0")
        self.lib, self.planes, self.whole = lib, planes, {}
        for name, numel, dt in (("E", NPAD * EK, torch.float32), ("eh", NPAD * EK, torch.bfloat16), ("el", NPAD * EK, torch.bfloat16),
                                ("mw", N * 5, torch.int32), ("keys", N, torch.int32), ("cat", N, torch.int32),
                                ("Mi", N * LDH, torch.float32), ("Vi", N * LDH, torch.float32), ("oh", NPAD * 160, torch.bfloat16)):
            self.whole[name], buf = _guarded(numel, dt, dev)
            setattr(self, name, buf)
        E = self.E.view(NPAD, EK)
        E[:N, :H].copy_(torch.from_numpy(np.ascontiguousarray(item)))
        E[:N, LDH:LDH + H].copy_(torch.from_numpy(np.ascontiguousarray(content)))
        self.mw.copy_(torch.from_numpy(mw.reshape(-1)))
        self.keys.copy_(torch.from_numpy(keys))
        self.cat.copy_(torch.from_numpy(cat))
        if moments is not None:
            self.Mi.copy_(torch.from_numpy(moments[0].reshape(-1)))
            self.Vi.copy_(torch.from_numpy(moments[1].reshape(-1)))
        # the five time tables as an arena: W = month | day | week | hour | minute, off[TCAR_V_MONTH + k]
        p = tables()["params"]
        self.W = torch.from_numpy(np.concatenate([p[n].reshape(-1) for n in ("month_embedding", "day_embedding", "week_embedding",
                                                                            "hour_embedding", "minute_embedding")])).to(dev)
        self.off = np.concatenate([[0], np.cumsum([v * HT for v in VOCAB])[:-1]])
        self.dims = _lib.Dims(N, H, HT, LDH, LDT)
        tt = (C.c_void_p * 5)(*[self.W.data_ptr() + 4 * int(o) for o in self.off])
        vp = lambda t: C.c_void_p(t.data_ptr())
        if planes:
            _lib.check(lib.tcar_split_bf16(vp(self.E), EK, N, EK, vp(self.eh), vp(self.el), EK, None, None, 0, 0, 0, None), "split")
        tmw = self.mw if time_mw is None else torch.from_numpy(time_mw.reshape(-1).copy()).to(dev)
        _lib.check(lib.tcar_cand_time_fwd_bf16(C.byref(self.dims), C.byref(tt), vp(tmw), None if planes else vp(self.E), vp(self.eh) if planes else None,
                                               vp(self.el) if planes else None, None), "cand_time_fwd")
        _lib.check(lib.tcar_time_onehot(C.byref(self.dims), vp(self.mw), vp(self.oh), 160, None), "onehot")
        torch.cuda.synchronize()

    def ctx(self):
        c = _lib.Ctx()
        c.d, c.scoring = self.dims, 3 if self.planes else 0
        c.E, c.W, c.Mi, c.Vi, c.mwdhm = (t.data_ptr() for t in (self.E, self.W, self.Mi, self.Vi, self.mw))
        if self.planes:
            c.e16h, c.e16l = self.eh.data_ptr(), self.el.data_ptr()
        for k in range(5):
            c.off[1 + k] = int(self.off[k])              # TCAR_V_MONTH = 1
        return c

    def names(self):
        return [n for n in self.whole if self.planes or n not in ("eh", "el")]


def _moments():
    rng = np.random.RandomState(11)
    return rng.standard_normal((N, LDH)).astype(np.float32), rng.random_sample((N, LDH)).astype(np.float32) + 0.5


def _device_payload(ids, ld=252):
    """the replacement rows of `ids` on the device, the float tables with a row stride of `ld` >= H floats (the slack poisoned)"""
    t, ids, dev = tables()["new"], np.asarray(ids), torch.device("cuda:0")

    def rows(x):
        out = np.full((len(ids), ld), np.nan, np.float32)
        out[:, :H] = x[ids]
        return torch.from_numpy(out).to(dev)
    i32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(dev)
    return dict(ids=i32(ids), item=rows(t["item"]), content=rows(t["content"]), mw=i32(t["mw_wild"][ids]), keys=i32(t["keys"][ids]),
                cat=i32(t["cat"][ids]), ld=ld)


def _update(lib, raw, pay, refresh, item=True, content=True, mw=True, keys=True, cat=True):
    d = _lib.CatalogUpdate()
    d.U, d.ids = int(pay["ids"].numel()), pay["ids"].data_ptr()
    if item:
        d.item, d.ld_item, d.zero_moments = pay["item"].data_ptr(), pay["ld"], 1
    if content:
        d.content, d.ld_content = pay["content"].data_ptr(), pay["ld"]
    if mw:
        d.mwdhm, d.onehot, d.onehot_inner = pay["mw"].data_ptr(), raw.oh.data_ptr(), 160
    d.refresh_time = refresh
    if keys:
        d.key, d.key_table = pay["keys"].data_ptr(), raw.keys.data_ptr()
    if cat:
        d.cat, d.cat_table = pay["cat"].data_ptr(), raw.cat.data_ptr()
    _lib.check(lib.tcar_catalog_update(C.byref(raw.ctx()), C.byref(d), None), "tcar_catalog_update")
    torch.cuda.synchronize()


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


@pytest.fixture(scope="module")
def lib():
    _need_gpu()
    return _lib.load()


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
def _np(*ts):
    return [t.cpu().numpy().copy() for t in ts]


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
