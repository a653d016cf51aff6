"""Catalog updates on the catalog-sharded and the replica engines, on the GPU (include/tcar_catalog_shard.h,
ShardedEngine.shard_update_items, DPEngine.replica_update_items).  The contract is that of tests/test_gpu_catalog_update.py — THE SAME
BITS as buffers, or engines, built from scratch from the final tables — so every comparison but one is torch.equal / tobytes; the one
tolerance (test 3) is the project's gate for scores against the fp64 oracle (tests/serve_shapes_ref.py).

Shapes and tables: those of catalog_case (N = 700, H = 250 / ldh = 256, Ht = 64, B = 8, T = 5).  Shards: W = 2 holds rows
384 / 316 — rank 0's buffers END at its last owned row, the canary directly behind; rank 1 has 68 padding rows that must stay zero —,
W = 3 holds 256 / 256 / 188.  Id sets: [0], [N - 1], the seams [383, 384] and [255, 256, 511, 512], rows 256 .. 383 (ONE shard at
either W: the other ranks own nothing), 37 scattered ids in random order, all N rows reversed.

  1  tcar_catalog_update_owned on raw canary-guarded buffers of every (W, rank) against tcar_split_bf16 / tcar_cand_time_fwd_bf16 /
     tcar_time_onehot over that shard of the final tables; with (0, N) against the bytes tcar_catalog_update leaves.
  2  W engines in one process (the collectives played by hand), fresh / trained with a dirty time block / trained with a clean one,
     updated, against W engines built from the final host tables and the final state: buffers, the rebuilt index, every serving call;
     at W = 1 also one training step (of one session: _one_session) and the whole exported state.
  3  the scores of the updated rows against an fp64 numpy dot of the final tables — and the same check refused over the old tables.
  4  the publishing idiom over shards: spare rows in the last shard, published into the lists of every rank's sessions, retired again.
  5  DPEngine.replica_update_items without a group against TcarEngine.update_items.
  6  two ranks over gloo on one device: agreement, then the bits of the in-process engines; a request that differs in one element on
     rank 1 raises on both ranks and leaves every catalog buffer as it was."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401
from tcar_amd import _lib

import serve_shapes_ref as R
from catalog_case import (B, CANARY, EK, FAR, H, HT, LDH, LDT, N, NPAD, SPARE, T, VOCAB, Raw, _bytes, _device_payload, _guarded, _moments,
                          final_tables, tables)
from catalog_case import _update as _update_whole
from dist_util import launch
from gpu_util import _need_gpu, _np, lib  # noqa: F401  (lib: the module-scoped fixture)
from shard_case import play, play_candidates, play_retrieve, split

pytestmark = pytest.mark.gpu

_ru = lambda x, m: (x + m - 1) // m * m
SHARDS = {w: [(r * _ru(-(-N // w), 128), min(N, (r + 1) * _ru(-(-N // w), 128)) - r * _ru(-(-N // w), 128)) for r in range(w)] for w in (1, 2, 3)}
assert SHARDS[2] == [(0, 384), (384, 316)] and SHARDS[3] == [(0, 256), (256, 256), (512, 188)]
_rs = np.random.RandomState(7).permutation(N)
ID_SETS = {"first": [0], "last": [N - 1], "seams-2": [383, 384], "seams-3": [255, 256, 511, 512], "one-shard": list(range(256, 384)),
           "scattered": _rs[:37].tolist(), "all-reversed": list(range(N - 1, -1, -1))}
ENGINE_IDS = ID_SETS["scattered"] + [i for i in (0, 127, 128, 255, 256, 383, 384, 511, 512, N - 1) if i not in ID_SETS["scattered"]]
SPLITS = {1: ([8], 8), 2: ([5, 3], 6), 3: ([3, 0, 5], 5)}       # sessions per rank (uneven, one rank with none at W = 3) and cap
TOPK, PANEL, SHORT = 20, 128, 64
WINDOW = (1000, 600000)
_split = functools.partial(split, splits=SPLITS)       # shard_case.split over the split sizes of THIS module


# ----------------------------------------------------------------------------------- 1  the kernel, raw bytes
class ShardRaw:
    """What a rank that owns the rows [n0, n0 + nl) holds of the catalog, built with the existing entry points alone from host
    tables: E whole, the key / category tables whole, a whole publish-time table; the planes, the publish times, the moments and the
    one-hot plane of the shard — each with canary words behind it."""

    def __init__(self, lib, n0, nl, item, content, mw, keys, cat, time_mw=None, moments=None):
        dev = torch.device("cuda:0")
        nlpad = _ru(nl, 128)
        self.lib, self.n0, self.nl, self.nlpad, self.whole = lib, n0, nl, nlpad, {}
        for name, numel, dt in (("E", NPAD * EK, torch.float32), ("eh", nlpad * EK, torch.bfloat16), ("el", nlpad * EK, torch.bfloat16),
                                ("mw", nl * 5, torch.int32), ("mw_all", N * 5, torch.int32), ("keys", N, torch.int32), ("cat", N, torch.int32),
                                ("Mi", nl * LDH, torch.float32), ("Vi", nl * LDH, torch.float32), ("oh", nlpad * 160, torch.bfloat16)):
            self.whole[name], buf = _guarded(numel, dt, dev)
            setattr(self, name, buf)
        E = self.E.view(NPAD, EK)
        E[:N, :H].copy_(torch.from_numpy(np.ascontiguousarray(item)))
        E[:N, LDH:LDH + H].copy_(torch.from_numpy(np.ascontiguousarray(content)))
        self.mw.copy_(torch.from_numpy(np.ascontiguousarray(mw[n0:n0 + nl]).reshape(-1)))
        self.mw_all.copy_(torch.from_numpy(mw.reshape(-1)))
        self.keys.copy_(torch.from_numpy(keys))
        self.cat.copy_(torch.from_numpy(cat))
        if moments is not None:
            self.Mi.copy_(torch.from_numpy(np.ascontiguousarray(moments[0][n0:n0 + nl]).reshape(-1)))
            self.Vi.copy_(torch.from_numpy(np.ascontiguousarray(moments[1][n0:n0 + nl]).reshape(-1)))
        p = tables()["params"]
        self.W = torch.from_numpy(np.concatenate([p[n].reshape(-1) for n in ("month_embedding", "day_embedding", "week_embedding",
                                                                            "hour_embedding", "minute_embedding")])).to(dev)
        self.off = np.concatenate([[0], np.cumsum([v * HT for v in VOCAB])[:-1]])
        self.dims, loc = _lib.Dims(N, H, HT, LDH, LDT), _lib.Dims(nl, H, HT, LDH, LDT)
        tt = (C.c_void_p * 5)(*[self.W.data_ptr() + 4 * int(o) for o in self.off])
        vp = lambda t: C.c_void_p(t.data_ptr())
        # the shard as the engine builds it: the split of its rows of E, the time block and the one-hot plane of its publish times
        _lib.check(lib.tcar_split_bf16(C.c_void_p(self.E.data_ptr() + 4 * n0 * EK), EK, nl, EK, vp(self.eh), vp(self.el), EK, None, None, 0, 0, 0,
                                       None), "split")
        tmw = self.mw if time_mw is None else torch.from_numpy(np.ascontiguousarray(time_mw[n0:n0 + nl]).reshape(-1).copy()).to(dev)
        _lib.check(lib.tcar_cand_time_fwd_bf16(C.byref(loc), C.byref(tt), vp(tmw), None, vp(self.eh), vp(self.el), None), "cand_time_fwd")
        _lib.check(lib.tcar_time_onehot(C.byref(loc), vp(self.mw), vp(self.oh), 160, None), "onehot")
        torch.cuda.synchronize()

    def ctx(self):
        c = _lib.Ctx()
        c.d, c.scoring = self.dims, 3
        c.E, c.W, c.Mi, c.Vi, c.mwdhm, c.e16h, c.e16l = (t.data_ptr() for t in (self.E, self.W, self.Mi, self.Vi, self.mw, self.eh, self.el))
        for k in range(5):
            c.off[1 + k] = int(self.off[k])              # TCAR_V_MONTH = 1
        return c


def _update_owned(lib, raw, pay, refresh, mw_all=True):
    d = _lib.CatalogUpdate()
    d.U, d.ids = int(pay["ids"].numel()), pay["ids"].data_ptr()
    d.item, d.ld_item, d.zero_moments = pay["item"].data_ptr(), pay["ld"], 1
    d.content, d.ld_content = pay["content"].data_ptr(), pay["ld"]
    d.mwdhm, d.onehot, d.onehot_inner = pay["mw"].data_ptr(), raw.oh.data_ptr(), 160
    d.refresh_time = refresh
    d.key, d.key_table = pay["keys"].data_ptr(), raw.keys.data_ptr()
    d.cat, d.cat_table = pay["cat"].data_ptr(), raw.cat.data_ptr()
    _lib.check(lib.tcar_catalog_update_owned(C.byref(raw.ctx()), C.byref(d), raw.n0, raw.nl, C.c_void_p(raw.mw_all.data_ptr()) if mw_all else None,
                                             None), "tcar_catalog_update_owned")
    torch.cuda.synchronize()


def _same_shard(got, want, what, skip=()):
    for name in got.whole:
        if name in skip:
            continue
        g, w = got.whole[name], want.whole[name]
        assert torch.equal(_bytes(g), _bytes(w)), "%s: %s differs in %d words" % (what, name, int((g != w).sum()))
        assert bool((g[-CANARY:] == 0x5A5A5A5A).all()), (what, name, "canary")
    assert not bool(got.E.view(NPAD, EK)[N:].any()), (what, "padding rows of E")
    pad = got.nl % 128
    if pad:                           # the rows [nl, nlpad) of the shard's last 128-row block
        for p in (got.eh, got.el):
            assert not bool(p.view(got.nlpad // 128, EK // 32, 128, 32)[-1, :, pad:, :].view(torch.int16).any()), (what, "padding rows of the planes")
        assert not bool(got.oh.view(got.nlpad // 128, 5, 128, 32)[-1, :, pad:, :].view(torch.int16).any()), (what, "padding rows of the one-hot plane")


@pytest.mark.parametrize("refresh", [0, 1])
@pytest.mark.parametrize("name", list(ID_SETS))
@pytest.mark.parametrize("W, rank", [(w, r) for w in (2, 3) for r in range(w)])
def test_a_shard_holds_the_bytes_of_buffers_built_from_the_final_tables(lib, W, rank, name, refresh):
    t, ids = tables(), ID_SETS[name]
    n0, nl = SHARDS[W][rank]
    mom = _moments()
    got = ShardRaw(lib, n0, nl, t["params"]["item_emb"][1:], t["content"][1:], t["mw"], t["keys"], t["cat"], moments=mom)
    _update_owned(lib, got, _device_payload(ids), refresh)
    params, content, mw, keys, cat = final_tables(ids, "mw_wild")
    m, v = mom[0].copy(), mom[1].copy()
    m[ids], v[ids] = 0, 0
    # refresh_time = 0: the time block keeps the OLD publish times (the caller owes a whole refresh), everything else is final
    want = ShardRaw(lib, n0, nl, params["item_emb"][1:], content[1:], mw, keys, cat, time_mw=None if refresh else t["mw"], moments=(m, v))
    _same_shard(got, want, "W=%d rank=%d %s refresh=%d" % (W, rank, name, refresh))


@pytest.mark.parametrize("refresh", [0, 1])
@pytest.mark.parametrize("name", ["scattered", "all-reversed"])
def test_the_owner_of_every_row_leaves_the_bytes_of_the_whole_catalog_call(lib, name, refresh):
    t, ids = tables(), ID_SETS[name]
    mom = _moments()
    args = (t["params"]["item_emb"][1:], t["content"][1:], t["mw"], t["keys"], t["cat"])
    got = ShardRaw(lib, 0, N, *args, moments=mom)
    _update_owned(lib, got, _device_payload(ids), refresh)
    want = Raw(lib, True, *args, moments=mom)
    _update_whole(lib, want, _device_payload(ids), refresh)
    for n in want.whole:
        assert torch.equal(_bytes(got.whole[n]), _bytes(want.whole[n])), (name, refresh, n)
    assert torch.equal(got.mw_all, got.mw) and bool((got.whole["mw_all"][-CANARY:] == 0x5A5A5A5A).all())
    # without a whole publish-time table the call writes none: the rest is the same
    bare = ShardRaw(lib, 0, N, *args, moments=mom)
    _update_owned(lib, bare, _device_payload(ids), refresh, mw_all=False)
    _same_shard(bare, got, "no mwdhm_all", skip=("mw_all",))
    assert torch.equal(bare.mw_all.cpu(), torch.from_numpy(t["mw"].reshape(-1)))


def test_ids_outside_the_catalog_and_rows_of_other_ranks_write_nothing_here(lib):
    t = tables()
    n0, nl = SHARDS[3][1]
    args = (t["params"]["item_emb"][1:], t["content"][1:], t["mw"], t["keys"], t["cat"])
    old = lambda: ShardRaw(lib, n0, nl, *args, moments=_moments())
    got = old()
    pay = _device_payload([1, 2, 3])
    _update_owned(lib, got, dict(pay, ids=torch.tensor([N, -1, 2 ** 31 - 1], dtype=torch.int32, device="cuda:0")), 1)
    _same_shard(got, old(), "ids outside the catalog")
    # rows 0 and N - 1 belong to ranks 0 and 2: every shard-local buffer of rank 1 keeps every byte
    ids = [0, N - 1]
    _update_owned(lib, got, _device_payload(ids), 1)
    for n in ("eh", "el", "mw", "Mi", "Vi", "oh"):
        assert torch.equal(_bytes(got.whole[n]), _bytes(old().whole[n])), n
    params, content, mw, keys, cat = final_tables(ids, "mw_wild")
    _same_shard(got, ShardRaw(lib, n0, nl, params["item_emb"][1:], content[1:], mw, keys, cat, moments=_moments()), "rows of other ranks")


# ------------------------------------------------------------------------ 2  updated engines against rebuilt ones
_STATE = {}


def trained(scoring):
    """the exported state after two training steps of a one-rank sharded engine over the OLD tables: computed once, never written"""
    if scoring not in _STATE:
        from tcar_amd.sharded import ShardedEngine
        t = tables()
        eng = ShardedEngine(t["params"], t["content"], t["mw"], max_grad=2.0, scoring=scoring, world=1, rank=0)
        for _ in range(2):
            eng.train_step(t["batch"])
        _STATE[scoring] = eng.export_state()
        for a in _STATE[scoring].values():
            a.setflags(write=False)
    return _STATE[scoring]


def _engines(W, params, content, mw, keys, cat, scoring, state=None, max_grad=2.0):
    from tcar_amd.sharded import ShardedEngine
    out = []
    for rank in range(W):
        e = ShardedEngine(params, content, mw, max_grad=max_grad, scoring=scoring, world=W, rank=rank)
        assert (e.n0, e.nl) == SHARDS[W][rank] and not e.xch.collective
        if state is not None:
            e.load_state(state)
        e.set_item_keys(keys)
        e.set_categories(cat)
        out.append(e)
    return out


def _recommend(engs, W, **kw):
    subs, edges, cap = _split(R.unlabelled(tables()["batch"]), W)
    _, _, outs = play([e.serve_pieces(s, TOPK, False, exclude_seen=True, panel=PANEL, cap=cap, T=T, **kw) for e, s in zip(engs, subs)])
    tk = [o[1].cpu().numpy().copy() for o in outs]
    return [(i, np.where(i >= 0, o[3].cpu().numpy(), 0)) for i, o in zip(tk, outs)]       # (an empty slot's score is whatever was there)


def _update(engs, ids, **kw):
    new, i = tables()["new"], np.asarray(ids)
    for e in engs:
        e.shard_update_items(ids, content=new["content"][i], item_rows=new["item"][i], mwdhm=new["mw"][i], keys=new["keys"][i],
                             categories=new["cat"][i], **kw)


def _final_state(state, ids):
    """the state an engine built from the final tables resumes from: the new item rows, no optimizer history of theirs"""
    new, i = tables()["new"], np.asarray(ids)
    st = {k: np.array(v) for k, v in state.items()}
    st["var/item_emb"][1 + i] = new["item"][i]
    st["m/item_emb"][1 + i], st["v/item_emb"][1 + i] = 0, 0
    return st


def _calls(engs, W):
    """every serving call of the sharded engine, the collectives played by hand -> {name: [numpy arrays, rank after rank]}: what the
    calls return for the live sessions (the rows of padding sessions and the slots behind a short list hold whatever the workspace
    held, which follows the engine's history) and the gathered states of the live sessions"""
    batch = tables()["batch"]
    subs, edges, cap = _split(batch, W)
    fsubs, _, _ = _split(R.unlabelled(batch), W)
    sizes = SPLITS[W][0]
    live = torch.tensor(np.concatenate([r * cap + np.arange(n) for r, n in enumerate(sizes)]), device="cuda:0")
    np1 = lambda x: x.cpu().numpy().copy()

    def lists(ids, *scores):                   # the ids and, where a slot is taken, its scores
        ids = np1(ids)
        return [ids] + [np.where(ids >= 0, np1(sc), 0) for sc in scores]
    out = {}
    _, states, outs = play([e.serve_pieces(s, TOPK, True, panel=PANEL, cap=cap, T=T) for e, s in zip(engs, subs)])
    out["streamed"] = [np1(states[:, live])] + [x for o in outs for x in [np1(o[0]), np1(o[2])] + lists(o[1], o[3])]
    for tag, kw in (("window + cap", dict(window=WINDOW, max_per_category=2)), ("plain", {})):
        _, states, outs = play([e.serve_pieces(s, TOPK, False, exclude_seen=True, panel=PANEL, cap=cap, T=T, **kw) for e, s in zip(engs, fsubs)])
        out["recommend " + tag] = [np1(states[:, live])] + [x for o in outs for x in lists(o[1], o[3])]
    states, short, _, _ = play_retrieve([e.retrieve_pieces(s, SHORT, None, panel=PANEL, cap=cap, T=T) for e, s in zip(engs, fsubs)], False)
    out["retrieve"] = [np1(states[:, live])] + [x for (i, c), n in zip(short, sizes) for x in lists(i[:n], c[:n])]
    states, short, parts, outs = play_retrieve([e.retrieve_pieces(s, SHORT, TOPK, panel=PANEL, window=WINDOW, cap=cap, T=T)
                                                for e, s in zip(engs, fsubs)], True)
    out["two-stage"] = [np1(states[:, live])] + [x for (i, c), o, n in zip(short, outs, sizes)
                                                 for x in lists(i[:n], c[:n], o[2][:n]) + lists(o[0][:n], o[1][:n])]
    rng = np.random.RandomState(5)
    cand = np.concatenate([np.tile(np.asarray(ENGINE_IDS[:20], np.int32), (B, 1)), rng.randint(0, N, (B, 20)).astype(np.int32)], 1)
    lsts, parts, outs = play_candidates([e.cand_pieces(s, None if s is None else cand[edges[r]:edges[r + 1]], None, cap, T, 40)
                                         for r, (e, s) in enumerate(zip(engs, fsubs))])
    out["candidates"] = [np1(lsts[live])] + [np1(x) for o in outs for x in o if x is not None]
    out["eval_step"] = [x for e, s in zip(engs, subs) if s is not None for x in _np(*e.eval_step(s))]
    return out


def _same_calls(a, b, what):
    assert list(a) == list(b)
    for name in a:
        assert len(a[name]) == len(b[name]), (what, name)
        for i, (x, y) in enumerate(zip(a[name], b[name])):
            assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, name, i)


BUFFERS = ("E", "e16h", "e16l", "Mi", "Vi", "mwdhm", "_item_keys", "_cat", "_ev_mw", "inv_n", "inv_off", "et_perm")
INDEX = BUFFERS[-3:]


def _prepared(scoring, W, state, max_grad=2.0):
    """W engines over the OLD tables in `state` and the state they carry (None: none)"""
    t = tables()
    st = None if state == "fresh" else trained(scoring)
    engs = _engines(W, t["params"], t["content"], t["mw"], t["keys"], t["cat"], scoring, st, max_grad)
    if state != "fresh":
        for e in engs:
            e._ensure_work(SPLITS[W][1], T)
            e._ensure_score(SPLITS[W][1], R.NEG)                     # the scoring family of the training step: the shard's one-hot plane exists
            assert e._time_dirty and (getattr(e, "s_oh16", None) is not None) == e.onehot
    if state == "clean":
        _recommend(engs, W)
        assert not any(e._time_dirty for e in engs)
    return engs, st


@pytest.mark.parametrize("state", ["fresh", "dirty", "clean"])
@pytest.mark.parametrize("W", [1, 2, 3])
@pytest.mark.parametrize("scoring", ["bf16x3-mixed", "bf16x3"])
def test_updated_shards_are_the_shards_built_from_the_final_tables(scoring, W, state):
    _need_gpu()
    t, ids = tables(), ENGINE_IDS
    what = "%s, W = %d, %s" % (scoring, W, state)
    engs, st = _prepared(scoring, W, state)
    if state != "fresh":
        engs[0].eval_step(_split(t["batch"], W)[0][0])     # the whole publish-time table of eval_step exists on rank 0: it must follow
        if state == "clean":
            _recommend(engs, W)
    dirty = [e._time_dirty for e in engs]
    caller_mw = t["mw"].copy()
    _update(engs, ids)
    assert [e._time_dirty for e in engs] == dirty and (t["mw"] == caller_mw).all()          # (the caller's table is not written)
    for e in engs:                                          # every shard owns some of ENGINE_IDS, and their publish times changed
        assert e._index_stale and e._mwdhm_host.tobytes() == final_tables(ids)[2][e.n0:e.n0 + e.nl].tobytes()
        assert e._mwdhm_full.tobytes() == final_tables(ids)[2].tobytes()
    if W == 1 and st is not None:                          # the state the updated engine exports IS the final state
        st2, want = engs[0].export_state(), _final_state(st, ids)
        assert sorted(st2) == sorted(want) and all(np.asarray(st2[k]).tobytes() == np.asarray(want[k]).tobytes() for k in want), what
    rebuilt = _rebuilt(engs, st, scoring, W, ids)
    if state != "fresh":
        for e in rebuilt:
            e._ensure_work(SPLITS[W][1], T)
            e._ensure_score(SPLITS[W][1], R.NEG)
    got, want = _calls(engs, W), _calls(rebuilt, W)
    _same_calls(got, want, what)
    if state == "clean":                                    # a clean time block stayed clean: no whole refresh ran, and the lists are right
        assert not any(dirty) and not any(e._time_dirty for e in engs)
    for r, (e, e2) in enumerate(zip(engs, rebuilt)):
        e._build_time_index()                               # (what the next training step does first: the index is stale)
        for name in BUFFERS + (("s_oh16",) if state != "fresh" and e.onehot else ()):
            a, b = getattr(e, name, None), getattr(e2, name, None)
            assert (a is None) == (b is None), (what, r, name)
            if a is not None:
                assert a.shape == b.shape and torch.equal(_bytes(a), _bytes(b)), (what, r, name)
        assert e._content.tobytes() == e2._content.tobytes() and e._mwdhm_host.tobytes() == e2._mwdhm_host.tobytes()
    for e in engs + rebuilt:
        e.check_forks()


def _rebuilt(engs, st, scoring, W, ids, max_grad=2.0):
    """W engines from the final host tables and the final state (at one rank: the state the updated engine exports)"""
    params, content, mw, keys, cat = final_tables(ids)
    st2 = None if st is None else engs[0].export_state() if W == 1 else _final_state(st, ids)
    p2 = params if st2 is None else {k[4:]: v for k, v in st2.items() if k.startswith("var/")}
    return _engines(W, p2, content, mw, keys, cat, scoring, st2, max_grad)


def _one_session():
    """The batch of the compared training step: ONE session whose five clicks name five different items and five different rows of
    every small table, its click time rows no publish field names, label and negatives outside the session.  The sharded step adds
    the session-side gradients of the item rows, of dec_pos and of the small tables with float atomics, beside the candidate-side time
    backward that adds into the same table rows (tests/test_gpu_sharded.py: "two runs agree to rounding noise only").  Here every
    such destination receives at most one session-side term and one candidate-side term, and a sum of two terms has no order — the
    remedy tests/test_gpu_catalog_update.py takes for its fp32 step.  The squared norms of those gradients are atomic sums of one
    piece per row as well, five pieces here: they matter to the bits only where a variable is CLIPPED (clip / max(norm, clip) is
    exactly 1 below the clip), which the trained dec_pos is at max_grad = 2 — so the two engines of the step clip nothing
    (max_grad=None), and no order-dependent sum reaches the state.  The step still reads every catalog row: the softmax runs over all
    N, so the candidate-time backward walks the whole rebuilt index, and Adam updates the moments of every item row.
    Measured with three repetitions each on an MI355X: with this session the updated engine, the rebuilt one and a second rebuilt one
    export the same bits every time on their own, but at max_grad = 2 dec_pos and its moments differed in the trained states when
    the whole suite ran in front (the five-piece norm); with the eight sessions of tables() two engines built from IDENTICAL inputs
    differ in 17 - 24 arrays (item_emb, dec_pos, the six small tables and their moments) by up to 7.4e-07 of the largest element,
    with the first two sessions or two sessions of distinct rows in 0 - 8 arrays from run to run."""
    live = N - SPARE
    rng = np.random.RandomState(77)
    seq = rng.permutation(np.arange(1, live + 1))[:T]
    rest = rng.permutation(np.setdiff1d(np.arange(live), seq - 1))
    rows = lambda lo, hi: rng.permutation(np.arange(lo, hi))[:T]
    b = dict(seq=seq, pm=rows(1, 13), pd=rows(1, 32), pw=rows(1, 6), ph=rows(1, 20), pmi=rows(1, 61), gap=rows(0, 12))
    b = {k: v.reshape(1, T).astype(np.int32) for k, v in b.items()}
    b.update(label=rest[:1].astype(np.int32), neg=rest[1:1 + R.NEG].reshape(1, R.NEG).astype(np.int32),
             cw=np.array([6], np.int32), ch=np.array([22], np.int32))
    assert all(len(set(v.reshape(-1).tolist())) == v.size for v in b.values())
    return b


@pytest.mark.parametrize("state", ["fresh", "dirty", "clean"])
def test_one_training_step_at_one_rank_leaves_the_exported_state_of_the_rebuilt_engine(state):
    """One training step in the updated engine and in the engine rebuilt from the final tables, then the loss, the rebuilt index and
    the whole exported state, bit for bit: the rebuilt index, the one-hot rows and the zeroed moments all feed it.  The step takes
    the one session of _one_session(), whose result the sharded step defines to the bit."""
    _need_gpu()
    ids, scoring, W = ENGINE_IDS, "bf16x3-mixed", 1
    what = "%s, W = 1, %s" % (scoring, state)
    engs, st = _prepared(scoring, W, state, max_grad=None)
    _update(engs, ids)
    (e,), (e2,) = engs, _rebuilt(engs, st, scoring, W, ids, max_grad=None)
    assert e._index_stale
    batch = _one_session()
    l1, l2 = (_np(x.train_step(batch))[0] for x in (e, e2))
    assert l1.tobytes() == l2.tobytes(), (what, "loss")
    assert not e._index_stale and all(torch.equal(getattr(e, n), getattr(e2, n)) for n in INDEX), (what, "the rebuilt index")
    s1, s2 = e.export_state(), e2.export_state()
    differ = [k for k in s1 if np.asarray(s1[k]).tobytes() != np.asarray(s2[k]).tobytes()]
    print(what, "state arrays that differ:", differ)
    assert sorted(s1) == sorted(s2) and not differ, (what, differ)
    e.check_forks()
    e2.check_forks()


def test_a_shard_whose_rows_are_not_named_keeps_its_index_and_a_stale_engine_disagrees():
    """the ids of ONE shard: the other rank's index stays fresh; and the lists of an updated clean engine are those of the final
    publish times, which an engine that kept the old ones does not give (no whole refresh follows, and none is needed)"""
    _need_gpu()
    t, ids, scoring, W = tables(), ID_SETS["one-shard"], "bf16x3-mixed", 2
    engs, st = _prepared(scoring, W, "clean")
    _update(engs, ids, verify=False)
    assert engs[0]._index_stale and not engs[1]._index_stale and not any(e._time_dirty for e in engs)
    got = _recommend(engs, W)
    assert not any(e._time_dirty for e in engs)
    params, content, mw, keys, cat = final_tables(ids)
    st2 = _final_state(st, ids)
    p2 = {k[4:]: v for k, v in st2.items() if k.startswith("var/")}
    want = _recommend(_engines(W, p2, content, mw, keys, cat, scoring, st2), W)
    stale = _recommend(_engines(W, p2, content, t["mw"], keys, cat, scoring, st2), W)
    for g, w in zip(got, want):
        assert g[0].tobytes() == w[0].tobytes() and g[1].tobytes() == w[1].tobytes()
    assert any(g[1].tobytes() != s[1].tobytes() for g, s in zip(got, stale))
    # a second update of the same rows with the same publish times changes none: the index is not marked again
    engs[0]._build_time_index()
    _update(engs, ids, verify=False)
    assert not engs[0]._index_stale


# ------------------------------------------------------------------- 3  independent of the code under test
@pytest.mark.parametrize("W", [2, 3])
@pytest.mark.parametrize("scoring", ["bf16x3-mixed", "bf16x3"])
def test_the_updated_rows_score_as_an_fp64_dot_of_the_final_tables(scoring, W):
    _need_gpu()
    from oracle.tcar_oracle import TcarOracle
    t, ids = tables(), ENGINE_IDS
    engs, _ = _prepared(scoring, W, "fresh")
    _update(engs, ids)
    fsubs, edges, cap = _split(R.unlabelled(t["batch"]), W)
    cand = np.tile(np.asarray(ids, np.int32), (B, 1))
    _, _, outs = play_candidates([e.cand_pieces(s, None if s is None else cand[edges[r]:edges[r + 1]], None, cap, T, len(ids))
                                  for r, (e, s) in enumerate(zip(engs, fsubs))])
    scores, rank_of, order = (np.concatenate([o[i].cpu().numpy() for o in outs]) for i in range(3))
    assert scores.shape == cand.shape

    def ref(params, content, mw, name):
        r = R._forward(TcarOracle(params, content, mw), t["batch"])
        s = r["A"] @ r["E"].T                                                  # the fp64 numpy dot
        assert np.abs(s - r["s"]).max() <= 1e-9 * np.abs(r["s"]).max()
        return dict(s=s, delta=1e-3 * np.abs(s).max(1), name=name)
    params, content, mw, _, _ = final_tables(ids)
    final, old = ref(params, content, mw, "final tables, shards"), ref(t["params"], t["content"], t["mw"], "old tables, shards")
    R.check_candidates(final, cand, scores, rank_of, order, name="updated rows, %s, W = %d" % (scoring, W))
    print({k: round(v, 4) for k, v in R.WORST.items() if k.startswith("final tables, shards")})
    # the rows moved by far more than the gate: the same scores are refused over the tables they replaced
    assert np.abs(final["s"][:, ids] - old["s"][:, ids]).max() > 100 * final["delta"].max()
    with pytest.raises(AssertionError):
        R.check_candidates(old, cand, scores, rank_of, order, name="updated rows against the OLD tables")


# ---------------------------------------------------------------------------------- 4  the publishing idiom
@pytest.mark.parametrize("W", [2, 3])
def test_spare_rows_of_the_last_shard_reach_the_lists_of_every_rank_and_are_retired_again(W):
    _need_gpu()
    from oracle.tcar_oracle import TcarOracle
    t, scoring = tables(), "bf16x3-mixed"
    batch = t["batch"]
    window, spare = (0, 10 ** 6), np.arange(N - SPARE, N)
    assert spare[0] >= SHARDS[W][-1][0]                            # every spare row lives in the last shard
    engs, _ = _prepared(scoring, W, "fresh")
    sizes = SPLITS[W][0]
    listed = lambda es=None: np.concatenate([o[0] for o, n in zip(_recommend(es or engs, W, window=window), sizes) if n])
    assert not np.isin(listed(), spare).any()                     # a spare row is in no pool
    r = R._forward(TcarOracle(t["params"], t["content"], t["mw"]), batch)
    s = r["s"].copy()
    s[:, spare] = -np.inf
    s[np.arange(B)[:, None], batch["seq"] - 1] = -np.inf           # exclude_seen
    top1 = s.argmax(1)
    part = np.einsum("bk,bk->b", r["A"][:, :2 * H], r["E"][top1][:, :2 * H])
    assert (part > 20 * 1e-3 * np.abs(r["s"]).max(1)).all()        # (clear of the logits gate: the engines cannot order them otherwise)
    pub, src, params = spare[:10], top1[np.arange(10) % B], t["params"]
    for e in engs:
        e.shard_update_items(pub, content=1.5 * t["content"][1 + src], item_rows=1.5 * params["item_emb"][1 + src], mwdhm=t["mw"][src],
                             keys=np.full(10, 500000), categories=t["cat"][src])
    now = listed()
    assert now.shape == (B, TOPK)
    for j, row in enumerate(pub):                                  # published: in the list of a session of whichever rank holds it
        assert row in now[j % B], (j, row, now[j % B])
    assert not np.isin(now, spare[10:]).any()
    for e in engs:
        e.shard_update_items(pub, keys=np.full(10, FAR))           # retired: the key moves out of every window
    assert not np.isin(listed(), spare).any()
    # and the engines are those built from the final tables
    p2 = {k: v.copy() for k, v in params.items()}
    content, mw, cat = t["content"].copy(), t["mw"].copy(), t["cat"].copy()
    p2["item_emb"][1 + pub] = 1.5 * params["item_emb"][1 + src]
    content[1 + pub], mw[pub], cat[pub] = 1.5 * t["content"][1 + src], t["mw"][src], t["cat"][src]
    fresh = _engines(W, p2, content, mw, t["keys"], cat, scoring)
    for kw in (dict(window=window), dict(), dict(window=window, max_per_category=2)):
        for a, b in zip(_recommend(engs, W, **kw), _recommend(fresh, W, **kw)):
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), kw


# ------------------------------------------------------------------------------------------- 5  the replicas
@pytest.mark.parametrize("scoring", ["f32", "bf16x3-mixed"])
def test_a_replica_without_a_group_gives_the_bits_of_update_items(scoring):
    _need_gpu()
    from tcar_amd.dp import DPEngine
    from tcar_amd.engine import TcarEngine
    t, ids = tables(), np.asarray(ENGINE_IDS)
    new, feed = t["new"], R.unlabelled(t["batch"])
    kw = dict(content=new["content"][ids], item_rows=new["item"][ids], mwdhm=new["mw"][ids], keys=new["keys"][ids], categories=new["cat"][ids])
    res = []
    for call in (DPEngine.replica_update_items, TcarEngine.update_items):
        eng = DPEngine(t["params"], t["content"], t["mw"], max_grad=2.0, scoring=scoring)
        assert not eng.xch.collective
        eng.set_item_keys(t["keys"])
        eng.set_categories(t["cat"])
        eng.Mi.fill_(0.25)                                              # an optimizer history the replaced rows must lose
        eng.Vi.fill_(0.5)
        eng.recommend(feed)                                             # a clean time block
        call(eng, ids, **kw)
        assert not eng._time_dirty and eng._index_stale
        res.append((_np(*eng.recommend(feed, window=WINDOW, max_per_category=2)), eng.export_state()))
    (r1, s1), (r2, s2) = res
    assert all(a.tobytes() == b.tobytes() for a, b in zip(r1, r2))
    assert sorted(s1) == sorted(s2) and not [k for k in s1 if np.asarray(s1[k]).tobytes() != np.asarray(s2[k]).tobytes()]
    with pytest.raises(_lib.TcarError):
        DPEngine.update_items(eng, ids, **kw)


# ------------------------------------------------------------------------------------- 6  two ranks over gloo
def _worker(rank, world, port, ret, scoring):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import tcar_amd  # noqa: F401
        from tcar_amd.sharded import ShardedEngine
        t, ids = tables(), np.asarray(ENGINE_IDS)
        new = t["new"]
        eng = ShardedEngine(t["params"], t["content"], t["mw"], max_grad=2.0, group=dist.group.WORLD, scoring=scoring)
        eng.set_item_keys(t["keys"])
        eng.set_categories(t["cat"])
        names = ("E", "e16h", "e16l", "Mi", "Vi", "mwdhm", "_item_keys", "_cat")
        snap = lambda: [getattr(eng, n).clone() for n in names]
        before = snap()
        kw = dict(content=new["content"][ids], item_rows=new["item"][ids], mwdhm=new["mw"][ids], keys=new["keys"][ids], categories=new["cat"][ids])
        # a request that differs in ONE element on rank 1: refused on BOTH ranks, every catalog buffer as it was
        bad = dict(kw, content=kw["content"].copy())
        if rank == 1:
            bad["content"][17, 3] += 1
        try:
            eng.shard_update_items(ids, **bad)
            raise AssertionError("rank %d: the ranks agreed on different requests" % rank)
        except _lib.TcarError as e:
            assert "rank 1 differs from rank 0's" in str(e), str(e)
        torch.cuda.synchronize()
        assert all(torch.equal(_bytes(a), _bytes(b)) for a, b in zip(before, snap())) and not eng._index_stale
        assert eng._content.tobytes() == t["content"].tobytes() and eng._mwdhm_full.tobytes() == t["mw"].tobytes()
        assert eng.xch.order.count("update_digest") == 1 and eng.xch.bytes_moved["update_digest"] == world * 16
        eng.shard_update_items(ids, **kw)                        # verify=True: the ranks agree
        assert eng.xch.order.count("update_digest") == 2
        subs, edges, cap = _split(R.unlabelled(t["batch"]), world)
        tk, sc = eng.recommend(subs[rank], k=TOPK, panel=PANEL, window=WINDOW, max_per_category=2, cap=cap, T=T)
        torch.cuda.synchronize()
        tk = tk.cpu().numpy()
        ret[rank] = {"topk": tk.tobytes(), "scores": np.where(tk >= 0, sc.cpu().numpy(), 0).tobytes(),
                     "buffers": [_bytes(getattr(eng, n)).cpu().numpy().tobytes() for n in names]}
        eng.close()
    except Exception as e:
        import traceback
        ret[rank] = "FAIL: " + repr(e) + "\n" + traceback.format_exc()
    finally:
        dist.destroy_process_group()


def test_two_ranks_over_gloo_agree_and_give_the_bits_of_the_two_engines_in_one_process():
    _need_gpu()
    scoring, world = "bf16x3-mixed", 2
    ret = launch(_worker, world, scoring, spawned_manager=True)
    for rk in range(world):
        assert isinstance(ret.get(rk), dict), ret.get(rk)
    engs, _ = _prepared(scoring, world, "fresh")
    _update(engs, ENGINE_IDS)
    outs = _recommend(engs, world, window=WINDOW, max_per_category=2)
    torch.cuda.synchronize()
    for rk, e in enumerate(engs):
        got = ret[rk]
        assert got["topk"] == outs[rk][0].tobytes() and got["scores"] == outs[rk][1].tobytes(), rk
        for n, b in zip(("E", "e16h", "e16l", "Mi", "Vi", "mwdhm", "_item_keys", "_cat"), got["buffers"]):
            assert b == _bytes(getattr(e, n)).cpu().numpy().tobytes(), (rk, n)
