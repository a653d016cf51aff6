"""What the GPU tests of in-place catalog updates share (test_gpu_catalog_update.py, test_gpu_catalog_shard.py): the shape — N = 700
(Npad = 768, the last 128-row block holds 60 live rows), H = 250 (ldh = 256: the pad columns 250 .. 255 of both blocks are live
hazards), Ht = 64, B = 8, T = 5 —, the OLD catalog with a replacement for every row, the host tables after an update, and the catalog
side of a context built from host tables into canary-guarded raw buffers, with tcar_catalog_update run on it.  Computed once, never
written."""
import ctypes as C

import numpy as np
import torch

from tcar_amd import _lib

import serve_shapes_ref as R

N, H, HT, B, T = 700, 250, 64, 8, 5
LDH, LDT = 256, 64
EK, NPAD = 2 * LDH + 5 * LDT, 768
SPARE = 50                                   # the last rows of the catalog: no session has read them
VOCAB = (13, 32, 8, 25, 61)
CANARY = 64                                  # 4-byte words behind every raw buffer
FAR = 2 ** 31 - 2                            # a key above every window's hi

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
        # every replacement row is at distance >= 1 from the row it replaces (test 3 of both modules rests on it)
        d_content = np.linalg.norm(new["content"] - content[1:], axis=1).min()
        d_item = np.linalg.norm(new["item"] - params["item_emb"][1:], axis=1).min()
        assert d_content >= 1 and d_item >= 1, ("a replacement row within 1 of the row it replaces", d_content, d_item)
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


def _guarded(numel, dtype, dev):
    """a buffer of `numel` elements with CANARY 4-byte words behind it -> (whole allocation as int32 words, the buffer)"""
    nbytes = numel * torch.empty((), dtype=dtype).element_size()
    assert nbytes % 4 == 0, ("a buffer of whole 4-byte words", numel, dtype, nbytes)
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
