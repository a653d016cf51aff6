"""Host side of in-place catalog updates (include/tcar_catalog.h): the bindings generated from the header, the argument checks that
answer before anything is launched, the engine's request validation on an engine that was never built, the engines that refuse, and
Seq2SeqAttNN.update_articles over an engine that only records — none of it needs a GPU."""
import ctypes as C
import datetime
import os
import subprocess
import types

import numpy as np
import pytest

import tcar_amd  # noqa: F401
from tcar_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["U", "ids", "item", "ld_item", "content", "ld_content", "mwdhm", "refresh_time", "key", "key_table", "cat", "cat_table",
          "zero_moments", "onehot", "onehot_inner"]


def test_the_catalog_layer_is_bound_and_the_other_layers_are_where_they_were():
    lib = _lib.load()
    assert _lib.CATALOG_SYMBOLS == ["tcar_catalog_abi_version", "tcar_catalog_update"]
    assert lib.tcar_catalog_abi_version() == _lib.CATALOG_ABI_VERSION == 1
    assert ("CATALOG", "tcar_catalog.h") in _lib.ABI_LAYERS and _lib.CATALOG_HEADER in _lib.HEADERS and "catalog.hip" in _lib.SOURCES
    assert _lib.ABI_LAYERS[0] == ("", "tcar_hip.h") and _lib.ABI_LAYERS[-1] == ("RAGGED", "tcar_ragged.h")
    assert _lib.ABI_VERSION == 30 and len(_lib.SYMBOLS) == 112 and len(_lib.Ctx._fields_) == 104
    for prefix, _ in _lib.ABI_LAYERS:
        if prefix != "CATALOG":
            assert not set(_lib.CATALOG_SYMBOLS) & set(getattr(_lib, _lib._name(prefix, "SYMBOLS"))), prefix
    assert lib.tcar_catalog_update.argtypes == [C.POINTER(_lib.Ctx), C.POINTER(_lib.CatalogUpdate), C.c_void_p]
    assert lib.tcar_catalog_update.restype is C.c_int32


def test_the_mirror_has_the_layout_the_compiler_gives_the_header(tmp_path):
    m = _lib.CatalogUpdate
    assert [f[0] for f in m._fields_] == FIELDS
    t = "tcar_catalog_update_t"
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "tcar_catalog.h"', 'int main() {', '  printf("%%zu\\n", sizeof(%s));' % t]
    lines += ['  printf("%%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (t, f, t, f) for f in FIELDS]
    lines.append('  return 0;\n}')
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([_lib._hipcc(), "-x", "c++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = iter(subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE).stdout.decode().split("\n"))
    assert int(next(got)) == C.sizeof(m)
    for f in FIELDS:
        d = getattr(m, f)
        assert next(got).split() == [str(d.offset), str(d.size)], f


def _context(p, scoring=0):
    """a context whose catalog side looks complete (host memory, never dereferenced: an accepted call would have to launch)"""
    c = _lib.Ctx()
    c.d = _lib.Dims(700, 250, 64, 256, 64)
    c.scoring = scoring
    c.E = c.W = c.Mi = c.Vi = c.mwdhm = c.e16h = c.e16l = p.value
    return c


def test_argument_errors_come_back_before_any_launch():
    lib = _lib.load()
    buf = (C.c_float * 4096)()
    p = C.cast(buf, C.c_void_p)
    good = dict(U=3, ids=p.value, item=p.value, ld_item=252, content=p.value, ld_content=256, mwdhm=p.value, refresh_time=1, key=p.value,
                key_table=p.value, cat=p.value, cat_table=p.value, zero_moments=1, onehot=p.value, onehot_inner=160)
    bad = [dict(U=-1), dict(ids=None),
           dict(item=None, content=None, mwdhm=None, key=None, key_table=None, cat=None, cat_table=None),      # no table
           dict(ld_item=248), dict(ld_item=250), dict(ld_item=254), dict(ld_content=249), dict(ld_content=0),       # ld < H, ld % 4
           dict(item=p.value + 4), dict(content=p.value + 8),                                                      # 16-byte alignment
           dict(key_table=None), dict(key=None), dict(cat_table=None), dict(cat=None),                             # both or neither
           dict(onehot_inner=128), dict(onehot_inner=170), dict(onehot_inner=0)]

    def call(ctx, **kw):
        d = _lib.CatalogUpdate()
        for f, v in dict(good, **kw).items():
            setattr(d, f, v)
        return lib.tcar_catalog_update(C.byref(ctx) if ctx is not None else None, C.byref(d), None)

    for ctx in (_lib.Ctx(), _context(p), _context(p, scoring=3)):
        for kw in bad:
            if ctx.d.H == 0 and ("ld_item" in kw or "ld_content" in kw) and all(v % 4 == 0 for v in kw.values()):
                continue                          # (ld < H needs a context that states H)
            assert call(ctx, **kw) == -1, kw
        # U == 0: nothing to do, whatever else the descriptor says — also on an empty context
        assert call(ctx, U=0) == 0 and call(ctx, U=0, ids=None, item=None, content=None, mwdhm=None) == 0
    assert call(None) == -1 and call(None, U=0) == -1
    assert lib.tcar_catalog_update(C.byref(_context(p)), None, None) == -1
    # refresh_time with no publish times anywhere: neither in the call nor in the context
    no_mw = _context(p)
    no_mw.mwdhm = None
    assert call(no_mw, mwdhm=None, onehot=None) == -1
    # an empty context refuses a descriptor that is in order: still before any launch
    assert call(_lib.Ctx(), ld_item=256) == -1
    # what the context must carry for what the call asks
    for field, kw in (("E", {}), ("e16h", {}), ("e16l", {}), ("mwdhm", {}), ("Mi", {}), ("Vi", {}), ("W", {})):
        ctx = _context(p, scoring=3)
        setattr(ctx, field, None)
        assert call(ctx, **kw) == -1, field
    ctx = _context(p)
    ctx.d = _lib.Dims(700, 250, 64, 250, 64)           # ldh not a multiple of 64
    assert call(ctx) == -1
    ctx.d = _lib.Dims(0, 250, 64, 256, 64)
    assert call(ctx) == -1


def _unbuilt_engine():
    from tcar_amd.engine import TcarEngine
    eng = TcarEngine.__new__(TcarEngine)
    eng.shard, eng.geo = (0, 700), types.SimpleNamespace(N=700, Npad=768, H=250)
    return eng


def test_the_engine_validates_an_update_before_any_device_call():
    """TcarEngine._update_request runs before the staging copy and the launch: on an engine that was never built (no device, no
    workspace, no library handle) a refused update raises ValueError and nothing else is reached"""
    eng = _unbuilt_engine()
    row = np.zeros((2, 250), np.float32)
    mw = np.ones((2, 5), np.int32)
    no_table = "update_items needs at least one of content, item_rows, mwdhm, keys, categories"
    ids_msg = "ids must be an integer array [U] of at least one catalog row"
    refused = [(lambda: eng.update_items([], content=row[:0]), ids_msg),
               (lambda: eng.update_items(np.zeros((2, 1), np.int64), content=row), ids_msg),
               (lambda: eng.update_items([1.0, 2.0], content=row), ids_msg),
               (lambda: eng.update_items([True, False], content=row), ids_msg),
               (lambda: eng.update_items([3, 700], content=row), "ids must lie in [0, N = 700)"),
               (lambda: eng.update_items([-1, 3], content=row), "ids must lie in [0, N = 700)"),
               (lambda: eng.update_items([5, 5], content=row), "ids must be pairwise distinct"),
               (lambda: eng.update_items([5, 6]), no_table),
               (lambda: eng.update_items([5, 6], content=row[:, :249]), "content must be a float array [2, 250]"),
               (lambda: eng.update_items([5, 6], content=row[:1]), "content must be a float array [2, 250]"),
               (lambda: eng.update_items([5, 6], content=np.zeros((2, 250), object)), "content must be a float array [2, 250]"),
               (lambda: eng.update_items([5, 6], item_rows=row.reshape(-1)), "item_rows must be a float array [2, 250]"),
               (lambda: eng.update_items([5, 6], mwdhm=mw[:, :4]), "mwdhm must be an integer array [2, 5]"),
               (lambda: eng.update_items([5, 6], mwdhm=mw.astype(np.float32)), "mwdhm must be an integer array [2, 5]"),
               (lambda: eng.update_items([5, 6], keys=[1, 2, 3]), "keys must be an integer array [2]"),
               (lambda: eng.update_items([5, 6], keys=[1.5, 2.0]), "keys must be an integer array [2]"),
               (lambda: eng.update_items([5, 6], categories=[[1, 2]]), "categories must be an integer array [2]"),
               (lambda: eng.update_items([5, 6], keys=[1, 2]), "keys update the item keys: call set_item_keys(keys) first"),
               (lambda: eng.update_items([5, 6], categories=[1, 2]),
                "categories update the category table: call set_categories(cat_of_item) first")]
    for call, text in refused:
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text
    eng._item_keys = object()                      # the key table is installed: the values are looked at next
    for keys in ([0, 2 ** 31], [-2 ** 31 - 1, 0]):
        with pytest.raises(ValueError) as e:
            eng.update_items([5, 6], keys=keys)
        assert str(e.value) == "item keys must fit int32"
    got = eng._update_request(np.array([6, 5], np.int64), row.astype(np.float64), None, mw.astype(np.int64), [2 ** 31 - 2, -2 ** 31], None)
    assert [None if x is None else (x.dtype, x.shape) for x in got] == [(np.int32, (2,)), (np.float32, (2, 250)), None, (np.int32, (2, 5)),
                                                                        (np.int32, (2,)), None]
    assert got[0].tolist() == [6, 5] and got[4].tolist() == [2 ** 31 - 2, -2 ** 31]
    eng.shard = (0, 350)                           # a request in order on an engine that holds a shard
    with pytest.raises(_lib.TcarError, match="whole catalog on this engine"):
        eng.update_items([5, 6], content=row)


def test_the_sharded_and_the_replica_engines_refuse():
    from tcar_amd.dp import DPEngine
    from tcar_amd.sharded import ShardedEngine
    row = np.zeros((1, 250), np.float32)
    with pytest.raises(_lib.TcarError, match=r"update_items\(\) needs the whole catalog on one engine"):
        ShardedEngine.__new__(ShardedEngine).update_items([1], content=row)
    with pytest.raises(_lib.TcarError, match=r"update_items\(\) is not for the data-parallel replicas"):
        DPEngine.__new__(DPEngine).update_items([1], content=row)


class _Recorder:
    """an engine that only records what the model hands it"""

    def __init__(self):
        self.calls, self.keys, self.cats = [], None, None

    def set_item_keys(self, keys):
        self.keys = np.array(keys)

    def set_categories(self, cat):
        self.cats = np.array(cat)

    def update_items(self, ids, **kw):
        self.calls.append((np.asarray(ids).copy(), kw))


def _model(n=12):
    from tcar_amd.host.model import Seq2SeqAttNN
    m = Seq2SeqAttNN.__new__(Seq2SeqAttNN)
    t0 = datetime.datetime(2017, 3, 30, 22, 58)
    m.publish_time = [t0 + datetime.timedelta(minutes=17 * i) for i in range(n)]
    from tcar_amd.host.data import publish_fields
    m.publish_time_MWDHM = np.asarray([publish_fields(t) for t in m.publish_time], np.int32)
    m.candidate_n = n + 1
    m._keys = m._key_t0 = None
    m._cat = np.arange(n, dtype=np.int64) % 3
    m.engine = _Recorder()
    return m, t0


def test_update_articles_derives_the_fields_and_keys_the_loader_derives():
    from tcar_amd.host.data import SessionStore, publish_fields
    m, t0 = _model()
    when = [datetime.datetime(2017, 4, 2, 0, 0), datetime.datetime(2017, 12, 31, 23, 59), t0]
    ids = [7, 2, 11]
    content = np.arange(3 * 4, dtype=np.float32).reshape(3, 4)
    # the loader's own fields of the same datetimes: a store built from one session that clicks articles published at `when`
    times = {"s": [{"click_t": t, "publish_t": t} for t in when]}
    store = SessionStore.from_dicts({"s": [1, 2, 3]}, times)
    want_mw = np.asarray(store.pub[:3], np.int32)
    assert want_mw.tolist() == [list(publish_fields(t)) for t in when] == [[4, 2, 7, 1, 1], [12, 31, 7, 24, 60], [3, 30, 4, 23, 59]]

    # before a window was ever used there are no keys: the call brings none
    m.update_articles(ids, content=content, publish_time=when)
    got_ids, kw = m.engine.calls[-1]
    assert got_ids.tolist() == ids and kw["keys"] is None and kw["categories"] is None and kw["item_rows"] is None
    assert kw["content"] is content and np.asarray(kw["mwdhm"]).tolist() == want_mw.tolist()
    assert m.publish_time_MWDHM[ids].tolist() == want_mw.tolist() and [m.publish_time[i] for i in ids] == when
    assert m.engine.keys is None and m._keys is None

    # with the keys installed they follow, in minutes since the earliest publish time the keys were built from
    m, t0 = _model()
    base = m._item_keys().copy()
    assert m._key_t0 == np.datetime64(t0, "s") and m.engine.keys.tolist() == base.tolist() == [17 * i for i in range(12)]
    m.update_articles(ids, publish_time=when, category=[5, 6, 7])
    got_ids, kw = m.engine.calls[-1]
    want_keys = m.minute_of(when)
    assert want_keys.tolist() == [int((t - t0).total_seconds()) // 60 for t in when] and want_keys[2] == 0
    assert np.asarray(kw["keys"]).tolist() == want_keys.tolist() and np.asarray(kw["mwdhm"]).tolist() == want_mw.tolist()
    assert np.asarray(kw["categories"]).tolist() == [5, 6, 7] and kw["content"] is None
    assert m._keys[ids].tolist() == want_keys.tolist() and m._keys.dtype == np.int32
    untouched = [i for i in range(12) if i not in ids]
    assert m._keys[untouched].tolist() == base[untouched].tolist()
    # the category table on the engine is the model's own table, updated in place
    assert m._cat_on_engine is m._cat and m._cat[ids].tolist() == [5, 6, 7] and m._cat[untouched].tolist() == [i % 3 for i in untouched]
    assert m.engine.cats.tolist() == [i % 3 for i in range(12)]              # installed from the old table, then updated by the call
    assert len(m.engine.calls) == 1

    # a time before the keys' origin cannot be a key: refused, and nothing reaches the engine or the model's tables
    before = m.publish_time_MWDHM.copy()
    with pytest.raises(ValueError, match="before the earliest publish time of the item keys"):
        m.update_articles([4], publish_time=[t0 - datetime.timedelta(minutes=1)])
    assert len(m.engine.calls) == 1 and (m.publish_time_MWDHM == before).all()
