"""Host side of catalog updates on the sharded and the replica engines (include/tcar_catalog_shard.h): the bindings of the new layer
and every pinned count and position of the others, the argument checks of tcar_catalog_update_owned that answer before anything is
launched, the digest of a request, dp.Collectives.agree over gloo in two CPU processes, the order validation -> agreement -> staging
on engines that were never built, and the routing of Seq2SeqAttNN.update_articles — none of it needs a GPU."""
import ctypes as C
import datetime
import os
import sys
import types

import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401
from tcar_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dist_util import launch  # noqa: E402


def test_the_layer_is_bound_and_every_pinned_count_and_position_is_unchanged():
    lib = _lib.load()
    assert _lib.CATALOG_SHARD_SYMBOLS == ["tcar_catalog_shard_abi_version", "tcar_catalog_update_owned"]
    assert lib.tcar_catalog_shard_abi_version() == _lib.CATALOG_SHARD_ABI_VERSION == 1
    i = _lib.ABI_LAYERS.index(("CATALOG", "tcar_catalog.h"))
    assert _lib.ABI_LAYERS[i + 1] == ("CATALOG_SHARD", "tcar_catalog_shard.h")           # directly behind the layer it builds on
    assert _lib.CATALOG_SHARD_HEADER in _lib.HEADERS and "catalog.hip" in _lib.SOURCES
    # what the other layers' tests pin
    assert _lib.CATALOG_SYMBOLS == ["tcar_catalog_abi_version", "tcar_catalog_update"] and _lib.CATALOG_ABI_VERSION == 1
    assert _lib.ABI_VERSION == 30 and len(_lib.SYMBOLS) == 112
    assert len(_lib.Ctx._fields_) == 104 and len(_lib.Shard._fields_) == 25
    assert _lib.ABI_LAYERS[0] == ("", "tcar_hip.h")
    assert _lib.ABI_LAYERS[-2] == ("RETRIEVE_SHARD", "tcar_retrieve_shard.h") and _lib.ABI_LAYERS[-1] == ("RAGGED", "tcar_ragged.h")
    for prefix, _ in _lib.ABI_LAYERS:
        if prefix != "CATALOG_SHARD":
            assert not set(_lib.CATALOG_SHARD_SYMBOLS) & set(getattr(_lib, _lib._name(prefix, "SYMBOLS"))), prefix
    f = lib.tcar_catalog_update_owned
    assert f.argtypes == [C.POINTER(_lib.Ctx), C.POINTER(_lib.CatalogUpdate), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    assert f.restype is C.c_int32


def _context(p, scoring=3):
    """a plane context whose catalog side looks complete (host memory, never dereferenced: an accepted call would have to launch)"""
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

    def call(ctx, n0=0, n_loc=384, mw_all=None, **kw):
        d = _lib.CatalogUpdate()
        for f, v in dict(good, **kw).items():
            setattr(d, f, v)
        return lib.tcar_catalog_update_owned(C.byref(ctx) if ctx is not None else None, C.byref(d), n0, n_loc, mw_all, None)

    ctx = _context(p)
    # the shard: n0 < 0, n_loc <= 0, n0 + n_loc > N — with and without a whole publish-time table
    for n0, n_loc in ((-1, 384), (-128, 128), (0, 0), (384, 0), (0, -5), (384, 317), (0, 701), (700, 1), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert call(ctx, n0, n_loc) == -1 and call(ctx, n0, n_loc, p) == -1, (n0, n_loc)
    # plane contexts only
    assert call(_context(p, scoring=0)) == -1 and call(_context(p, scoring=0), 0, 700) == -1
    # the argument errors of tcar_catalog_update, on every shard shape that is in order
    bad = [dict(U=-1), dict(ids=None),
           dict(item=None, content=None, mwdhm=None, key=None, key_table=None, cat=None, cat_table=None),
           dict(ld_item=248), dict(ld_item=254), dict(ld_content=249), dict(ld_content=0),
           dict(item=p.value + 4), dict(content=p.value + 8),
           dict(key_table=None), dict(key=None), dict(cat_table=None), dict(cat=None),
           dict(onehot_inner=128), dict(onehot_inner=170), dict(onehot_inner=0)]
    for n0, n_loc in ((0, 384), (384, 316), (0, 700), (699, 1)):
        for kw in bad:
            assert call(ctx, n0, n_loc, **kw) == -1, (n0, n_loc, kw)
        for field in ("E", "e16h", "e16l", "mwdhm", "Mi", "Vi", "W"):
            c2 = _context(p)
            setattr(c2, field, None)
            assert call(c2, n0, n_loc) == -1, field
        # U == 0: nothing to do, whatever else the call says
        assert call(ctx, n0, n_loc, U=0) == 0 and call(ctx, n0, n_loc, p, U=0, ids=None, item=None, content=None, mwdhm=None) == 0
    assert call(ctx, -1, 0, U=0) == 0 and call(_lib.Ctx(), U=0) == 0
    assert call(None) == -1 and call(None, U=0) == -1
    assert lib.tcar_catalog_update_owned(C.byref(ctx), None, 0, 384, None, None) == -1
    assert call(_lib.Ctx()) == -1


# ---------------------------------------------------------------------------------------------------- the digest
def _request(seed=0, U=6):
    rng = np.random.RandomState(seed)
    return dict(ids=rng.permutation(700)[:U].astype(np.int32), content=rng.standard_normal((U, 250)).astype(np.float32),
                item_rows=rng.standard_normal((U, 250)).astype(np.float32), mwdhm=rng.randint(0, 8, (U, 5)).astype(np.int32),
                keys=rng.randint(0, 10 ** 6, U).astype(np.int32), categories=rng.randint(0, 9, U).astype(np.int32))


def _unbuilt(cls, keys=True):
    eng = cls.__new__(cls)
    eng.shard, eng.geo, eng.dev = (0, 700), types.SimpleNamespace(N=700, Npad=768, H=250), None
    if keys:
        eng._item_keys = eng._cat = object()
    return eng


def test_requests_that_validate_to_the_same_arrays_hash_equal_and_nothing_else_does():
    from tcar_amd.dp import update_digest
    from tcar_amd.engine import TcarEngine
    eng = _unbuilt(TcarEngine)
    names = ("ids", "content", "item_rows", "mwdhm", "keys", "categories")
    dig = lambda r: update_digest(*eng._update_request(*[r.get(n) for n in names]))
    r = _request()
    d0 = dig(r)
    assert isinstance(d0, bytes) and len(d0) == 16 and dig(_request()) == d0
    # the same values in other clothes: lists, int64 / float64 arrays, tensors, strided views
    wide = np.zeros((6, 500), np.float32)
    wide[:, ::2] = r["content"]
    same = [dict(r, ids=r["ids"].tolist()), dict(r, ids=r["ids"].astype(np.int64), mwdhm=r["mwdhm"].astype(np.int64)),
            dict(r, content=r["content"].astype(np.float64)), dict(r, content=torch.from_numpy(r["content"]), keys=torch.from_numpy(r["keys"])),
            dict(r, content=wide[:, ::2], categories=r["categories"].astype(np.int16)), dict(r, item_rows=np.asfortranarray(r["item_rows"]))]
    for s in same:
        assert dig(s) == d0
    # any changed element, field or order
    other = []
    for n in names:
        x = r[n].copy()
        x.reshape(-1)[-1] += 1
        other.append(dict(r, **{n: x}))
        if n != "ids":
            other.append({k: v for k, v in r.items() if k != n})                  # the field is absent
    x = r["content"].copy()
    x[2, 7] = np.nextafter(x[2, 7], np.float32(9))                                # one ulp
    other.append(dict(r, content=x))
    other.append(dict(r, content=-0.0 * r["content"]))
    other.append(dict(r, content=r["item_rows"], item_rows=r["content"]))         # two fields swapped
    other.append(dict(r, keys=r["categories"], categories=r["keys"]))
    perm = np.r_[1, 0, 2:6]
    other.append({k: v[perm] for k, v in r.items()})                               # the same rows in another order
    other.append(dict(r, ids=r["ids"][perm]))
    other.append({k: v[:5] for k, v in r.items()})                                 # U
    zero = dict(ids=np.arange(4), content=np.zeros((4, 250), np.float32))          # payloads of equal bytes under different fields
    other += [zero, dict(ids=np.arange(4), item_rows=np.zeros((4, 250), np.float32))]
    digs = [dig(o) for o in other]
    assert d0 not in digs and len(set(digs)) == len(digs)


# ---------------------------------------------------------------------------------------- agreement over gloo
def _agree_worker(rank, world, port, ret):
    import torch.distributed as dist
    for k in ("TCAR_FORCE_COLLECTIVES", "TCAR_RCCL_DIRECT", "TCAR_SIM_WORLD"):
        os.environ.pop(k, None)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    try:
        import tcar_amd  # noqa: F401
        from tcar_amd import _lib, dp
        from tcar_amd.sharded import ShardedEngine
        # without live collectives: a no-op (one rank, a sim world) — nothing is gathered, whatever the digest
        for xc in (dp.Collectives(), dp.Collectives(world=4, rank=0, sim=True)):
            xc.agree(b"x" * 16)
            xc.agree(b"")
            assert xc.order == []
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
        xc = dp.Collectives(dist.group.WORLD)
        same, mine = dp.update_digest(*[_request()[n] for n in ("ids", "content", "item_rows", "mwdhm", "keys", "categories")]), bytes([rank]) * 16
        xc.agree(same)                                           # equal digests: returns
        assert xc.order == ["update_digest"] and xc.bytes_moved["update_digest"] == world * 16
        try:
            xc.agree(mine, key="again")
            raise AssertionError("rank %d: unequal digests agreed" % rank)
        except _lib.TcarError as e:                              # on BOTH ranks, naming rank 1
            assert "rank 1 differs from rank 0's" in str(e) and "seen on rank %d" % rank in str(e), str(e)
        assert xc.order == ["update_digest", "again"]
        try:
            xc.agree(b"short")
            raise AssertionError("a digest of 5 bytes was taken")
        except ValueError:
            pass
        # an engine that was never built: a request that differs in ONE element on rank 1 raises on both ranks before the staging
        eng = _unbuilt(ShardedEngine)
        eng.xch, reached = xc, []
        eng.flush = lambda: reached.append("flush")
        eng._stage_update = lambda *a: reached.append("stage") or (_ for _ in ()).throw(RuntimeError("staged"))
        r = _request()
        if rank == 1:
            r["content"] = r["content"].copy()
            r["content"][3, 100] += 1
        try:
            eng.shard_update_items(**r)
            raise AssertionError("rank %d: the update went through" % rank)
        except _lib.TcarError as e:
            assert "differs from rank 0's" in str(e)
        assert reached == ["flush"] and xc.order[-1] == "update_digest"
        ret[rank] = "ok"
    except Exception as e:
        import traceback
        ret[rank] = "FAIL: " + repr(e) + "\n" + traceback.format_exc()
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_agree_over_gloo_returns_on_equal_digests_and_raises_on_both_ranks_otherwise():
    world = 2
    ret = launch(_agree_worker, world)
    for r in range(world):
        assert ret.get(r) == "ok", ret.get(r)


# ----------------------------------------------------------------- validation, then agreement, then staging
class _Agree:
    collective = True

    def __init__(self, log):
        self.log = log

    def agree(self, digest, key="update_digest", device=None):
        assert isinstance(digest, bytes) and len(digest) == 16
        self.log.append(("agree", digest))


@pytest.mark.parametrize("which", ["sharded", "replica"])
def test_a_refused_request_reaches_no_collective_and_an_accepted_one_agrees_before_it_stages(which):
    from tcar_amd.dp import DPEngine, update_digest
    from tcar_amd.engine import TcarEngine
    from tcar_amd.sharded import ShardedEngine
    log = []
    eng = _unbuilt(ShardedEngine if which == "sharded" else DPEngine, keys=False)
    eng.xch = _Agree(log)
    eng.flush = lambda: log.append(("flush",))

    def stage(*a):
        log.append(("stage",))
        raise RuntimeError("staged")
    eng._stage_update = stage
    call = eng.shard_update_items if which == "sharded" else eng.replica_update_items
    row = np.zeros((2, 250), np.float32)
    refused = [(lambda: call([], content=row[:0]), "ids must be an integer array [U] of at least one catalog row"),
               (lambda: call([3, 700], content=row), "ids must lie in [0, N = 700)"),
               (lambda: call([5, 5], content=row), "ids must be pairwise distinct"),
               (lambda: call([5, 6]), "update_items needs at least one of content, item_rows, mwdhm, keys, categories"),
               (lambda: call([5, 6], content=row[:, :249]), "content must be a float array [2, 250]"),
               (lambda: call([5, 6], mwdhm=np.ones((2, 4), np.int32)), "mwdhm must be an integer array [2, 5]"),
               (lambda: call([5, 6], keys=[1, 2]), "keys update the item keys: call set_item_keys(keys) first"),
               (lambda: call([5, 6], categories=[1, 2]), "categories update the category table: call set_categories(cat_of_item) first")]
    for fn, text in refused:
        with pytest.raises(ValueError) as e:
            fn()
        assert str(e.value) == text
    assert log == []                                   # the same ValueErrors as update_items, before anything else
    with pytest.raises(RuntimeError, match="staged"):
        call([6, 5], content=row)
    want = update_digest(*TcarEngine._update_request(eng, [6, 5], row, None, None, None, None))
    # (the replica leaves flush to TcarEngine.update_items, behind the agreement; the sharded engine flushes first)
    assert [x for x in log if x[0] != "flush"] == [("agree", want), ("stage",)]
    assert log[0] == (("flush",) if which == "sharded" else ("agree", want))
    # verify=False: no agreement, and with it no synchronisation
    del log[:]
    with pytest.raises(RuntimeError, match="staged"):
        call([6, 5], content=row, verify=False)
    assert [x[0] for x in log if x[0] != "flush"] == ["stage"]
    # the old names keep refusing
    with pytest.raises(_lib.TcarError):
        eng.update_items([6, 5], content=row)


# -------------------------------------------------------------------------------------------------- the model
class _Recorder:
    def __init__(self, names):
        self.calls = []
        for n in names:
            setattr(self, n, (lambda n: lambda ids, **kw: self.calls.append((n, np.asarray(ids).tolist(), kw)))(n))


@pytest.mark.parametrize("names, want", [(("update_items",), "update_items"),
                                         (("update_items", "replica_update_items"), "replica_update_items"),
                                         (("update_items", "shard_update_items", "shard_retrieve"), "shard_update_items")])


def test_update_articles_routes_by_engine(names, want):
    from tcar_amd.host.data import publish_fields
    from tcar_amd.host.model import Seq2SeqAttNN
    m = Seq2SeqAttNN.__new__(Seq2SeqAttNN)
    t0 = datetime.datetime(2017, 3, 30, 22, 58)
    m.publish_time = [t0 + datetime.timedelta(minutes=17 * i) for i in range(12)]
    m.publish_time_MWDHM = np.asarray([publish_fields(t) for t in m.publish_time], np.int32)
    m.candidate_n, m._keys, m._key_t0, m._cat = 13, None, None, None
    m.engine = _Recorder(names)
    content = np.ones((2, 4), np.float32)
    when = [datetime.datetime(2017, 4, 2, 0, 0), t0]
    m.update_articles([7, 2], content=content, publish_time=when)
    (name, ids, kw), = m.engine.calls
    assert name == want and ids == [7, 2] and kw["content"] is content and sorted(kw) == ["categories", "content", "item_rows", "keys", "mwdhm"]
    assert np.asarray(kw["mwdhm"]).tolist() == [list(publish_fields(t)) for t in when]
    assert m.publish_time_MWDHM[[7, 2]].tolist() == np.asarray(kw["mwdhm"]).tolist()
