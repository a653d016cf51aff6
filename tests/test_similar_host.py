"""Host side of related items (include/tcar_similar.h): the numpy model of tests/similar_ref.py against a brute-force fp64 loop, the
ABI layer, the argument checks of the three entry points, which answer before anything is launched, the request validation of the
engine and of the model class, and the command-line flag — none of it needs a GPU."""
import ctypes as C
import types

import numpy as np
import pytest

import tcar_amd  # noqa: F401
from tcar_amd import _lib

from similar_ref import lists, query_rows, rnorm_f32, sims_f32, sims_f64, tol_sim


def _exact(rng, N, H):
    """rows of four 0.5s (norm exactly 1), row 0 all zero: every cosine is a multiple of 1/4 in any order"""
    x = np.zeros((N, H), np.float32)
    for n in range(1, N):
        x[n, rng.choice(H, 4, replace=False)] = 0.5
    return x


def test_the_model_against_a_brute_force_loop():
    rng = np.random.RandomState(5)
    for N, H, Q, k in ((6, 4, 2, 3), (30, 7, 5, 8), (40, 9, 6, 50), (25, 16, 4, 5)):
        content = _exact(rng, N, H)
        ids = rng.randint(-1, N, Q)
        ids[0] = 0
        rows = query_rows(content, ids)
        want = np.zeros((Q, N))
        for q in range(Q):
            for n in range(N):
                x, y = rows[q].astype(np.float64), content[n].astype(np.float64)
                nx, ny = np.sqrt(sum(v * v for v in x)), np.sqrt(sum(v * v for v in y))
                want[q, n] = sum(a * b for a, b in zip(x, y)) / (nx * ny) if nx > 0 and ny > 0 else 0.0
        s32, s64 = sims_f32(rows, content), sims_f64(rows, content)
        assert s32.dtype == np.float32 and np.array_equal(s32.astype(np.float64), want) and np.array_equal(s64, want)
        assert not np.signbit(s32[0]).any() and (rnorm_f32(content)[1:] == 1).all() and rnorm_f32(content)[0] == 0
        assert np.array_equal(sims_f32(content, content), sims_f32(content, content).T)
        excl = [[int(i)] if i >= 0 else [] for i in ids]
        topk, score = lists(s32, k, excl=excl)
        for q in range(Q):
            order = sorted((n for n in range(N) if n != ids[q]), key=lambda n: (want[q, n], n), reverse=True)[:k]
            assert topk[q, :len(order)].tolist() == order and (topk[q, len(order):] == -1).all()
            assert score[q, :len(order)].tolist() == [want[q, n] for n in order] and (score[q, len(order):] == 0).all()
    # random rows: the fp32 model within the bound of the fp64 one
    X = rng.standard_normal((20, 250)).astype(np.float32)
    assert np.abs(sims_f32(X[:5], X) - sims_f64(X[:5], X)).max() <= tol_sim(250)


def test_the_similar_layer_is_bound_behind_mmr_and_the_other_layers_are_where_they_were():
    lib = _lib.load()
    i = _lib.ABI_LAYERS.index(("SIMILAR", "tcar_similar.h"))
    assert _lib.ABI_LAYERS[i - 1] == ("MMR", "tcar_mmr.h")
    assert _lib.ABI_LAYERS[-2:] == [("RETRIEVE_SHARD", "tcar_retrieve_shard.h"), ("RAGGED", "tcar_ragged.h")]
    assert _lib.SIMILAR_SYMBOLS == ["tcar_similar_abi_version", "tcar_sim_queries", "tcar_sim_panel", "tcar_similar_step"]
    assert lib.tcar_similar_abi_version() == _lib.SIMILAR_ABI_VERSION == 1
    assert _lib.SIMILAR_HEADER in _lib.HEADERS and "similar.hip" in _lib.SOURCES          # both enter the build id
    assert [f[0] for f in _lib.Similar._fields_] == ["qid", "qrow", "ld_qrow", "xq", "rq"] and C.sizeof(_lib.Similar) == 40
    i32, i64, vp, P = C.c_int32, C.c_int64, C.c_void_p, C.POINTER
    assert lib.tcar_sim_queries.argtypes == [i32, i32, i32, vp, i64, vp, vp, i64, vp, i64, vp, vp]
    assert lib.tcar_sim_panel.argtypes == [i32, i32, i32, i32, vp, i64, vp, i64, vp, vp, i64, vp]
    assert lib.tcar_similar_step.argtypes == [P(_lib.Ctx), i32, P(_lib.Similar), P(_lib.Serve), P(_lib.Window), P(_lib.Quota), vp]
    every = [s for prefix, _ in _lib.ABI_LAYERS if prefix != "SIMILAR" for s in getattr(_lib, _lib._name(prefix, "SYMBOLS"))]
    assert not set(_lib.SIMILAR_SYMBOLS) & set(every)


def test_argument_errors_come_back_before_any_launch():
    lib = _lib.load()
    buf = (C.c_float * 4096)()                    # host memory: never dereferenced, an accepted call would have to launch
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 2)
    off4 = C.c_void_p(p.value + 4)
    # ---- tcar_sim_queries
    names = ("Q", "N", "H", "content", "ldc", "qid", "qrow", "ldq", "xq", "ldx", "rq", "stream")
    base = dict(Q=3, N=50, H=8, content=p, ldc=8, qid=p, qrow=None, ldq=0, xq=p, ldx=8, rq=p, stream=None)
    queries = lambda **kw: lib.tcar_sim_queries(*[dict(base, **kw)[a] for a in names])          # noqa: E731
    for bad in (dict(qrow=p, ldq=8), dict(qid=None), dict(Q=-1), dict(N=0), dict(H=0), dict(content=None), dict(ldc=7), dict(content=odd),
                dict(qid=odd), dict(xq=None), dict(ldx=7), dict(xq=odd), dict(rq=None), dict(rq=odd),
                dict(qid=None, qrow=p, ldq=7), dict(qid=None, qrow=odd, ldq=8)):
        assert queries(**bad) == -1, bad
    assert queries(Q=0) == 0 and queries(Q=0, qid=None, qrow=p, ldq=8, content=None) == 0
    # ---- tcar_sim_panel
    names = ("Q", "n0", "n", "H", "content", "ldc", "xq", "ldx", "rq", "panel", "ld", "stream")
    base = dict(Q=3, n0=0, n=40, H=8, content=p, ldc=8, xq=p, ldx=8, rq=p, panel=p, ld=40, stream=None)
    panel = lambda **kw: lib.tcar_sim_panel(*[dict(base, **kw)[a] for a in names])              # noqa: E731
    for bad in (dict(ld=36), dict(ld=42), dict(n=41, ld=41), dict(n=49153, ld=49156), dict(H=0), dict(H=-3), dict(Q=-1), dict(n0=-1),
                dict(n=-1), dict(content=None), dict(xq=None), dict(rq=None), dict(panel=None), dict(ldc=7), dict(ldx=7),
                dict(panel=off4), dict(content=odd), dict(xq=odd), dict(rq=odd), dict(n0=2 ** 31 - 8)):
        assert panel(**bad) == -1, bad
    assert panel(Q=0) == 0 and panel(n=0) == 0 and panel(n=0, ld=0) == 0
    assert panel(Q=0, n=49152, ld=49152) == 0 and panel(Q=0, content=off4, xq=off4) == 0      # no 16-byte alignment asked of the tables
    # ---- tcar_similar_step
    ctx, q, s, w, quota = _lib.Ctx(), _lib.Similar(), _lib.Serve(), _lib.Window(), _lib.Quota()
    ctx.d.n_items, ctx.d.H, ctx.d.ldh, ctx.d.ldt = 50, 8, 64, 64
    ctx.E = p.value
    q.qid, q.xq, q.rq = p.value, p.value, p.value
    for f, v in dict(k=20, panel=128, panel_buf=p.value, state=p.value, state_bytes=3 * 64 * 4, topk=p.value, score=p.value).items():
        setattr(s, f, v)
    step = lambda Q=3, cc=ctx, qq=q, ss=s, ww=None, uu=None: lib.tcar_similar_step(                # noqa: E731
        C.byref(cc) if cc is not None else None, Q, C.byref(qq) if qq is not None else None, C.byref(ss) if ss is not None else None,
        C.byref(ww) if ww is not None else None, C.byref(uu) if uu is not None else None, None)
    assert step(Q=0) == 0                           # the base is good: what follows fails for the reason it names

    def broken(obj, **kw):
        cp = type(obj)()
        C.memmove(C.byref(cp), C.byref(obj), C.sizeof(obj))
        for f, v in kw.items():
            setattr(cp, f, v)
        return cp
    assert step(cc=None) == -1 and step(qq=None) == -1 and step(ss=None) == -1 and step(Q=-1) == -1
    for kw in (dict(qrow=p.value, ld_qrow=8), dict(qid=None), dict(xq=None), dict(rq=None), dict(qid=None, qrow=p.value, ld_qrow=7)):
        assert step(qq=broken(q, **kw)) == -1, kw
    for kw in (dict(k=0), dict(k=65), dict(panel=0), dict(panel=100), dict(panel=49280), dict(panel_buf=None), dict(panel_buf=p.value + 4),
               dict(state=None), dict(topk=None), dict(state_bytes=8), dict(X=-1), dict(excl=p.value, X=0)):
        assert step(ss=broken(s, **kw)) == -1, kw
    assert step(cc=broken(ctx, E=None)) == -1
    assert step(ww=w) == -1                         # a window without its pointers
    quota.cat, quota.cap = p.value, 0
    assert step(uu=quota) == -1                     # a cap below 1
    assert step(Q=0, qq=broken(q, qid=None, qrow=p.value, ld_qrow=8)) == 0


def _stub():
    from tcar_amd.engine import TcarEngine
    eng = TcarEngine.__new__(TcarEngine)
    eng.shard, eng.geo = (0, 700), types.SimpleNamespace(N=700, Npad=768, H=8, ldh=64, ek=168)
    return eng


def test_the_engine_validates_the_request_before_any_device_call():
    from tcar_amd.host.model import Seq2SeqAttNN
    from tcar_amd.sharded import ShardedEngine
    eng = _stub()
    rows = np.zeros((3, 8), np.float32)
    for kw, text in ((dict(), "exactly one of ids"), (dict(ids=[1], content=rows), "exactly one of ids"),
                     (dict(ids=[1.5]), "ids must be"), (dict(ids=[[1, 2]]), "ids must be"), (dict(ids=[]), "ids must be"),
                     (dict(ids=[True]), "ids must be"), (dict(ids=3), "ids must be"),
                     (dict(content=np.zeros((3, 7), np.float32)), "content must be"), (dict(content=np.zeros(8, np.float32)), "content must be"),
                     (dict(content=np.zeros((3, 8), np.int32)), "content must be"), (dict(content=np.zeros((0, 8), np.float32)), "content must be"),
                     (dict(ids=[1], k=0), "k must be"), (dict(ids=[1], k=65), "k must be"), (dict(ids=[1], k=True), "k must be"),
                     (dict(ids=[1], k=2.0), "k must be"), (dict(ids=[1], exclude_self=1), "exclude_self must be"),
                     (dict(ids=[1, 2], exclude=[[3]]), "exclude must be"), (dict(ids=[1], exclude=[3]), "exclude must be"),
                     (dict(ids=[1], exclude=[[0.5]]), "exclude must be"), (dict(ids=[1], panel=100), "panel must be"),
                     (dict(ids=[1], panel=49280), "panel must be"), (dict(ids=[1], window=(0, 5)), "call set_item_keys"),
                     (dict(ids=[1], max_per_category=2), "call set_categories"), (dict(ids=[1], max_per_category=0), "max_per_category must be")):
        with pytest.raises(ValueError, match=text):
            eng.similar_items(**kw)
    eng._item_keys = object()
    for window in ((0,), 5, (np.zeros(3), np.zeros(3))):
        with pytest.raises(ValueError, match="window = "):
            eng.similar_items(ids=[1, 2], window=window)
    # what a good request becomes: ids outside the catalog are the empty query, exclude_self is the first column of the lists
    Q, qid, qrows, excl, bounds, quota, panel = eng._similar_request(np.asarray([5, -1, 700, 2 ** 40, 699]), 20, None, True,
                                                                    [[1, 2]] * 5, None, (3, [4, 5, 6, 7, 8]), None)
    assert Q == 5 and qid.dtype == np.int32 and qid.tolist() == [5, -1, -1, -1, 699] and qrows is None and quota is None
    assert excl.dtype == np.int32 and excl.tolist() == [[5, 1, 2], [-1, 1, 2], [-1, 1, 2], [-1, 1, 2], [699, 1, 2]] and panel == 768
    assert bounds[0].tolist() == [3] * 5 and bounds[1].tolist() == [4, 5, 6, 7, 8]
    Q, qid, qrows, excl, bounds, quota, panel = eng._similar_request(None, np.int64(7), rows.astype(np.float64), True, None, 256, None, None)
    assert Q == 3 and qid is None and qrows.dtype == np.float32 and qrows.shape == (3, 8) and excl is None and bounds is None and panel == 256
    assert eng._similar_request([4], 1, None, False, None, None, None, None)[3] is None
    # engines that do not hold the whole catalog refuse, after the request itself was found good
    eng.shard = (0, 350)
    with pytest.raises(_lib.TcarError, match="whole catalog"):
        eng.similar_items(ids=[1])
    with pytest.raises(ValueError, match="k must be"):
        eng.similar_items(ids=[1], k=0)
    sh = ShardedEngine.__new__(ShardedEngine)
    with pytest.raises(_lib.TcarError, match="similar_items.*whole catalog"):
        sh.similar_items(ids=[1])
    m = Seq2SeqAttNN.__new__(Seq2SeqAttNN)
    m.engine = sh
    for call in (lambda: m.related_articles([1], k=5), lambda: m.similar_to_content(rows, k=5)):
        with pytest.raises(_lib.TcarError, match="whole catalog"):
            call()


def test_eval_related_is_range_checked_and_refused_where_it_cannot_work():
    from tcar_amd.host import cli
    from tcar_amd.host.model import Seq2SeqAttNN
    check = lambda gpus=1, **values: cli.check_eval_options(values, gpus=gpus)
    for bad in (-1, 65, 1000):
        with pytest.raises(ValueError, match=r"--eval_related must be in \[1, 64\]"):
            check(eval_related=bad, dp_mode="replica")
    for bad in (1.5, "3", True):
        with pytest.raises(ValueError, match="--eval_related must be an integer"):
            check(eval_related=bad, dp_mode="replica")
    with pytest.raises(ValueError, match="eval_related.*sharded"):
        check(eval_related=5, dp_mode="sharded")
    for ok in ((0, "sharded"), (1, "replica"), (64, "replica"), (np.int64(10), "replica")):
        check(eval_related=ok[0], dp_mode=ok[1])
    ap = cli.build_parser()
    assert ap.parse_args([]).eval_related == 0 and ap.parse_args(["--eval_related", "10"]).eval_related == 10
    m = Seq2SeqAttNN.__new__(Seq2SeqAttNN)
    assert m._eval_request({}).eval_related == 0 and m._eval_request({"eval_related": 7}).eval_related == 7
    m.eval_related = 9
    assert m._eval_request({}).eval_related == 9 and m._eval_request({"eval_related": 0}).eval_related == 0
    for kw, text in ((dict(eval_related=65), r"\[1, 64\]"), (dict(eval_related=4, dp_mode="sharded"), "sharded")):
        with pytest.raises(ValueError, match=text):
            m._eval_request(kw)


def test_related_sums():
    from tcar_amd.host.metrics import related_sums
    cat = np.asarray([0, 0, 1, 1, 2])
    topk = np.asarray([[1, 2, -1], [0, 1, 4], [-1, -1, -1]])
    sims = np.asarray([[0.5, 0.25, 9.0], [1.0, 0.5, 0.0], [7.0, 7.0, 7.0]], np.float32)
    cos, same = related_sums(topk, sims, [0, 3, 4], cat)
    assert cos == 2.25 and same == 1.0             # item 1 shares article 0's category; nothing listed shares article 3's
