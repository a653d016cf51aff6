"""Host side of the warm start (include/tcar_warm.h): the fp64 statement of the rule (tests/warm_ref.py) on hand-made cases, the ABI
layer, the argument checks of both entry points, which answer before anything is launched, the request validation of the engine
and of the model class, the refusals of the engines that do not hold one whole catalog, the command-line flags and the sample of
--eval_coldstart — none of it needs a GPU."""
import ctypes as C
import types

import numpy as np
import pytest

import tcar_amd  # noqa: F401
from tcar_amd import _lib

from warm_ref import EPS, blend, bound


# --------------------------------------------------------------------------------------------- the reference
def test_the_reference_on_hand_made_lists():
    table = np.asarray([[1.0, -2.0, 4.0], [3.0, 0.0, -4.0], [8.0, 8.0, 8.0], [-1.0, 1.0, 0.5]], np.float32)
    nbr = np.asarray([[-1, -1, -1],               # every slot empty
                      [2, -1, -1],                # one donor: the row itself, whatever its weight
                      [0, 1, 3],                  # a negative cosine is dropped
                      [0, 1, 3],                  # ... and so is one below min_sim (row 3 at min_sim 0.3)
                      [1, 1, 0],                  # a repeated donor counts every time it is listed
                      [0, 4, -7]])                # ids outside the table are empty slots
    sim = np.asarray([[0.9, 0.5, 0.1], [0.25, 0.0, 0.0], [0.5, -0.5, 0.5], [0.5, 0.25, 0.75], [0.5, 0.25, 0.25], [0.5, 0.9, 0.9]], np.float32)
    rows, support, wsum, scale = blend(nbr, sim, table)
    table = table.astype(np.float64)
    assert support.tolist() == [0, 1, 2, 3, 3, 1] and wsum.tolist() == [0.0, 0.25, 1.0, 1.5, 1.0, 0.5]
    assert not rows[0].any() and not np.signbit(rows[0]).any() and not scale[0].any()
    assert rows[1].tolist() == [8.0, 8.0, 8.0]
    assert rows[2].tolist() == [0.0, -0.5, 2.25] and scale[2].tolist() == [1.0, 2.0, 4.0]            # (row 0 + row 3) / 2
    assert np.array_equal(rows[3], (0.5 * table[0] + 0.25 * table[1] + 0.75 * table[3]) / 1.5)
    assert np.array_equal(rows[4], 0.75 * table[1] + 0.25 * table[0])
    assert rows[5].tolist() == [1.0, -2.0, 4.0]
    # min_sim: compared on the fp32 values, >= keeps a cosine that equals it
    rows, support, wsum, _ = blend(nbr, sim, table, min_sim=0.5)
    assert support.tolist() == [0, 0, 2, 2, 1, 1] and wsum.tolist() == [0, 0, 1.0, 1.25, 0.5, 0.5]
    assert not rows[1].any() and np.array_equal(rows[3], (0.5 * table[0] + 0.75 * table[3]) / 1.25)
    # NaN and infinities among the cosines: NaN donates nothing
    _, support, _, _ = blend([[0, 1]], np.asarray([[np.nan, 0.5]], np.float32), table)
    assert support.tolist() == [1]
    # a convex combination: every entry inside the range of its donors, and the bound scales with them
    rng = np.random.RandomState(0)
    t = rng.standard_normal((50, 9))
    n, s = rng.randint(0, 50, (6, 7)), rng.random_sample((6, 7)).astype(np.float32)
    rows, _, _, scale = blend(n, s, t)
    assert (rows <= t[n].max(1) + 1e-12).all() and (rows >= t[n].min(1) - 1e-12).all()
    assert np.array_equal(bound(7, scale), 16 * EPS * np.abs(t[n]).max(1))


# --------------------------------------------------------------------------------------------- the ABI layer
def test_the_warm_layer_is_bound_and_its_header_is_what_the_bindings_read():
    lib = _lib.load()
    assert ("WARM", "tcar_warm.h") in _lib.ABI_LAYERS and _lib.WARM_HEADER in _lib.HEADERS and "warm.hip" in _lib.SOURCES
    assert _lib.WARM_SYMBOLS == ["tcar_warm_abi_version", "tcar_rows_blend", "tcar_warm_step"]
    assert lib.tcar_warm_abi_version() == _lib.WARM_ABI_VERSION == 1
    assert [f[0] for f in _lib.Warm._fields_] == ["U", "ids", "min_sim", "xq", "rq", "serve", "window", "rows", "ld_rows", "support", "wsum",
                                                  "zero_moments"]
    i32, i64, f32, vp = C.c_int32, C.c_int64, C.c_float, C.c_void_p
    assert lib.tcar_rows_blend.argtypes == [i32, i32, i32, i32, vp, vp, f32, vp, i64, vp, i64, vp, vp, vp]
    assert lib.tcar_warm_step.argtypes == [C.POINTER(_lib.Ctx), C.POINTER(_lib.Warm), vp]
    every = [s for prefix, _ in _lib.ABI_LAYERS if prefix != "WARM" for s in getattr(_lib, _lib._name(prefix, "SYMBOLS"))]
    assert not set(_lib.WARM_SYMBOLS) & set(every)


def test_argument_errors_come_back_before_any_launch():
    lib = _lib.load()
    buf = (C.c_float * 8192)()                    # host memory: never dereferenced, an accepted call would have to launch
    base_p = (C.addressof(buf) + 15) & ~15
    p, far = C.c_void_p(base_p), C.c_void_p(base_p + 16384)
    odd, off4 = C.c_void_p(base_p + 2), C.c_void_p(base_p + 4)
    names = ("U", "k", "N", "H", "nbr", "sim", "min_sim", "table", "ldt", "out", "ldo", "support", "wsum", "stream")
    base = dict(U=3, k=16, N=50, H=8, nbr=p, sim=p, min_sim=0.0, table=p, ldt=8, out=far, ldo=8, support=p, wsum=p, stream=None)
    blend_ = lambda **kw: lib.tcar_rows_blend(*[dict(base, **kw)[a] for a in names])          # noqa: E731
    for bad in (dict(U=-1), dict(k=0), dict(k=65), dict(N=0), dict(H=0), dict(nbr=None), dict(sim=None), dict(table=None), dict(out=None),
                dict(support=None), dict(wsum=None), dict(nbr=odd), dict(sim=odd), dict(table=odd), dict(out=odd), dict(support=odd),
                dict(wsum=odd), dict(ldt=7), dict(ldo=7), dict(min_sim=-0.5), dict(min_sim=1.5), dict(min_sim=float("nan")),
                dict(out=p), dict(out=C.c_void_p(base_p + 4 * (49 * 8 + 7))),               # out inside the rows of table
                dict(table=far, out=C.c_void_p(base_p + 16384 - 4 * 17), ldo=8)):          # the last row of out reaches into table
        assert blend_(**bad) == -1, bad
    assert blend_(U=0) == 0 and blend_(U=0, out=off4, table=off4, ldt=9, ldo=11) == 0     # no 16-byte alignment asked of the tables
    assert blend_(U=0, min_sim=1.0) == 0 and blend_(U=0, k=64) == 0 and blend_(U=0, k=1) == 0

    # ---- tcar_warm_step
    ctx, w, s, win = _lib.Ctx(), _lib.Warm(), _lib.Serve(), _lib.Window()
    ctx.d.n_items, ctx.d.H, ctx.d.Ht, ctx.d.ldh, ctx.d.ldt = 50, 8, 8, 64, 64
    ctx.E, ctx.Mi, ctx.Vi = far.value, p.value, p.value                                       # (E: 50 rows of ek = 448 floats; never read)
    for f, v in dict(k=16, panel=128, panel_buf=p.value, state=p.value, state_bytes=1 << 20, excl=p.value, X=3, topk=p.value,
                     score=p.value).items():
        setattr(s, f, v)
    w.U, w.ids, w.min_sim, w.xq, w.rq, w.serve = 0, p.value, 0.25, p.value, p.value, C.addressof(s)
    w.rows, w.ld_rows, w.support, w.wsum, w.zero_moments = p.value, 8, p.value, p.value, 1
    step = lambda cc=ctx, ww=w: lib.tcar_warm_step(C.byref(cc) if cc is not None else None, C.byref(ww) if ww is not None else None, None)  # noqa: E731
    assert step() == 0                              # U == 0 with good arguments: nothing is launched

    def broken(obj, **kw):
        cp = type(obj)()
        C.memmove(C.byref(cp), C.byref(obj), C.sizeof(obj))
        for f, v in kw.items():
            setattr(cp, f, v)
        return cp
    assert step(cc=None) == -1 and step(ww=None) == -1
    for kw in (dict(U=-1), dict(ids=None), dict(xq=None), dict(rq=None), dict(serve=None), dict(rows=None), dict(rows=off4.value),
               dict(ld_rows=7), dict(ld_rows=10), dict(support=None), dict(wsum=None), dict(min_sim=-1.0), dict(min_sim=2.0),
               dict(window=C.addressof(win))):                                             # a window without its pointers
        assert step(ww=broken(w, **kw)) == -1, kw
    for kw in (dict(k=0), dict(k=65), dict(panel=0), dict(panel=100), dict(panel=49280), dict(panel_buf=None), dict(panel_buf=off4.value),
               dict(state=None), dict(topk=None), dict(score=None), dict(excl=None), dict(X=0)):
        bad_s = broken(s, **kw)
        assert step(ww=broken(w, serve=C.addressof(bad_s))) == -1, kw
    for kw in (dict(E=None), dict(E=off4.value), dict(Mi=None), dict(Vi=None), dict(scoring=3)):   # (scoring without planes)
        assert step(cc=broken(ctx, **kw)) == -1, kw
    assert step(cc=broken(ctx, Mi=None), ww=broken(w, zero_moments=0)) == 0                 # the moments are needed only to be zeroed
    bad_d = broken(ctx)
    bad_d.d.ldh = 60
    assert step(cc=bad_d) == -1
    small, few = broken(s, state_bytes=8), broken(s, X=2)
    assert step(ww=broken(w, U=3, serve=C.addressof(small))) == -1                          # a state too small for U rows
    assert step(ww=broken(w, U=3, serve=C.addressof(few))) == -1                            # exclusion lists that cannot hold the U ids
    assert step(ww=broken(w, U=3, rows=far.value)) == -1                                    # rows inside E


# --------------------------------------------------------------------------------------------- the engine
def _stub():
    from tcar_amd.engine import TcarEngine
    eng = TcarEngine.__new__(TcarEngine)
    eng.shard, eng.geo = (0, 700), types.SimpleNamespace(N=700, Npad=768, H=8, ldh=64, ek=168)
    return eng


def test_the_engine_validates_the_request_before_any_device_call():
    eng = _stub()
    for kw, text in ((dict(ids=[1.5]), "ids must be an integer array"), (dict(ids=[[1, 2]]), "ids must be an integer array"),
                     (dict(ids=[]), "ids must be an integer array"), (dict(ids=3), "ids must be an integer array"),
                     (dict(ids=[-1]), r"ids must lie in \[0, N = 700\)"), (dict(ids=[700]), "ids must lie in"),
                     (dict(ids=[4, 9, 4]), "pairwise distinct"),
                     (dict(ids=[1], k=0), "k must be"), (dict(ids=[1], k=65), "k must be"), (dict(ids=[1], k=True), "k must be"),
                     (dict(ids=[1], k=2.0), "k must be"), (dict(ids=[1], min_sim=-0.1), "min_sim must be"),
                     (dict(ids=[1], min_sim=1.5), "min_sim must be"), (dict(ids=[1], min_sim=float("nan")), "min_sim must be"),
                     (dict(ids=[1], min_sim="0.5"), "min_sim must be"), (dict(ids=[1], min_sim=True), "min_sim must be"),
                     (dict(ids=[1, 2], exclude=[[3]]), "exclude must be"), (dict(ids=[1], exclude=[3]), "exclude must be"),
                     (dict(ids=[1], exclude=[[0.5]]), "exclude must be"), (dict(ids=[1], panel=100), "panel must be"),
                     (dict(ids=[1], panel=49280), "panel must be"), (dict(ids=[1], window=(0, 5)), "call set_item_keys")):
        with pytest.raises(ValueError, match=text):
            eng.warm_start_items(**kw)
    eng._item_keys = object()
    for window in ((0,), 5, (np.zeros(3), np.zeros(3))):
        with pytest.raises(ValueError, match="window = "):
            eng.warm_start_items(ids=[1, 2], window=window)
    # the ids are validated by the code update_items validates them with: the same refusals, word for word
    for ids in ([1.5], [-1], [700], [4, 9, 4]):
        with pytest.raises(ValueError) as a:
            eng.warm_start_items(ids)
        with pytest.raises(ValueError) as b:
            eng.update_items(ids, keys=[0] * len(ids))
        assert str(a.value) == str(b.value)
    # what a good request becomes: ONE pair of scalars is every row's window, a pair per id stays
    ids, k, min_sim, excl, bounds, panel = eng._warm_request(np.asarray([5, 699, 0]), np.int64(7), 0.25, [[1, -4, 2 ** 40]] * 3, (3, 90), None)
    assert ids.dtype == np.int32 and ids.tolist() == [5, 699, 0] and k == 7 and min_sim == 0.25 and panel == 768
    assert excl.dtype == np.int32 and excl.tolist() == [[1, -1, -1]] * 3
    assert bounds[0].tolist() == [3] * 3 and bounds[1].tolist() == [90] * 3
    bounds = eng._warm_request([5, 6], 16, 0, None, ([1, 2], [8, 9]), 256)[4]
    assert bounds[0].tolist() == [1, 2] and bounds[1].tolist() == [8, 9]
    assert eng._warm_request([5], 1, 1, np.zeros((1, 0), np.int64), None, 128)[3:] == (None, None, 128)
    # an engine that holds a shard refuses, after the request itself was found good
    eng.shard = (0, 350)
    with pytest.raises(_lib.TcarError, match="needs the whole catalog on one engine"):
        eng.warm_start_items([1])
    with pytest.raises(ValueError, match="k must be"):
        eng.warm_start_items([1], k=0)


def test_the_sharded_and_the_replica_engine_and_the_model_over_them_refuse():
    from tcar_amd.dp import DPEngine
    from tcar_amd.host.model import Seq2SeqAttNN
    from tcar_amd.sharded import ShardedEngine
    for cls in (ShardedEngine, DPEngine):
        e = cls.__new__(cls)
        with pytest.raises(_lib.TcarError, match="needs the whole catalog on one engine"):
            e.warm_start_items([1])
        m = Seq2SeqAttNN.__new__(Seq2SeqAttNN)
        m.engine = e
        for call in (lambda: m.warm_start_articles([1]), lambda: m.update_articles([1], item_rows="neighbors"),
                     lambda: m.update_articles([1], content=np.zeros((1, 8), np.float32), item_rows="neighbors")):
            with pytest.raises(_lib.TcarError, match="whole catalog on one engine"):
                call()


def test_update_articles_takes_neighbors_and_no_other_string():
    from tcar_amd.host.model import Seq2SeqAttNN

    class Recorder:
        def __init__(self):
            self.calls = []

        def update_items(self, ids, **kw):
            self.calls.append(("update_items", np.asarray(ids).tolist(), sorted(k for k, v in kw.items() if v is not None)))

        def warm_start_items(self, ids, **kw):
            self.calls.append(("warm_start_items", np.asarray(ids).tolist(), kw))
            return "warm"

        def set_item_keys(self, keys):
            self.calls.append(("set_item_keys",))
    m = Seq2SeqAttNN.__new__(Seq2SeqAttNN)
    m.engine, m._keys, m._cat = Recorder(), None, None
    for bad in ("bogus", "neighbours", "", "Neighbors"):
        with pytest.raises(ValueError, match='item_rows must be an array .* "neighbors"'):
            m.update_articles([1, 2], content=np.zeros((2, 8), np.float32), item_rows=bad)
    assert m.engine.calls == []                                     # refused before the update it would follow
    # the update of the content first, then the warm start of the same rows
    m.update_articles([1, 2], content=np.zeros((2, 8), np.float32), item_rows="neighbors", donors=9)
    assert m.engine.calls == [("update_items", [1, 2], ["content"]),
                              ("warm_start_items", [1, 2], dict(k=9, min_sim=0.0, window=None))]
    # nothing but the warm start; an array and None go where they went
    m.engine.calls.clear()
    m.update_articles([3], item_rows="neighbors")
    m.update_articles([3], item_rows=np.ones((1, 8), np.float32))
    m.update_articles([3], content=np.ones((1, 8), np.float32))
    assert [c[:2] for c in m.engine.calls] == [("warm_start_items", [3]), ("update_items", [3]), ("update_items", [3])]
    assert m.engine.calls[0][2] == dict(k=16, min_sim=0.0, window=None) and m.engine.calls[1][2] == ["item_rows"]
    assert m.engine.calls[2][2] == ["content"]
    # a donor window is in minutes over the item keys: they are installed first
    import datetime as dt
    m.engine.calls.clear()
    m.candidate_n, m.publish_time = 4, [dt.datetime(2020, 1, 1, 0, i) for i in range(3)]
    assert m.warm_start_articles([0], donors=4, window=(0, 2), min_sim=0.5, panel=128) == "warm"
    assert m.engine.calls == [("set_item_keys",), ("warm_start_items", [0], dict(k=4, min_sim=0.5, window=(0, 2), panel=128))]


# --------------------------------------------------------------------------------------------- the command line
def test_eval_coldstart_is_range_checked_and_refused_where_it_cannot_work():
    from tcar_amd.host import cli
    from tcar_amd.host.eval_passes import COLD_START_OPTIONS, ColdStartRequest, check_cold_start_options, cold_start_request
    from tcar_amd.host.model import Seq2SeqAttNN
    check = lambda gpus=1, **values: check_cold_start_options(values, gpus=gpus)       # noqa: E731
    assert [o.name for o in COLD_START_OPTIONS] == ["coldstart", "coldstart_donors"]
    assert all(r.text.startswith("--eval_coldstart ") for r in COLD_START_OPTIONS[0].rules)
    assert all(r.text.startswith("--coldstart_donors ") for r in COLD_START_OPTIONS[1].rules)
    for bad in (-0.25, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"--eval_coldstart must be a fraction in \(0, 0.5\]"):
            check(coldstart=bad, eval_panel=128)
    for bad in (0.51, 1, 2.0):
        with pytest.raises(ValueError, match="--eval_coldstart must be at most 0.5"):
            check(coldstart=bad, eval_panel=128)
    for bad in ("0.25", True, None):
        with pytest.raises(ValueError, match="--eval_coldstart must be a number"):
            check(coldstart=bad, eval_panel=128)
    with pytest.raises(ValueError, match="--eval_coldstart needs --eval_panel"):
        check(coldstart=0.25)
    with pytest.raises(ValueError, match="--eval_coldstart .* --dp_mode sharded"):
        check(coldstart=0.25, eval_panel=128, dp_mode="sharded")
    for gpus in (2, 8):
        with pytest.raises(ValueError, match="--eval_coldstart cannot be combined with --gpus > 1"):
            check(gpus=gpus, coldstart=0.25, eval_panel=128)
    for bad in (0.5, "3", True):
        with pytest.raises(ValueError, match="--coldstart_donors must be an integer"):
            check(coldstart=0.25, eval_panel=128, coldstart_donors=bad)
    for bad in (-1, 65):
        with pytest.raises(ValueError, match=r"--coldstart_donors must be in \[1, 64\]"):
            check(coldstart=0.25, eval_panel=128, coldstart_donors=bad)
    for ok in (dict(), dict(coldstart=0), dict(coldstart=0, dp_mode="sharded"), dict(coldstart=0.5, eval_panel=128),
               dict(coldstart=1e-3, eval_panel=256, coldstart_donors=64), dict(coldstart=np.float32(0.25), eval_panel=128, coldstart_donors=1)):
        check(**ok)
    # the flags: refused by the command line before any data is loaded
    ap = cli.build_parser()
    off = ap.parse_args([])
    assert off.coldstart == 0 and off.coldstart_donors == 16
    on = ap.parse_args(["--eval_coldstart", "0.25", "--coldstart_donors", "8", "--eval_panel", "128"])
    assert on.coldstart == 0.25 and on.coldstart_donors == 8
    check_cold_start_options(vars(off), off.gpus)
    check_cold_start_options(vars(on), on.gpus)
    for argv, text in ((["--eval_coldstart", "0.25"], "needs --eval_panel"), (["--eval_coldstart", "0.75", "--eval_panel", "128"], "at most 0.5"),
                       (["--eval_coldstart", "0.25", "--eval_panel", "128", "--gpus", "2"], "--gpus > 1"),
                       (["--eval_coldstart", "0.25", "--synthetic", "100", "--dp_mode", "sharded"], "sharded")):
        with pytest.raises(ValueError, match=text):
            cli.main(argv + ["--datapath", "/nonexistent/"])        # (refused before load_datas could fail on the path)
    # the model's resolver: args over the values the model was built with, else off
    m = Seq2SeqAttNN.__new__(Seq2SeqAttNN)
    req = m._eval_request({"eval_panel": 128})
    assert cold_start_request(m, {}, req) is None
    assert cold_start_request(m, {"coldstart": 0.25}, req) == ColdStartRequest(0.25, 16)
    assert cold_start_request(m, {"coldstart": 0.25, "coldstart_donors": 5}, req) == ColdStartRequest(0.25, 5)
    m.coldstart, m.coldstart_donors = 0.5, 7
    assert cold_start_request(m, {}, req) == ColdStartRequest(0.5, 7) and cold_start_request(m, {"coldstart": 0}, req) is None
    with pytest.raises(ValueError, match="needs --eval_panel"):
        cold_start_request(m, {}, m._eval_request({}))
    with pytest.raises(ValueError, match="--gpus > 1"):
        cold_start_request(m, {"gpus": 2}, req)


def test_the_cold_sample_is_a_function_of_the_seed_alone():
    from tcar_amd.host.eval_passes import cold_sample
    rng = np.random.RandomState(3)
    labels = rng.randint(0, 400, 1000)
    arts = np.unique(labels)
    a = cold_sample(labels, 0.25, 2020)
    assert a.dtype == np.int64 and len(a) == round(0.25 * len(arts)) and np.array_equal(a, np.unique(a)) and np.isin(a, arts).all()
    # the order and the multiplicity of the labels, and every global random stream, are nothing to it
    np.random.seed(1)
    import random
    random.seed(1)
    np.random.random_sample(100)
    assert np.array_equal(cold_sample(labels[::-1], 0.25, 2020), a) and np.array_equal(cold_sample(arts, 0.25, 2020), a)
    state = np.random.get_state()[1].copy()
    cold_sample(labels, 0.25, 2020)
    assert np.array_equal(np.random.get_state()[1], state)          # and it moves none of them
    assert not np.array_equal(cold_sample(labels, 0.25, 2021), a)
    assert len(cold_sample(labels, 0.5, 7)) == round(0.5 * len(arts)) and len(cold_sample([5, 5, 5], 0.01, 7)) == 1
    assert len(cold_sample([], 0.25, 7)) == 0
    b = cold_sample(labels, 0.5, 2020)
    assert len(np.setdiff1d(arts, b)) >= len(b) - 1                  # at most half: the donors are at least as many as the cold rows
