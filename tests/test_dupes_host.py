"""Host side of the duplicate audit (include/tcar_dupes.h): the ABI layer, the argument checks of every entry point, which answer
before anything is launched, the model of tests/dupes_ref.py in fp32 against fp64 on exact rows, the groups of
host.metrics.duplicate_groups, the request validation of the engine and of the model class, and the command-line flag — none of it
needs a GPU."""
import ctypes as C
import types

import numpy as np
import pytest

import tcar_amd  # noqa: F401
from tcar_amd import _lib

from dupes_ref import audit_f64, audit_from_sims
from similar_case import exact_content
from similar_ref import sims_f32


def test_the_dupes_layer_is_bound_behind_similar_and_the_other_layers_are_where_they_were():
    lib = _lib.load()
    layers = _lib.ABI_LAYERS
    i = layers.index(("DUPES", "tcar_dupes.h"))
    assert layers[i - 1] == ("SIMILAR", "tcar_similar.h") and layers[i - 2] == ("MMR", "tcar_mmr.h")
    assert layers[i + 1:] == [("RETRIEVE_SHARD", "tcar_retrieve_shard.h"), ("RAGGED", "tcar_ragged.h")]
    assert layers[layers.index(("QUOTA", "tcar_quota.h")) + 1] == ("SECTIONS", "tcar_sections.h")
    assert layers[layers.index(("CATALOG", "tcar_catalog.h")) + 1] == ("CATALOG_SHARD", "tcar_catalog_shard.h")
    assert _lib.ABI_VERSION == 30 and len(_lib.SYMBOLS) == 112 and len(_lib.Ctx._fields_) == 104
    assert _lib.SIMILAR_SYMBOLS == ["tcar_similar_abi_version", "tcar_sim_queries", "tcar_sim_panel", "tcar_similar_step"]
    assert _lib.DUPES_SYMBOLS == ["tcar_dupes_abi_version", "tcar_dup_rnorm", "tcar_dup_reset", "tcar_dup_tiles", "tcar_dup_finish",
                                  "tcar_dupes_step"]
    assert lib.tcar_dupes_abi_version() == _lib.DUPES_ABI_VERSION == 1
    assert _lib.DUPES_HEADER in _lib.HEADERS and "dupes.hip" in _lib.SOURCES          # both enter the build id,
    assert any(h.endswith("sim_tile.h") for h in _lib.HEADERS)                         # and so does the tile both kernels share
    assert [f[0] for f in _lib.Dupes._fields_] == ["t", "stripe", "key", "lo", "hi", "r", "count", "best", "partner", "partner_sim"]
    assert C.sizeof(_lib.Dupes) == 64 and _lib.Dupes.t.size == 4 and _lib.Dupes.key.offset == 8 and _lib.Dupes.r.offset == 24
    i32, i64, f32, vp, P = C.c_int32, C.c_int64, C.c_float, C.c_void_p, C.POINTER
    assert lib.tcar_dup_rnorm.argtypes == [i32, i32, vp, i64, vp, vp]
    assert lib.tcar_dup_reset.argtypes == [i32, vp, vp, vp]
    assert lib.tcar_dup_tiles.argtypes == [i32, i32, vp, i64, vp, i32, i32, f32, vp, i32, i32, vp, vp, vp]
    assert lib.tcar_dup_finish.argtypes == [i32, vp, vp, vp, vp]
    assert lib.tcar_dupes_step.argtypes == [P(_lib.Ctx), P(_lib.Dupes), vp]
    every = [s for prefix, _ in layers if prefix != "DUPES" for s in getattr(_lib, _lib._name(prefix, "SYMBOLS"))]
    assert not set(_lib.DUPES_SYMBOLS) & set(every)


def test_argument_errors_come_back_before_any_launch():
    lib = _lib.load()
    buf = (C.c_float * 4096)()                    # host memory: never dereferenced, an accepted call would have to launch
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 2)
    off4 = C.c_void_p(p.value + 4)
    nan = float("nan")
    # ---- tcar_dup_rnorm
    names = ("N", "H", "content", "ldc", "r", "stream")
    base = dict(N=130, H=8, content=p, ldc=8, r=p, stream=None)
    rnorm = lambda **kw: lib.tcar_dup_rnorm(*[dict(base, **kw)[a] for a in names])              # noqa: E731
    for bad in (dict(N=0), dict(N=-1), dict(H=0), dict(H=-2), dict(content=None), dict(content=odd), dict(ldc=7), dict(r=None),
                dict(r=odd), dict(N=2 ** 31 - 1, ldc=2 ** 40)):
        assert rnorm(**bad) == -1, bad
    # ---- tcar_dup_reset
    reset = lambda N=130, count=p, best=p: lib.tcar_dup_reset(N, count, best, None)            # noqa: E731
    for bad in (dict(N=0), dict(N=-5), dict(count=None), dict(count=odd), dict(best=None), dict(best=odd), dict(best=off4)):
        assert reset(**bad) == -1, bad
    # ---- tcar_dup_tiles: N = 130 is three row blocks
    names = ("N", "H", "content", "ldc", "r", "b0", "b1", "t", "key", "lo", "hi", "count", "best", "stream")
    base = dict(N=130, H=8, content=p, ldc=8, r=p, b0=1, b1=1, t=0.9, key=None, lo=0, hi=0, count=p, best=p, stream=None)
    tiles = lambda **kw: lib.tcar_dup_tiles(*[dict(base, **kw)[a] for a in names])              # noqa: E731
    for bad in (dict(N=0), dict(H=0), dict(content=None), dict(content=odd), dict(ldc=7), dict(r=None), dict(r=odd), dict(count=None),
                dict(count=odd), dict(best=None), dict(best=odd), dict(best=off4), dict(b0=-1), dict(b0=2, b1=1), dict(b1=4),
                dict(b0=4, b1=4), dict(t=0.0), dict(t=-0.5), dict(t=1.0000001), dict(t=nan), dict(t=float("inf")),
                dict(lo=0, hi=5), dict(lo=-3, hi=0), dict(key=odd, lo=0, hi=5), dict(N=2 ** 31 - 1, ldc=2 ** 40)):
        assert tiles(**bad) == -1, bad
    # b0 == b1 launches nothing: the whole range of good values, a window with its keys, a table that is not 16-byte aligned
    for ok in (dict(), dict(b0=0, b1=0), dict(b0=3, b1=3), dict(t=1.0), dict(t=1e-30), dict(key=p, lo=5, hi=2), dict(key=p, lo=0, hi=0),
               dict(content=off4, ldc=9), dict(N=1, b0=1), dict(N=1, H=1, ldc=1, b0=0, b1=0)):
        assert tiles(**ok) == 0, ok
    # ---- tcar_dup_finish
    finish = lambda N=130, best=p, partner=p, psim=p: lib.tcar_dup_finish(N, best, partner, psim, None)     # noqa: E731
    for bad in (dict(N=0), dict(best=None), dict(best=off4), dict(partner=None), dict(partner=odd), dict(psim=None), dict(psim=odd)):
        assert finish(**bad) == -1, bad
    # ---- tcar_dupes_step
    ctx, d = _lib.Ctx(), _lib.Dupes()
    ctx.d.n_items, ctx.d.H, ctx.d.ldh, ctx.d.ldt = 130, 8, 64, 64
    ctx.E = p.value
    d.t, d.stripe = 0.9, 2
    d.r = d.count = d.best = d.partner = d.partner_sim = p.value
    step = lambda cc=ctx, dd=d: lib.tcar_dupes_step(C.byref(cc) if cc is not None else None,    # noqa: E731
                                                     C.byref(dd) if dd is not None else None, None)

    def broken(obj, **kw):
        cp = type(obj)()
        C.memmove(C.byref(cp), C.byref(obj), C.sizeof(obj))
        for f, v in kw.items():
            setattr(cp, f, v)
        return cp
    assert step(cc=None) == -1 and step(dd=None) == -1
    for kw in (dict(t=0.0), dict(t=1.5), dict(t=nan), dict(stripe=0), dict(stripe=-1), dict(lo=0, hi=7), dict(key=odd.value, hi=7),
               dict(r=None), dict(r=odd.value), dict(count=None), dict(best=None), dict(best=off4.value), dict(partner=None),
               dict(partner_sim=None), dict(partner_sim=odd.value)):
        assert step(dd=broken(d, **kw)) == -1, kw
    assert step(cc=broken(ctx, E=None)) == -1
    for dims in (dict(n_items=0), dict(H=0), dict(ldh=7)):
        cc = broken(ctx)
        for f, v in dims.items():
            setattr(cc.d, f, v)
        assert step(cc=cc) == -1, dims


def test_the_model_in_fp32_agrees_with_fp64_on_exact_rows():
    """similar_case.exact_content: every cosine is in {0, 1/4, 1/2, 3/4, 1}, so fp32 and fp64 must flag the same pairs at thresholds
    that ARE such values; equal rows tie and the larger id wins"""
    rng = np.random.RandomState(3)
    for N, H in ((40, 8), (90, 33), (150, 250)):
        content = exact_content(rng, N, H)
        content[N - 1] = content[5]                                                     # at least one verbatim pair
        S = sims_f32(content, content)
        assert set(np.unique(S).tolist()) <= {0.0, 0.25, 0.5, 0.75, 1.0} and S.dtype == np.float32
        keys = rng.randint(0, 100, N)
        for member in (None, (keys >= 30) & (keys < 80)):
            for t in (0.5, 0.75, 1.0):
                got, want = audit_from_sims(S, t, member), audit_f64(content, t, member)
                assert got[0].dtype == got[1].dtype == np.int32 and got[2].dtype == np.float32
                assert (got[0] == want[0]).all() and (got[1] == want[1]).all() and (got[2] == want[2]).all(), (N, H, t)
                count, partner, sim = got
                assert count[0] == 0 and partner[0] == -1                                # the all-zero row is never flagged
                assert ((partner >= 0) == (count > 0)).all() and (sim[count == 0] == 0).all() and (sim[count > 0] >= t).all()
                if member is not None:
                    assert not count[~member].any() and member[partner[partner >= 0]].all()
                for i in np.flatnonzero(count > 0):                                       # the partner by brute force: (sim, id) descending
                    ok = [j for j in range(N) if j != i and (member is None or (member[i] and member[j])) and S[i, j] >= t]
                    assert len(ok) == count[i] and partner[i] == max(ok, key=lambda j: (S[i, j], j))
        count, partner, _ = audit_from_sims(S, 1.0)
        assert count[5] >= 1 and partner[5] == N - 1 and partner[N - 1] == max(j for j in range(N - 1) if S[N - 1, j] == 1.0)
    # NaN is never at or above a threshold, and changes nothing else
    S = np.asarray([[1, .9, np.nan], [.9, 1, .95], [np.nan, .95, 1]], np.float32)
    count, partner, sim = audit_from_sims(S, 0.9)
    assert count.tolist() == [1, 2, 1] and partner.tolist() == [1, 2, 1] and sim.tolist() == [np.float32(.9), np.float32(.95), np.float32(.95)]


def test_duplicate_groups():
    from tcar_amd.host.metrics import duplicate_groups
    assert duplicate_groups([-1] * 6) == [] and duplicate_groups([]) == []
    assert duplicate_groups([1, 0, -1, -1]) == [[0, 1]]                                  # a mutual pair
    assert duplicate_groups([-1, 2, 3, 4, 3, -1]) == [[1, 2, 3, 4]]                      # a chain that ends in a mutual pair
    assert duplicate_groups([5, 5, 5, -1, 5, 4]) == [[0, 1, 2, 4, 5]]                    # a star around 5
    assert duplicate_groups([-1, 7, 9, -1, -1, -1, -1, 1, -1, 2]) == [[1, 7], [2, 9]]    # ordered by their first id
    assert duplicate_groups(np.asarray([3, -1, -1, -1], np.int32)) == [[0, 3]]           # an edge seen from one side only
    got = duplicate_groups(np.asarray([9, 0, 1, 2, 3, 6, 5, -1, -1, 8]))
    assert got == [[0, 1, 2, 3, 4, 8, 9], [5, 6]] and all(isinstance(i, int) for g in got for i in g)


def _stub():
    from tcar_amd.engine import TcarEngine
    eng = TcarEngine.__new__(TcarEngine)
    eng.shard, eng.geo = (0, 700), types.SimpleNamespace(N=700, Npad=768, H=8, ldh=64, ek=168)
    return eng


def test_the_engine_validates_the_request_before_any_device_call():
    from tcar_amd.host.model import Seq2SeqAttNN
    from tcar_amd.sharded import ShardedEngine
    eng = _stub()
    for kw, text in ((dict(threshold=0), "threshold must be"), (dict(threshold=0.0), "threshold must be"),
                     (dict(threshold=-0.5), "threshold must be"), (dict(threshold=1.01), "threshold must be"),
                     (dict(threshold=float("nan")), "threshold must be"), (dict(threshold=True), "threshold must be"),
                     (dict(threshold="0.9"), "threshold must be"), (dict(threshold=None), "threshold must be"),
                     (dict(threshold=[0.9]), "threshold must be"), (dict(threshold=1e-60), "threshold must be"),
                     (dict(stripe=0), "stripe must be"), (dict(stripe=-2), "stripe must be"), (dict(stripe=1.0), "stripe must be"),
                     (dict(stripe=True), "stripe must be"), (dict(window=(0, 5)), "call set_item_keys")):
        with pytest.raises(ValueError, match=text):
            eng.find_duplicates(**kw)
    eng._item_keys = object()
    for window in ((0,), 5, (0, 1, 2), (np.zeros(3, np.int64), np.zeros(3, np.int64)), (0.5, 3), (True, 3), ("a", "b")):
        with pytest.raises(ValueError, match="window = "):
            eng.find_duplicates(window=window)
    # what a good request becomes: the threshold as the fp32 the kernel compares with, bounds clipped to int32, the default stripe
    t, bounds, stripe = eng._dupes_request(0.98, None, None)
    assert t == float(np.float32(0.98)) and bounds is None and stripe == 11              # 700 items are 11 row blocks: one launch
    assert eng._dupes_request(1, (np.int64(3), np.asarray(2 ** 40)), 4) == (1.0, (3, 2 ** 31 - 1), 4)
    assert eng._dupes_request(np.float32(0.5), (-2 ** 40, 7), np.int64(50)) == (0.5, (-2 ** 31, 7), 11)
    eng.geo.N = 2 ** 20                                                                  # 16,384 row blocks: 16 of them are 2^18 tiles
    assert eng._dupes_request(0.9, None, None)[2] == 16
    eng.geo.N = 2 ** 26
    assert eng._dupes_request(0.9, None, None)[2] == 1
    # engines that do not hold the whole catalog refuse, after the request itself was found good
    eng.geo.N, eng.shard = 700, (0, 350)
    with pytest.raises(_lib.TcarError, match="whole catalog"):
        eng.find_duplicates()
    with pytest.raises(ValueError, match="threshold must be"):
        eng.find_duplicates(threshold=2)
    sh = ShardedEngine.__new__(ShardedEngine)
    with pytest.raises(_lib.TcarError, match="find_duplicates.*whole catalog"):
        sh.find_duplicates(0.9)
    m = Seq2SeqAttNN.__new__(Seq2SeqAttNN)
    m.engine = sh
    with pytest.raises(_lib.TcarError, match="whole catalog"):
        m.duplicate_articles(0.9)
    with pytest.raises(_lib.TcarError, match="whole catalog"):
        m.duplicate_articles(0.9, window=(0, 60))


def test_audit_duplicates_is_refused_where_it_cannot_work_before_data_loads(capsys):
    from tcar_amd.host import cli
    ap = cli.build_parser()
    assert ap.parse_args([]).audit_duplicates == 0 and ap.parse_args(["--audit_duplicates", "0.95"]).audit_duplicates == 0.95
    assert "audit_duplicates" not in [o.name for o in cli.EVAL_OPTIONS]                  # it is no evaluation option
    for bad in (-0.1, 1.5, float("nan"), True, "0.9"):
        with pytest.raises(ValueError, match=r"--audit_duplicates must be a cosine threshold in \(0, 1\]"):
            cli.check_audit_option(bad)
    for ok in ((0, "sharded", 8), (0.9, "replica", 1), (1.0, "replica", 0), (np.float32(0.5), "replica", 1)):
        cli.check_audit_option(*ok)
    with pytest.raises(ValueError, match="audit_duplicates.*sharded"):
        cli.check_audit_option(0.9, "sharded", 1)
    with pytest.raises(ValueError, match="audit_duplicates.*--gpus > 1"):
        cli.check_audit_option(0.9, "replica", 2)
    # through main(): the refusal comes before the fold is built
    base = ["--synthetic", "300", "--synthetic_train", "200", "--synthetic_test", "50", "--audit_duplicates", "0.98"]
    for more, text in ((["--dp_mode", "sharded"], "sharded"), (["--gpus", "2"], "--gpus > 1"), (["--audit_duplicates", "1.5"], "threshold")):
        with pytest.raises(ValueError, match=text):
            cli.main(base + more)
    assert "load the datasets" not in capsys.readouterr().out
