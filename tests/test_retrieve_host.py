"""Host side of retrieval and the two-stage call (include/tcar_retrieve.h): the numpy model the GPU tests compare with against a
brute-force loop, the bindings generated from the header, the argument checks that answer before anything is launched, the engine's
request validation and the command line's rules — none of it needs a GPU."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import tcar_amd  # noqa: F401
from tcar_amd import _lib

from retrieve_ref import shortlist, shortlist_brute

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_numpy_model_against_the_brute_force_loop():
    rng = np.random.RandomState(5)
    for B, N, C_ in ((3, 1, 1), (4, 9, 4), (4, 9, 9), (5, 17, 30), (3, 40, 7)):
        x = (rng.randint(-3, 4, (B, N)) / 2.0).astype(np.float32)              # many ties
        x[0, ::3] = np.nan
        x[B - 1, : N // 2] = -0.0
        x[B - 1, N // 2:] = 0.0
        if N > 4:
            x[1, 1], x[1, 2], x[1, 3] = np.inf, -np.inf, np.nan
        excl = rng.randint(-1, N + 2, (B, 5)).astype(np.int32)                 # -1, repeats and ids past the catalog
        key = rng.randint(0, 10, N).astype(np.int32)
        lo, hi = rng.randint(0, 5, B).astype(np.int32), rng.randint(3, 11, B).astype(np.int32)
        for kw in ({}, {"excl": excl}, {"key": key, "lo": lo, "hi": hi}, {"excl": excl, "key": key, "lo": lo, "hi": hi}):
            ids, sc = shortlist(x, C_, **kw)
            ids2, sc2 = shortlist_brute(x, C_, **kw)
            assert (ids == ids2).all() and sc.tobytes() == sc2.tobytes(), (B, N, C_, sorted(kw))
            assert ids.shape == (B, C_) and ids.dtype == np.int32 and sc.dtype == np.float32
            assert (sc[ids < 0] == -np.inf).all() and not np.isnan(sc).any()
    # the sign of a zero does not order: ids alone do, and the scores keep their bits
    ids, sc = shortlist(np.asarray([[0.0, -0.0, 0.0, -0.0]], np.float32), 4)
    assert ids.tolist() == [[3, 2, 1, 0]] and np.signbit(sc[0]).tolist() == [True, False, True, False]


def test_the_retrieve_layer_is_bound_and_the_other_layers_are_where_they_were():
    lib = _lib.load()
    assert _lib.RETRIEVE_SYMBOLS == ["tcar_retrieve_abi_version", "tcar_retrieve_state_bytes", "tcar_retrieve_reset", "tcar_retrieve_panel",
                                     "tcar_retrieve_finish", "tcar_retrieve_step", "tcar_retrieve_rerank_step"]
    assert lib.tcar_retrieve_abi_version() == _lib.RETRIEVE_ABI_VERSION == 1
    assert ("RETRIEVE", "tcar_retrieve.h") in _lib.ABI_LAYERS and _lib.RETRIEVE_HEADER in _lib.HEADERS and "retrieve.hip" in _lib.SOURCES
    assert _lib.ABI_VERSION == 30 and len(_lib.SYMBOLS) == 112 and _lib.CAND_ABI_VERSION == 1 and len(_lib.CAND_SYMBOLS) == 4
    every = _lib.SYMBOLS + _lib.SERVE_SYMBOLS + _lib.WINDOW_SYMBOLS + _lib.QUOTA_SYMBOLS + _lib.SERVE_SHARD_SYMBOLS + _lib.CAND_SYMBOLS
    assert not set(_lib.RETRIEVE_SYMBOLS) & set(every)
    i32, i64, vp, P = C.c_int32, C.c_int64, C.c_void_p, C.POINTER
    assert lib.tcar_retrieve_state_bytes.restype is i64 and lib.tcar_retrieve_state_bytes.argtypes == [i32, i32]
    assert lib.tcar_retrieve_panel.argtypes == [i32, i32, i32, vp, i64, i32, vp, i32, vp, vp, vp, vp, vp]
    assert lib.tcar_retrieve_finish.argtypes == [i32, i32, vp, vp, vp, vp]
    assert lib.tcar_retrieve_step.argtypes == [P(_lib.Ctx), P(_lib.Batch), i32, P(_lib.Retrieve), vp]
    assert lib.tcar_retrieve_rerank_step.argtypes == [P(_lib.Ctx), P(_lib.Batch), i32, P(_lib.Retrieve), P(_lib.Rerank), vp]
    for B, C_ in ((1, 1), (5, 300), (512, 1024)):
        assert lib.tcar_retrieve_state_bytes(B, C_) == B * (2 * C_ + 4) * 4
    assert lib.tcar_retrieve_state_bytes(4, 0) == -1 and lib.tcar_retrieve_state_bytes(4, 1025) == -1


def test_the_mirrors_have_the_layout_the_compiler_gives_the_header(tmp_path):
    want = {"tcar_retrieve_t": (_lib.Retrieve, ["C", "panel", "panel_buf", "state", "state_bytes", "excl", "X", "ids", "scores", "window"]),
            "tcar_rerank_t": (_lib.Rerank, ["k", "cand_score", "rank_of", "order", "topk", "score"])}
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "tcar_retrieve.h"', 'int main() {']
    for c, (m, names) in want.items():
        assert [f[0] for f in m._fields_] == names
        lines.append('  printf("%%zu\\n", sizeof(%s));' % c)
        lines += ['  printf("%%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (c, f, c, f) for f in names]
    lines.append('  return 0;\n}')
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([_lib._hipcc(), "-x", "c++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = iter(subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE).stdout.decode().split("\n"))
    for c, (m, names) in want.items():
        assert int(next(got)) == C.sizeof(m), c
        for f in names:
            d = getattr(m, f)
            assert next(got).split() == [str(d.offset), str(d.size)], (c, f)


def test_argument_errors_come_back_before_any_launch():
    lib = _lib.load()
    buf = (C.c_float * 4096)()                    # host memory: never dereferenced, an accepted call would have to launch
    p = C.cast(buf, C.c_void_p)
    names = ("B", "n0", "n", "panel", "ld", "C", "excl", "X", "key", "lo", "hi", "state", "stream")
    base = dict(B=2, n0=0, n=100, panel=p, ld=128, C=7, excl=None, X=0, key=None, lo=None, hi=None, state=p, stream=None)
    fold = lambda **kw: lib.tcar_retrieve_panel(*[dict(base, **kw)[a] for a in names])
    assert fold(C=0) == -1 and fold(C=1025) == -1 and fold(B=-1) == -1
    assert fold(n=49153, ld=49156) == -1 and fold(n=-1) == -1 and fold(n0=-1) == -1 and fold(n0=2 ** 31 - 50) == -1
    assert fold(ld=126) == -1 and fold(ld=96) == -1                                        # ld % 4, ld < n
    assert fold(panel=C.c_void_p(p.value + 4)) == -1 and fold(panel=None) == -1 and fold(state=None) == -1
    assert fold(state=C.c_void_p(p.value + 2)) == -1
    assert fold(excl=p, X=0) == -1 and fold(X=-1) == -1
    assert fold(key=p) == -1 and fold(key=p, lo=p) == -1 and fold(lo=p, hi=p) == -1          # a window is all three or none
    assert fold(B=0) == 0 and fold(n=0) == 0 and fold(B=0, panel=None, state=None) == 0
    assert lib.tcar_retrieve_reset(2, 0, p, None) == -1 and lib.tcar_retrieve_reset(2, 1025, p, None) == -1
    assert lib.tcar_retrieve_reset(2, 7, None, None) == -1 and lib.tcar_retrieve_reset(0, 7, None, None) == 0
    assert lib.tcar_retrieve_finish(2, 0, p, p, p, None) == -1 and lib.tcar_retrieve_finish(2, 1025, p, p, p, None) == -1
    assert lib.tcar_retrieve_finish(2, 7, None, p, p, None) == -1 and lib.tcar_retrieve_finish(2, 7, p, None, p, None) == -1
    assert lib.tcar_retrieve_finish(0, 7, None, None, None, None) == 0

    ctx, bt, d, r = _lib.Ctx(), _lib.Batch(), _lib.Retrieve(), _lib.Rerank()
    bt.B, bt.T = 2, 3
    good = dict(C=7, panel=128, panel_buf=p.value, state=p.value, state_bytes=2 * 18 * 4, ids=p.value, scores=p.value, excl=None, X=0,
                window=None)
    step = lambda: lib.tcar_retrieve_step(C.byref(ctx), C.byref(bt), 0, C.byref(d), None)
    both = lambda: lib.tcar_retrieve_rerank_step(C.byref(ctx), C.byref(bt), 0, C.byref(d), C.byref(r), None)
    r.k, r.cand_score, r.rank_of, r.order, r.topk, r.score = 5, p.value, p.value, p.value, p.value, p.value
    for bad in (dict(C=0), dict(C=1025), dict(panel=0), dict(panel=100), dict(panel=49280), dict(panel_buf=None), dict(state=None),
                dict(ids=None), dict(state_bytes=2 * 18 * 4 - 4), dict(panel_buf=p.value + 4), dict(X=-1), dict(excl=p.value, X=0)):
        for f, v in dict(good, **bad).items():
            setattr(d, f, v)
        assert step() == -1 and both() == -1, bad
    w = _lib.Window()                              # a window descriptor without its arrays
    for f, v in dict(good, window=C.addressof(w)).items():
        setattr(d, f, v)
    assert step() == -1
    for f, v in good.items():
        setattr(d, f, v)
    assert step() == -1                            # an empty context (no parameters): still before any launch
    for bad in (dict(k=0), dict(k=65), dict(k=8), dict(cand_score=None), dict(order=None), dict(topk=None)):       # k = 8 > C = 7
        rr = dict(k=5, cand_score=p.value, order=p.value, topk=p.value)
        for f, v in dict(rr, **bad).items():
            setattr(r, f, v)
        assert both() == -1, bad
    assert lib.tcar_retrieve_step(None, C.byref(bt), 0, C.byref(d), None) == -1
    assert lib.tcar_retrieve_step(C.byref(ctx), C.byref(bt), 0, None, None) == -1
    r.k, r.cand_score, r.order, r.topk = 5, p.value, p.value, p.value
    assert lib.tcar_retrieve_rerank_step(C.byref(ctx), C.byref(bt), 0, C.byref(d), None, None) == -1
    bt.B = 0
    assert step() == 0 and both() == 0


def test_the_engine_validates_a_request_before_any_device_call():
    """TcarEngine._retrieve_request runs before the upload and the step: on an engine that was never built (no device, no workspace,
    no library handle) a refused request raises ValueError and nothing else is reached"""
    from tcar_amd.engine import TcarEngine
    from tcar_amd.sharded import ShardedEngine
    eng = TcarEngine.__new__(TcarEngine)
    eng.shard, eng.geo = (0, 700), types.SimpleNamespace(N=700, Npad=768)
    feed = {}
    refused = [(lambda: eng.retrieve(feed, 0), "the shortlist must hold 1 to 1024 items"),
               (lambda: eng.retrieve(feed, 1025), "the shortlist must hold 1 to 1024 items"),
               (lambda: eng.retrieve(feed, 12.0), "the shortlist must hold 1 to 1024 items"),
               (lambda: eng.recommend_two_stage(feed, k=20, shortlist=0), "the shortlist must hold 1 to 1024 items"),
               (lambda: eng.recommend_two_stage(feed, k=20, shortlist=1025), "the shortlist must hold 1 to 1024 items"),
               (lambda: eng.recommend_two_stage(feed, k=30, shortlist=20), "k = 30 items cannot come out of a shortlist of 20"),
               (lambda: eng.recommend_two_stage(feed, k=65, shortlist=128), "k must be in [1, 64]"),
               (lambda: eng.recommend_two_stage(feed, k=0, shortlist=128), "k must be in [1, 64]"),
               (lambda: eng.retrieve(feed, 64, window=(0, 5)), "a window compares item keys: call set_item_keys(keys) first"),
               (lambda: eng.recommend_two_stage(feed, window=(0, 5)), "a window compares item keys: call set_item_keys(keys) first"),
               (lambda: eng.retrieve(feed, 64, panel=100), "panel must be a positive multiple of 128, at most 49152"),
               (lambda: eng.recommend_two_stage(feed, panel=49280), "panel must be a positive multiple of 128, at most 49152")]
    for call, text in refused:
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text
    assert eng._retrieve_request(1024, 64, None, None, 768) == 768 and eng._retrieve_request(1, None, 128, None, 768) == 128
    eng.shard = (0, 350)
    for call in (lambda: eng.retrieve(feed, 64), lambda: eng.recommend_two_stage(feed)):
        with pytest.raises(_lib.TcarError, match="whole catalog on this engine"):
            call()
    sh = ShardedEngine.__new__(ShardedEngine)
    with pytest.raises(_lib.TcarError, match=r"retrieve\(\) needs the whole catalog on one engine"):
        sh.retrieve(feed, 64)
    with pytest.raises(_lib.TcarError, match=r"recommend_two_stage\(\) needs the whole catalog on one engine"):
        sh.recommend_two_stage(feed)


def test_eval_shortlist_is_range_checked_and_refused_where_it_cannot_work():
    from tcar_amd.host import cli
    from tcar_amd.host.model import Seq2SeqAttNN
    from tcar_amd.host.synth import SynthFold
    check = lambda gpus=1, **values: cli.check_eval_options(values, gpus=gpus)
    for bad in (1, 64, -3, 1025):
        with pytest.raises(ValueError, match=r"--eval_shortlist must be in \[65, 1024\]"):
            check(eval_shortlist=bad, eval_panel=256, dp_mode="replica")
    with pytest.raises(ValueError, match="eval_shortlist needs --eval_panel"):
        check(eval_shortlist=80, eval_panel=0, dp_mode="replica")
    with pytest.raises(ValueError, match="eval_shortlist.*sharded"):
        check(eval_shortlist=80, dp_mode="sharded")        # (with --eval_panel the refusal of --eval_panel comes first)
    with pytest.raises(ValueError, match="eval_shortlist.*cat_cap"):
        check(eval_shortlist=80, eval_panel=256, dp_mode="replica", cat_cap=3)
    for ok in ((0, 0, "sharded", 0), (0, 128, "replica", 3), (65, 128, "replica", 0), (1024, 49152, "replica", 0)):
        check(eval_shortlist=ok[0], eval_panel=ok[1], dp_mode=ok[2], cat_cap=ok[3])
    ap = cli.build_parser()
    assert ap.parse_args([]).eval_shortlist == 0 and ap.parse_args(["--eval_shortlist", "80"]).eval_shortlist == 80
    fold = SynthFold(n_items=60, dim=8, n_train=40, n_test=10, seed=1)
    for kw in (dict(eval_shortlist=80), dict(eval_shortlist=80, eval_panel=128, cat_cap=2), dict(eval_shortlist=2000, eval_panel=128)):
        args = fold.model_args(batch_size=8, epoch=1, neg_num=2, hidden_size=8, time_hidden_size=4, lr=0.003, emb_stddev=0.3, stddev=0.1,
                               **kw)
        with pytest.raises(ValueError, match="eval_shortlist"):
            Seq2SeqAttNN(args)
    m = Seq2SeqAttNN.__new__(Seq2SeqAttNN)
    with pytest.raises(ValueError, match="shortlist and max_per_category"):
        m.recommend({}, k=5, shortlist=100, max_per_category=2)
