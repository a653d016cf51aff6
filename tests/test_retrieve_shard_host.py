"""Host side of retrieval and candidate scoring over catalog shards (include/tcar_retrieve_shard.h): the numpy merge the GPU tests
compare with, the bindings generated from the header, the argument checks that answer before anything is launched, the sharded
engine's request validation and the command line's rules — none of it needs a GPU."""
import ctypes as C
import types

import numpy as np
import pytest

import tcar_amd  # noqa: F401
from tcar_amd import _lib

from retrieve_merge_ref import merge_shortlists
from retrieve_ref import shortlist, shortlist_brute


def test_the_layer_is_bound_before_the_ragged_row_and_shares_no_symbol():
    lib = _lib.load()
    assert _lib.RETRIEVE_SHARD_SYMBOLS == ["tcar_retrieve_shard_abi_version", "tcar_retrieve_merge", "tcar_retrieve_panel_live",
                                           "tcar_shard_retrieve_fold", "tcar_cand_scores_owned", "tcar_shard_cand_scores",
                                           "tcar_cand_combine", "tcar_rerank_take"]
    assert lib.tcar_retrieve_shard_abi_version() == _lib.RETRIEVE_SHARD_ABI_VERSION == 1
    assert _lib.ABI_LAYERS[-1] == ("RAGGED", "tcar_ragged.h") and _lib.ABI_LAYERS[-2] == ("RETRIEVE_SHARD", "tcar_retrieve_shard.h")
    assert _lib.RETRIEVE_SHARD_HEADER in _lib.HEADERS
    for prefix, _ in _lib.ABI_LAYERS:
        if prefix != "RETRIEVE_SHARD":
            assert not set(_lib.RETRIEVE_SHARD_SYMBOLS) & set(getattr(_lib, _lib._name(prefix, "SYMBOLS"))), prefix
    i32, i64, vp, P = C.c_int32, C.c_int64, C.c_void_p, C.POINTER
    assert lib.tcar_retrieve_merge.argtypes == [i32, i32, i32, vp, i64, vp, vp]
    assert lib.tcar_retrieve_panel_live.argtypes == lib.tcar_retrieve_panel.argtypes[:-1] + [vp, vp]
    assert lib.tcar_cand_scores_owned.argtypes == lib.tcar_cand_scores.argtypes[:-1] + [i32, vp]
    assert lib.tcar_shard_retrieve_fold.argtypes == [P(_lib.Ctx), P(_lib.Shard), P(_lib.Retrieve), vp, vp]
    assert lib.tcar_shard_cand_scores.argtypes == [P(_lib.Ctx), P(_lib.Shard), i32, vp, i64, vp, i64, vp]
    assert lib.tcar_cand_combine.argtypes == [i32, i32, i32, i32, i32, vp, i64, vp, i64, vp, i64, vp]


def test_argument_errors_come_back_before_any_launch():
    lib = _lib.load()
    buf = (C.c_float * 8192)()                    # host memory: never dereferenced, an accepted call would have to launch
    p = C.cast(buf, C.c_void_p)
    q = C.c_void_p(p.value + 4 * 4096)
    rw = 2 * 7 + 4

    def call(fn, names, base):
        return lambda **kw: fn(*[dict(base, **kw)[a] for a in names])
    merge = call(lib.tcar_retrieve_merge, ("B", "C", "S", "states", "stride", "out", "stream"),
                 dict(B=2, C=7, S=3, states=p, stride=2 * rw, out=q, stream=None))
    assert merge(S=0) == -1 and merge(S=65) == -1 and merge(C=0) == -1 and merge(C=1025) == -1 and merge(B=-1) == -1
    assert merge(stride=2 * rw - 1) == -1                                                    # a short stride
    assert merge(out=None) == -1 and merge(states=None) == -1 and merge(out=C.c_void_p(q.value + 2)) == -1
    assert merge(out=C.c_void_p(p.value + 4 * rw)) == -1                                     # out inside the inputs
    assert merge(B=0) == 0 and merge(B=0, states=None, out=None) == 0
    assert merge(S=1, stride=0, out=p) == -1                                                 # one state merged onto itself

    live = call(lib.tcar_retrieve_panel_live, ("B", "n0", "n", "panel", "ld", "C", "excl", "X", "key", "lo", "hi", "state", "live", "stream"),
                dict(B=2, n0=0, n=100, panel=p, ld=128, C=7, excl=None, X=0, key=None, lo=None, hi=None, state=q, live=q, stream=None))
    assert live(C=0) == -1 and live(C=1025) == -1 and live(n=49153, ld=49156) == -1 and live(ld=126) == -1 and live(state=None) == -1
    assert live(key=p) == -1 and live(excl=p, X=0) == -1 and live(panel=C.c_void_p(p.value + 4)) == -1
    assert live(B=0) == 0 and live(n=0) == 0

    owned = call(lib.tcar_cand_scores_owned,
                 ("B", "C", "N", "K", "att", "ld_att", "E", "ldE", "a_hi", "a_lo", "a_inner", "e_hi", "e_lo", "e_inner", "nsplit", "cand",
                  "ld_cand", "out", "ld_out", "id0", "stream"),
                 dict(B=2, C=7, N=300, K=100, att=None, ld_att=0, E=None, ldE=0, a_hi=p, a_lo=p, a_inner=128, e_hi=p, e_lo=p, e_inner=128,
                      nsplit=3, cand=p, ld_cand=7, out=q, ld_out=7, id0=256, stream=None))
    assert owned(id0=-1) == -1 and owned(id0=2 ** 31 - 300) == -1 and owned(C=0) == -1 and owned(C=1025) == -1 and owned(N=0) == -1
    assert owned(K=98) == -1 and owned(nsplit=2) == -1 and owned(a_lo=None) == -1 and owned(ld_out=6) == -1 and owned(out=None) == -1
    assert owned(B=0) == 0

    comb = call(lib.tcar_cand_combine, ("B", "C", "S", "rps", "N", "cand", "ldc", "parts", "stride", "out", "ldo", "stream"),
                dict(B=2, C=7, S=3, rps=128, N=300, cand=p, ldc=7, parts=p, stride=14, out=q, ldo=7, stream=None))
    assert comb(S=0) == -1 and comb(S=65) == -1 and comb(C=0) == -1 and comb(C=1025) == -1 and comb(stride=13) == -1
    assert comb(out=None) == -1 and comb(parts=None) == -1 and comb(cand=None) == -1 and comb(rps=0) == -1 and comb(N=0) == -1
    assert comb(ldc=6) == -1 and comb(ldo=6) == -1 and comb(out=C.c_void_p(p.value + 8)) == -1
    assert comb(B=0) == 0 and comb(B=0, out=None) == 0

    ctx, sh, d = _lib.Ctx(), _lib.Shard(), _lib.Retrieve()
    good = dict(C=7, panel=128, panel_buf=p.value, state=q.value, state_bytes=4 * rw * 4, excl=None, X=0, window=None)
    fold = lambda: lib.tcar_shard_retrieve_fold(C.byref(ctx), C.byref(sh), C.byref(d), None, None)
    for bad in (dict(C=0), dict(C=1025), dict(panel=0), dict(panel=100), dict(panel_buf=None), dict(state=None), dict(X=-1), {}):
        for f, v in dict(good, **bad).items():                  # ({}: an empty shard context, still before any launch)
            setattr(d, f, v)
        assert fold() == -1, bad
    assert lib.tcar_shard_retrieve_fold(C.byref(ctx), C.byref(sh), None, None, None) == -1
    assert lib.tcar_shard_retrieve_fold(None, C.byref(sh), C.byref(d), None, None) == -1
    part = lambda **kw: lib.tcar_shard_cand_scores(C.byref(ctx), C.byref(sh), *[dict(dict(C=7, cand=p, ldc=7, part=q, ldp=7, stream=None), **kw)[a]
                                                                                for a in ("C", "cand", "ldc", "part", "ldp", "stream")])
    assert part() == -1 and part(C=0) == -1 and part(C=1025) == -1 and part(ldc=6) == -1 and part(ldp=6) == -1 and part(cand=None) == -1
    assert lib.tcar_shard_cand_scores(None, None, 7, p, 7, q, 7, None) == -1


def test_the_merge_of_any_column_partition_is_the_shortlist_of_the_whole_matrix():
    rng = np.random.RandomState(9)
    for B, N, C_ in ((3, 1, 1), (4, 9, 4), (4, 30, 9), (5, 17, 30), (3, 40, 7)):
        x = (rng.randint(-3, 4, (B, N)) / 2.0).astype(np.float32)              # many ties
        x[0, ::3] = np.nan
        x[B - 1, : N // 2] = -0.0
        x[B - 1, N // 2:] = 0.0
        if N > 4:
            x[1, 1], x[1, 2] = np.inf, -np.inf
        excl = rng.randint(-1, N + 2, (B, 5)).astype(np.int32)
        key = rng.randint(0, 10, N).astype(np.int32)
        lo, hi = rng.randint(0, 5, B).astype(np.int32), rng.randint(3, 11, B).astype(np.int32)
        for kw in ({}, {"excl": excl, "key": key, "lo": lo, "hi": hi}):
            want = shortlist(x, C_, **kw)
            brute = shortlist_brute(x, C_, **kw)
            assert (want[0] == brute[0]).all() and want[1].tobytes() == brute[1].tobytes()
            for S in (1, 2, 3, 5):
                cuts = sorted(rng.randint(0, N + 1, S - 1).tolist())            # empty pieces included
                edges = [0] + cuts + [N]
                parts = []
                for a, b in zip(edges, edges[1:]):
                    # a piece's own shortlist over GLOBAL ids: the other columns are not there (NaN is never listed)
                    piece = np.full_like(x, np.nan)
                    piece[:, a:b] = x[:, a:b]
                    parts.append(shortlist(piece, C_, **kw))
                for order in (parts, parts[::-1]):
                    ids, sc = merge_shortlists(order, C_)
                    assert (ids == want[0]).all() and sc.tobytes() == want[1].tobytes(), (B, N, C_, S, cuts, sorted(kw))
                    assert ids.dtype == np.int32 and sc.dtype == np.float32


def test_the_sharded_engine_validates_a_request_before_any_device_call():
    """the three collective calls run the single-engine request checks (TcarEngine._retrieve_request / _cand_request, the shard's
    padded rows as the panel bound) before any upload or collective: on an engine that was never built (no device, no workspace, no
    exchange) a refused request raises the single-engine message and nothing else is reached"""
    from tcar_amd.sharded import ShardedEngine
    sh = ShardedEngine.__new__(ShardedEngine)
    sh.geo, sh.nl = types.SimpleNamespace(N=700, Npad=768), 350
    feed = {"seq": np.ones((3, 2), np.int32)}
    refused = [(lambda: sh.shard_retrieve(feed, 0), "the shortlist must hold 1 to 1024 items"),
               (lambda: sh.shard_retrieve(feed, 1025), "the shortlist must hold 1 to 1024 items"),
               (lambda: sh.shard_retrieve(None, 12.0, cap=4, T=2), "the shortlist must hold 1 to 1024 items"),
               (lambda: sh.shard_recommend_two_stage(feed, k=20, shortlist=1025), "the shortlist must hold 1 to 1024 items"),
               (lambda: sh.shard_recommend_two_stage(feed, k=30, shortlist=20), "k = 30 items cannot come out of a shortlist of 20"),
               (lambda: sh.shard_recommend_two_stage(feed, k=65, shortlist=128), "k must be in [1, 64]"),
               (lambda: sh.shard_recommend_two_stage(None, k=0, shortlist=128, cap=4, T=2), "k must be in [1, 64]"),
               (lambda: sh.shard_retrieve(feed, 64, window=(0, 5)), "a window compares item keys: call set_item_keys(keys) first"),
               (lambda: sh.shard_recommend_two_stage(feed, window=(0, 5)), "a window compares item keys: call set_item_keys(keys) first"),
               (lambda: sh.shard_retrieve(feed, 64, panel=100), "panel must be a positive multiple of 128, at most 49152"),
               (lambda: sh.retrieve_pieces(feed, 64, panel=49280), "panel must be a positive multiple of 128, at most 49152"),
               (lambda: sh.shard_score_candidates(feed, np.zeros((2, 4), np.int32)), "candidates must be [B, C] with B = 3 sessions"),
               (lambda: sh.shard_score_candidates(feed, np.zeros((3, 1025), np.int32)), "C must be in [1, 1024]"),
               (lambda: sh.shard_score_candidates(feed, np.zeros((3, 4))), "candidates must be an integer array"),
               (lambda: sh.shard_score_candidates(feed, np.zeros((3, 4), np.int32), np.zeros((3, 5), np.int32)),
                "clicked must have the shape of candidates, [3, 4]"),
               (lambda: sh.cand_pieces(None, None, cap=4, T=2), "a rank without sessions needs the step's list length: C must be in [1, 1024]"),
               (lambda: sh.cand_pieces(None, None, cap=4, T=2, C=1025),
                "a rank without sessions needs the step's list length: C must be in [1, 1024]")]
    for call, text in refused:
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text
    ragged = {"seq": np.ones(5, np.int32), "len": np.array([2, 3], np.int32)}
    for call in (lambda: sh.shard_retrieve(ragged, 64), lambda: sh.shard_recommend_two_stage(ragged),
                 lambda: sh.shard_score_candidates(ragged, np.zeros((2, 4), np.int32))):
        with pytest.raises(ValueError, match="catalog-sharded engine takes rectangular feeds"):
            call()
    # the single-engine names keep refusing
    for call, text in ((lambda: sh.retrieve(feed, 64), r"retrieve\(\) needs the whole catalog on one engine"),
                       (lambda: sh.recommend_two_stage(feed), r"recommend_two_stage\(\) needs the whole catalog on one engine"),
                       (lambda: sh.score_candidates(feed, np.zeros((3, 4), np.int32)), "candidate scoring needs the whole catalog")):
        with pytest.raises(_lib.TcarError, match=text):
            call()
    assert ShardedEngine.RETRIEVE_COLLECTIVES == ("serve_rows", "retrieve_states", "retrieve_shortlists", "cand_parts")
    assert ShardedEngine.CAND_COLLECTIVES == ("serve_rows", "cand_lists", "cand_parts")


def test_shard_eval_shortlist_is_range_checked_and_refused_where_it_cannot_work():
    from tcar_amd.host import cli
    from tcar_amd.host.model import Seq2SeqAttNN
    from tcar_amd.host.synth import SynthFold
    check = lambda gpus=1, **values: cli.check_eval_options(values, gpus=gpus)
    for bad in (1, 64, -3, 1025):
        with pytest.raises(ValueError, match=r"--shard_eval_shortlist must be in \[65, 1024\]"):
            check(shard_eval_shortlist=bad, shard_eval_panel=256, dp_mode="sharded")
    with pytest.raises(ValueError, match="shard_eval_shortlist needs --shard_eval_panel"):
        check(shard_eval_shortlist=80, shard_eval_panel=0, dp_mode="sharded")
    with pytest.raises(ValueError, match="shard_eval_shortlist.*needs --dp_mode sharded"):
        check(shard_eval_shortlist=80, dp_mode="replica")  # (with --shard_eval_panel the refusal of --shard_eval_panel comes first)
    for ok in ((0, 0, "sharded"), (0, 0, "replica"), (0, 256, "sharded"), (65, 128, "sharded"), (1024, 49152, "sharded")):
        check(shard_eval_shortlist=ok[0], shard_eval_panel=ok[1], dp_mode=ok[2])
    ap = cli.build_parser()
    assert ap.parse_args([]).shard_eval_shortlist == 0 and ap.parse_args(["--shard_eval_shortlist", "80"]).shard_eval_shortlist == 80
    # the single-engine options keep refusing the sharded mode
    with pytest.raises(ValueError, match="eval_shortlist.*sharded"):
        check(eval_shortlist=80, dp_mode="sharded")
    with pytest.raises(ValueError, match="eval_candidates.*sharded"):
        check(eval_candidates=16, dp_mode="sharded")
    fold = SynthFold(n_items=60, dim=8, n_train=40, n_test=10, seed=1)
    for kw in (dict(shard_eval_shortlist=80), dict(shard_eval_shortlist=80, shard_eval_panel=128),
               dict(shard_eval_shortlist=80, dp_mode="sharded"), dict(shard_eval_shortlist=2000, shard_eval_panel=128, dp_mode="sharded")):
        args = fold.model_args(batch_size=8, epoch=1, neg_num=2, hidden_size=8, time_hidden_size=4, lr=0.003, emb_stddev=0.3, stddev=0.1,
                               **kw)
        with pytest.raises(ValueError, match="shard_eval"):
            Seq2SeqAttNN(args)
