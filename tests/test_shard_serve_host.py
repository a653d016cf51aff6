"""Host side of the catalog-sharded streamed selection (include/tcar_serve_shard.h): the numpy model of the state merge (merging the
per-shard states IS the whole-catalog state), the bindings generated from the header, the argument checks, which answer before anything
is launched, and the trainer's option — none of it needs a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tcar_amd  # noqa: F401
from tcar_amd import _lib

from select_ref import capped_walk, finish, fold_state, merge_states, pack_states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOTYPE = r"^((?:const )?\w+\*?) (tcar_\w+)\(([^)]*)\)\s*;"


def _random_case(rng):
    N = int(rng.choice([1, 3, 7, 40, 200]))
    k = int(rng.choice([1, 5, 20, 64]))
    x = rng.randint(-3, 4, size=N).astype(np.float32) * np.float32(0.5)         # heavy ties: 7 distinct scores
    cat = rng.randint(0, 4, size=N).astype(np.int32)
    S = int(rng.randint(1, 9))
    cuts = np.sort(rng.randint(0, N + 1, size=S - 1))                            # repeated cuts and cuts at 0 / N: empty shards
    edges = [0] + cuts.tolist() + [N]
    label = int(rng.randint(0, N))
    pool = rng.rand(N) < rng.choice([0.0, 0.3, 1.0])                             # partial eligibility; 0.0: the label alone
    excl = rng.choice(N, size=int(rng.randint(0, min(N, 4) + 1)), replace=False).tolist()
    cap = int(rng.choice([1, 2, 5])) if rng.rand() < 0.6 else None
    return N, k, x, cat, edges, label, pool, excl, cap


def test_merging_the_shard_states_gives_the_state_of_the_whole_catalog():
    rng = np.random.RandomState(11)
    seen_empty = seen_short = seen_capped = 0
    for _ in range(400):
        N, k, x, cat, edges, label, pool, excl, cap = _random_case(rng)
        ids = np.arange(N)
        kw = dict(label=label, lab_score=x[label], excl=excl, cat=cat, cap=cap)
        whole = fold_state(ids, x, k, pool=pool, **kw)
        parts = [fold_state(ids[a:b], x[a:b], k, pool=pool[a:b], **kw) for a, b in zip(edges[:-1], edges[1:])]
        seen_empty += any(a == b for a, b in zip(edges[:-1], edges[1:]))
        seen_short += any(len(p["ids"]) < k for p in parts)
        seen_capped += cap is not None and cap < k
        got = merge_states(parts, k, cat, cap)
        assert got["ids"] == whole["ids"] and got["scores"].tobytes() == whole["scores"].tobytes()
        assert got["count"] == whole["count"] and got["m"] == whole["m"]
        assert abs(got["s"] - whole["s"]) <= 1e-12 * whole["s"]                  # the sum: fp64, up to the order of its terms
        # and the model is the definition: the walk over the eligible items of the whole row
        ok = (pool | (ids == label)) & ~np.isin(ids, excl)
        assert whole["ids"] == capped_walk(x, cat if cap else np.arange(N), k, cap or 1, eligible=ok)
        tk, rank, ce = finish(got, k, x[label])
        assert tk[:len(whole["ids"])] == whole["ids"] and set(tk[len(whole["ids"]):]) <= {-1}
        assert rank == 1 + int(((x > x[label]) & (pool | (ids == label)) & (ids != label)).sum())
    assert seen_empty > 20 and seen_short > 20 and seen_capped > 20


def test_an_empty_state_adds_nothing_and_no_nan():
    k = 5
    empty = fold_state(np.zeros(0, np.int64), np.zeros(0, np.float32), k)
    assert empty == {"ids": [], "scores": empty["scores"], "count": 0, "m": -np.inf, "s": 0.0}
    one = fold_state(np.array([3, 9]), np.array([1.5, -2.0], np.float32), k)
    for order in ([empty, one], [one, empty], [empty, one, empty]):
        got = merge_states(order, k)
        assert got["ids"] == [3, 9] and got["m"] == 1.5 and got["s"] == one["s"] and not np.isnan(got["s"])
    none = merge_states([empty, empty], k)
    assert none["ids"] == [] and none["m"] == -np.inf and none["s"] == 0.0
    words = pack_states([none, one], k)
    assert words.shape == (2, 2 * k + 4) and (words[0, k:2 * k] == -1).all() and (words[0, :k].view(np.float32) == -np.inf).all()
    assert words[1, k:k + 2].tolist() == [3, 9] and words[1, 2 * k] == 0


def test_the_serve_shard_header_is_parsed_and_bound():
    with open(os.path.join(ROOT, "include", "tcar_serve_shard.h")) as f:
        header = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    lib = _lib.load()
    assert lib.tcar_serve_shard_abi_version() == _lib.SERVE_SHARD_ABI_VERSION == 1
    assert _lib.SERVE_SHARD_HEADER in _lib.HEADERS                  # the header enters the build id
    protos = re.findall(PROTOTYPE, header, flags=re.M)
    assert [name for _, name, _ in protos] == _lib.SERVE_SHARD_SYMBOLS == ["tcar_serve_shard_abi_version", "tcar_select_merge",
                                                                            "tcar_shard_serve_begin", "tcar_shard_serve_fold"]
    assert not set(_lib.SERVE_SHARD_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.SERVE_SYMBOLS) | set(_lib.WINDOW_SYMBOLS) | set(_lib.QUOTA_SYMBOLS))
    i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
    assert lib.tcar_select_merge.argtypes == [i32, i32, i32, vp, i64, vp, vp, i32, vp] and lib.tcar_select_merge.restype is C.c_int
    assert lib.tcar_shard_serve_begin.argtypes == [C.POINTER(_lib.Ctx), C.POINTER(_lib.Shard), i32, vp, vp, vp]
    assert lib.tcar_shard_serve_fold.argtypes == [C.POINTER(_lib.Ctx), C.POINTER(_lib.Shard), vp, vp, C.POINTER(_lib.Serve),
                                                  C.POINTER(_lib.Window), C.POINTER(_lib.Quota), vp]
    # everything new lives in tcar_serve_shard.h: the other headers' numbers are where they were
    assert _lib.ABI_VERSION == 30 and _lib.SERVE_ABI_VERSION == 1 and _lib.WINDOW_ABI_VERSION == 1 and _lib.QUOTA_ABI_VERSION == 1
    assert len(_lib.SYMBOLS) == 112 and len(_lib.SERVE_SYMBOLS) == 6 and len(_lib.WINDOW_SYMBOLS) == 3 and len(_lib.QUOTA_SYMBOLS) == 3


def test_merge_argument_errors_come_back_before_any_launch():
    lib = _lib.load()
    buf = (C.c_float * 65536)()                   # host memory: never dereferenced, an accepted call would have to launch
    p = C.cast(buf, C.c_void_p)
    q = C.c_void_p(p.value + 4 * 32768)
    B, k = 2, 20
    rows = B * (2 * k + 4)
    names = ("B", "k", "S", "states", "stride", "out", "cat", "cap", "stream")
    base = dict(B=B, k=k, S=3, states=p, stride=rows, out=q, cat=None, cap=0, stream=None)
    merge = lambda **kw: lib.tcar_select_merge(*[dict(base, **kw)[a] for a in names])
    assert merge(S=0) == -1 and merge(S=65) == -1 and merge(S=-1) == -1
    assert merge(k=65) == -1 and merge(k=0) == -1 and merge(B=-1) == -1
    assert merge(cap=2) == -1                                      # a cap with no table
    assert merge(cat=p, cap=0) == -1 and merge(cat=p, cap=-1) == -1        # a table with no cap
    assert merge(states=None) == -1 and merge(out=None) == -1
    assert merge(stride=rows - 1) == -1                            # the shards' rows would overlap
    assert merge(out=p) == -1 and merge(out=C.c_void_p(p.value + 4 * (2 * rows + 8))) == -1      # out inside the inputs
    assert merge(B=0, S=0) == -1 and merge(B=0, cap=2) == -1       # (an argument error is one at B == 0 too)
    assert merge(B=0) == 0 and merge(B=0, states=None, out=None) == 0 and merge(B=0, cat=p, cap=3) == 0

    ctx, sh, s = _lib.Ctx(), _lib.Shard(), _lib.Serve()
    s.k, s.panel, s.panel_buf, s.state, s.state_bytes = k, 256, p.value, p.value, 65536 * 4
    fold = lambda: lib.tcar_shard_serve_fold(C.byref(ctx), C.byref(sh), None, None, C.byref(s), None, None, None)
    for bad in (100, 0, -128, 49152 + 128):
        s.panel = bad
        assert fold() == -1, bad
    s.panel = 256
    s.k = 65
    assert fold() == -1
    s.k = k
    assert fold() == -1                                            # an empty context / descriptor: still before any launch
    assert lib.tcar_shard_serve_fold(C.byref(ctx), C.byref(sh), p, None, C.byref(s), None, None, None) == -1       # label without its score
    assert lib.tcar_shard_serve_fold(C.byref(ctx), C.byref(sh), None, None, None, None, None, None) == -1
    assert lib.tcar_shard_serve_begin(C.byref(ctx), C.byref(sh), 0, None, None, None) == -1
    assert lib.tcar_shard_serve_begin(None, C.byref(sh), 0, None, None, None) == -1


def test_shard_eval_panel_is_validated_like_its_neighbours():
    from tcar_amd.host import cli
    from tcar_amd.host.model import Seq2SeqAttNN
    from tcar_amd.host.synth import SynthFold
    check = lambda gpus=1, **values: cli.check_eval_options(values, gpus=gpus)
    for bad in (-128, 100, 49152 + 128):
        with pytest.raises(ValueError, match="shard_eval_panel"):
            check(shard_eval_panel=bad, dp_mode="sharded")
    with pytest.raises(ValueError, match="sharded"):
        check(shard_eval_panel=128, dp_mode="replica")
    check(shard_eval_panel=0, dp_mode="replica")
    check(shard_eval_panel=0, dp_mode="sharded")
    check(shard_eval_panel=128, dp_mode="sharded")
    check(shard_eval_panel=49152, dp_mode="sharded")
    assert cli.build_parser().parse_args([]).shard_eval_panel == 0
    a = cli.build_parser().parse_args(["--shard_eval_panel", "256", "--dp_mode", "sharded"])
    assert a.shard_eval_panel == 256 and a.eval_panel == 0
    # the refusals of the single-engine options under sharded stay what they were
    with pytest.raises(ValueError, match="sharded"):
        check(eval_panel=128, dp_mode="sharded")
    with pytest.raises(ValueError, match="sharded"):
        check(fresh_hours=48, eval_panel=128, dp_mode="sharded")
    with pytest.raises(ValueError, match="sharded"):
        check(cat_cap=2, eval_panel=128, dp_mode="sharded")
    fold = SynthFold(n_items=60, dim=8, n_train=40, n_test=10, seed=1)
    small = dict(batch_size=8, epoch=1, neg_num=2, hidden_size=8, time_hidden_size=4, lr=0.003, emb_stddev=0.3, stddev=0.1)
    with pytest.raises(ValueError, match="sharded"):
        Seq2SeqAttNN(fold.model_args(shard_eval_panel=128, **small))
    with pytest.raises(ValueError, match="shard_eval_panel"):
        Seq2SeqAttNN(fold.model_args(shard_eval_panel=100, dp_mode="sharded", **small))
