"""Host side of the diversity re-rank (include/tcar_mmr.h): the numpy model of tests/mmr_ref.py against a brute-force loop, what
mu = 0 means, the pool cut, repeated ids, host.metrics.content_ild_batch, the request validation of the engine and of the command
line, the ABI layer and the argument checks that answer before anything is launched — none of it needs a GPU."""
import ctypes as C
import types

import numpy as np
import pytest

import tcar_amd  # noqa: F401
from tcar_amd import _lib

from cand_ref import rank_model
from mmr_ref import MAX_POOL, brute_walk, dots_f32, pool_of, tau_greedy, walk_f32, walk_f64


def _case(rng, B, C, N, H, levels=8):
    """small exact inputs: content rows of a few 0.5s (norm 1 where four are set), scores on `levels` levels, repeats and empty slots"""
    content = np.zeros((N, H), np.float32)
    for n in range(N):
        content[n, rng.choice(H, min(4, H), replace=False)] = 0.5
    cand = rng.randint(0, N, (B, C)).astype(np.int32)
    score = (rng.randint(0, levels, (B, C)) / 8.0).astype(np.float32)
    gone = rng.rand(B, C) < 0.15
    cand[gone] = -1
    score[gone] = -np.inf
    return content, cand, score


def test_the_model_against_the_brute_force_loop():
    rng = np.random.RandomState(3)
    for B, C, N, H, k in ((3, 1, 4, 4, 1), (4, 6, 5, 8, 4), (4, 9, 30, 12, 9), (3, 20, 8, 7, 6)):
        content, cand, score = _case(rng, B, C, N, H)
        order = rank_model(score, cand)[1]
        for mu in (0.0, 0.5, 2.0):
            want = brute_walk(cand, score, content, mu, k)
            t32, s32, m32 = walk_f32(cand, score, order, content, mu, k)
            t64, s64, m64, gap = walk_f64(cand, score, order, content, mu, k)
            assert (t32 == want).all() and (t64 == want).all(), (B, C, N, H, k, mu)
            assert s32.tobytes() == s64.tobytes() and np.array_equal(m32.astype(np.float64), m64)      # every value is exact
            assert (m32[:, 0] == 0).all() and (m32 >= 0).all() and (m32 <= 1).all()
            short, m_replay, count = tau_greedy(cand, score, order, content, mu, t32)
            assert (short == 0).all() and np.array_equal(m_replay, m64) and (count == (t32 >= 0).sum(1)).all()


def test_mu_zero_is_the_head_of_the_rank_order():
    rng = np.random.RandomState(4)
    content, cand, score = _case(rng, 5, 40, 12, 16)
    score[2, 3] = np.nan
    order = rank_model(np.where(np.isnan(score), np.float32(9), score), cand)[1]       # the NaN slot sits FIRST in the order: it is skipped
    topk, sc, msim = walk_f32(cand, score, order, content, 0.0, 10, fill=-5.0)
    for b in range(5):
        head = [s for s in order[b] if s >= 0 and not np.isnan(score[b, s])][:10]
        assert topk[b, :len(head)].tolist() == cand[b, head].tolist() and (topk[b, len(head):] == -1).all()
        assert sc[b, :len(head)].tobytes() == score[b, head].tobytes() and (sc[b, len(head):] == -5.0).all()


def test_the_pool_is_cut_at_256_slots_of_the_order():
    rng = np.random.RandomState(6)
    N, H, C = 400, 8, 300
    content = np.zeros((N, H), np.float32)
    content[:, 0] = 1.0                                        # every item is a duplicate of every other
    content[N - 1] = [0, 1, 0, 0, 0, 0, 0, 0]                  # ... but one
    cand = rng.permutation(N - 1)[:C].astype(np.int32)[None, :]
    cand[0, 7] = N - 1
    score = np.linspace(5, 6, C, dtype=np.float32)[None, :].copy()
    score[0, 7] = 0.0                                          # the odd one scores lowest: rank 300, outside the pool
    order = rank_model(score, cand)[1]
    assert len(pool_of(cand[0], score[0], order[0], N)) == MAX_POOL
    topk, _, msim = walk_f32(cand, score, order, content, 100.0, 3)
    assert N - 1 not in topk[0] and (msim[0] == [0, 1, 1]).all()       # the penalty would have pulled it in at once
    score[0, 7] = 5.9                                          # inside the pool it is the second pick
    order = rank_model(score, cand)[1]
    topk, _, msim = walk_f32(cand, score, order, content, 100.0, 3)
    assert topk[0, 1] == N - 1 and (msim[0] == [0, 0, 1]).all()


def test_a_repeated_id_is_a_slot_of_its_own_and_a_perfect_duplicate_of_its_twin():
    content = np.eye(4, dtype=np.float32)
    cand = np.asarray([[2, 2, 1, 3]], np.int32)
    score = np.asarray([[4.0, 4.0, 3.5, 1.0]], np.float32)
    order = rank_model(score, cand)[1]
    assert order.tolist() == [[0, 1, 2, 3]]
    topk, sc, msim = walk_f32(cand, score, order, content, 0.0, 4)
    assert topk.tolist() == [[2, 2, 1, 3]]
    topk, sc, msim = walk_f32(cand, score, order, content, 1.0, 4)
    assert topk.tolist() == [[2, 1, 2, 3]] and msim.tolist() == [[0, 0, 1, 0]] and sc.tolist() == [[4.0, 3.5, 4.0, 1.0]]
    topk, sc, msim = walk_f32(cand, score, order, content, 8.0, 4)
    assert topk.tolist() == [[2, 1, 3, 2]] and msim.tolist() == [[0, 0, 0, 1]]
    # an all-zero content row is similar to nothing, itself included
    content[2] = 0
    topk, _, msim = walk_f32(cand, score, order, content, 8.0, 4)
    assert topk.tolist() == [[2, 2, 1, 3]] and (msim == 0).all()


def test_the_dot_of_the_model_has_the_order_the_header_states():
    rng = np.random.RandomState(8)
    for H in (1, 7, 8, 9, 250):
        X, y = rng.standard_normal((5, H)).astype(np.float32), rng.standard_normal(H).astype(np.float32)
        got = dots_f32(X, y)
        for p in range(5):
            acc = np.zeros((2, 4), np.float32)
            for c in range(H):
                acc[(c % 8) // 4, c % 4] += X[p, c] * y[c]
            h = [(acc[i, 0] + acc[i, 1]) + (acc[i, 2] + acc[i, 3]) for i in range(2)]
            assert got[p] == h[0] + h[1]
        assert np.abs(got - X.astype(np.float64) @ y.astype(np.float64)).max() <= (H + 8) * 2.0 ** -24 * np.abs(X).max() * np.abs(y).max() * H


def test_content_ild_batch():
    from tcar_amd.host.metrics import content_ild_batch
    content = np.asarray([[1, 0], [2, 0], [0, 3], [1, 1], [0, 0]], np.float32)
    topk = np.asarray([[0, 1, -1], [0, 2, -1], [0, 1, 2], [3, -1, -1], [-1, -1, -1], [0, 3, -1], [0, 4, 2]], np.int32)
    got = content_ild_batch(topk, content)
    assert got.dtype == np.float64 and got.shape == (7,)
    np.testing.assert_allclose(got[[0, 1, 2]], [0.0, 1.0, 2.0 / 3.0], atol=1e-15)
    assert np.isnan(got[3]) and np.isnan(got[4])
    np.testing.assert_allclose(got[5], 1 - np.sqrt(0.5), atol=1e-15)
    np.testing.assert_allclose(got[6], 1.0, atol=1e-15)                 # an all-zero row has cosine 0 with everything
    # against the plain double loop
    rng = np.random.RandomState(2)
    content = rng.standard_normal((30, 6))
    topk = rng.randint(-1, 30, (9, 7))
    want = []
    for row in topk:
        ids = [i for i in row if i >= 0]
        pairs = [1 - content[i] @ content[j] / np.sqrt((content[i] @ content[i]) * (content[j] @ content[j]))
                 for a, i in enumerate(ids) for b, j in enumerate(ids) if a != b]
        want.append(np.mean(pairs) if len(ids) >= 2 else np.nan)
    np.testing.assert_allclose(content_ild_batch(topk, content), want, rtol=1e-12, equal_nan=True)


def test_the_engine_validates_the_penalty_before_any_device_call():
    from tcar_amd.engine import TcarEngine
    from tcar_amd.host.model import Seq2SeqAttNN
    from tcar_amd.sharded import ShardedEngine
    eng = TcarEngine.__new__(TcarEngine)
    eng.shard, eng.geo = (0, 700), types.SimpleNamespace(N=700, Npad=768, H=8, ldh=64, ek=168)
    for bad in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf"), 1e39, "2", None.__class__, [1.0], True):
        with pytest.raises(ValueError, match="diversity must be"):
            eng.recommend_two_stage({}, k=20, shortlist=128, diversity=bad)
        with pytest.raises(ValueError, match="diversity must be"):
            eng.diversify(np.zeros((2, 30), np.int32), np.zeros((2, 30), np.float32), 20, bad)
    assert eng._diversity_request(0) == 0.0 and eng._diversity_request(np.float32(0.5)) == 0.5 and eng._diversity_request(3) == 3.0
    with pytest.raises(ValueError, match="the shortlist must hold"):           # the other rules of the request still answer first
        eng.recommend_two_stage({}, k=20, shortlist=0, diversity=1.0)
    for cand, sc, k in ((np.zeros((2, 30)), np.zeros((2, 30)), 20), (np.zeros((2, 30), np.int32), np.zeros((2, 29)), 20),
                        (np.zeros((2, 30), np.int32), np.zeros((2, 30), np.int32), 20), (np.zeros((2, 30), np.int32), np.zeros((2, 30)), 31),
                        (np.zeros((2, 30), np.int32), np.zeros((2, 30)), 65), (np.zeros((2, 1025), np.int32), np.zeros((2, 1025)), 20),
                        (np.zeros(30, np.int32), np.zeros(30), 20)):
        with pytest.raises(ValueError):
            eng.diversify(cand, sc, k, 1.0)
    sh = ShardedEngine.__new__(ShardedEngine)
    for call in (lambda: sh.shard_recommend_two_stage({}, diversity=1.0), lambda: sh.recommend_two_stage({}, diversity=0.0)):
        with pytest.raises(_lib.TcarError, match="diversity.*does not take the keyword"):
            call()
    m = Seq2SeqAttNN.__new__(Seq2SeqAttNN)
    with pytest.raises(ValueError, match="diversity re-ranks the shortlist"):
        m.recommend({}, k=5, diversity=1.0)


def test_eval_diversity_is_checked_and_refused_where_it_cannot_work():
    from tcar_amd.host import cli
    check = lambda gpus=1, **values: cli.check_eval_options(values, gpus=gpus)
    for bad in (-1.0, float("nan"), float("inf"), "1", True):
        with pytest.raises(ValueError, match="--eval_diversity must be"):
            check(eval_diversity=bad, eval_shortlist=128, eval_panel=256, dp_mode="replica")
    with pytest.raises(ValueError, match="eval_diversity needs --eval_shortlist"):
        check(eval_diversity=1.0, eval_shortlist=0, dp_mode="replica")
    with pytest.raises(ValueError, match="eval_diversity.*sharded"):
        check(eval_diversity=1.0, dp_mode="sharded")       # (with --eval_shortlist the refusal of --eval_shortlist comes first)
    for ok in ((0, 0, "sharded"), (0.0, 128, "replica"), (0.5, 65, "replica"), (3, 1024, "replica")):
        check(eval_diversity=ok[0], eval_shortlist=ok[1], eval_panel=256 if ok[1] else 0, dp_mode=ok[2])
    ap = cli.build_parser()
    assert ap.parse_args([]).eval_diversity == 0 and ap.parse_args(["--eval_diversity", "1.5"]).eval_diversity == 1.5


def test_the_mmr_layer_is_bound_behind_retrieve_and_the_other_layers_are_where_they_were():
    lib = _lib.load()
    i = _lib.ABI_LAYERS.index(("MMR", "tcar_mmr.h"))
    assert _lib.ABI_LAYERS[i - 1] == ("RETRIEVE", "tcar_retrieve.h")
    assert _lib.ABI_LAYERS[-2:] == [("RETRIEVE_SHARD", "tcar_retrieve_shard.h"), ("RAGGED", "tcar_ragged.h")]
    assert _lib.MMR_SYMBOLS == ["tcar_mmr_abi_version", "tcar_mmr_walk", "tcar_mmr_rerank_step", "tcar_mmr_rerank_step_ragged"]
    assert lib.tcar_mmr_abi_version() == _lib.MMR_ABI_VERSION == 1
    assert _lib.MMR_HEADER in _lib.HEADERS and "mmr.hip" in _lib.SOURCES
    assert [f[0] for f in _lib.Mmr._fields_] == ["mu", "msim"] and C.sizeof(_lib.Mmr) == 16
    i32, i64, f32, vp, P = C.c_int32, C.c_int64, C.c_float, C.c_void_p, C.POINTER
    assert lib.tcar_mmr_walk.argtypes == [i32, i32, i32, f32, i32, i32, vp, i64, vp, i64, vp, i64, vp, vp, vp, vp, vp]
    assert lib.tcar_mmr_rerank_step.argtypes == [P(_lib.Ctx), P(_lib.Batch), i32, P(_lib.Retrieve), P(_lib.Rerank), P(_lib.Mmr), vp]
    assert lib.tcar_mmr_rerank_step_ragged.argtypes == [P(_lib.Ctx), P(_lib.Batch), vp, i32, P(_lib.Retrieve), P(_lib.Rerank), P(_lib.Mmr), vp]
    every = [s for prefix, _ in _lib.ABI_LAYERS if prefix != "MMR" for s in getattr(_lib, _lib._name(prefix, "SYMBOLS"))]
    assert not set(_lib.MMR_SYMBOLS) & set(every)


def test_argument_errors_come_back_before_any_launch():
    lib = _lib.load()
    buf = (C.c_float * 4096)()                    # host memory: never dereferenced, an accepted call would have to launch
    p = C.cast(buf, C.c_void_p)
    names = ("B", "C", "k", "mu", "N", "H", "content", "ldc", "cand", "ld_cand", "score", "ld_score", "order", "topk", "out", "msim", "stream")
    base = dict(B=2, C=30, k=20, mu=1.0, N=50, H=8, content=p, ldc=8, cand=p, ld_cand=30, score=p, ld_score=30, order=p, topk=p, out=p,
                msim=p, stream=None)
    walk = lambda **kw: lib.tcar_mmr_walk(*[dict(base, **kw)[a] for a in names])
    for bad in (dict(C=0), dict(C=1025, ld_cand=1025, ld_score=1025), dict(k=0), dict(k=65, C=100, ld_cand=100, ld_score=100), dict(k=31),
                dict(mu=-1.0), dict(mu=float("nan")), dict(mu=float("inf")), dict(order=None), dict(topk=None), dict(content=None),
                dict(cand=None), dict(score=None), dict(B=-1), dict(N=0), dict(H=0), dict(ldc=7), dict(ld_cand=29), dict(ld_score=29),
                dict(content=C.c_void_p(p.value + 2))):
        assert walk(**bad) == -1, bad
    assert walk(B=0) == 0 and walk(B=0, order=None, topk=None) == 0
    ctx, bt, d, r, m = _lib.Ctx(), _lib.Batch(), _lib.Retrieve(), _lib.Rerank(), _lib.Mmr()
    bt.B, bt.T = 2, 3
    for f, v in dict(C=30, panel=128, panel_buf=p.value, state=p.value, state_bytes=2 * 64 * 4, ids=p.value, scores=p.value).items():
        setattr(d, f, v)
    r.k, r.cand_score, r.rank_of, r.order, r.topk, r.score = 20, p.value, p.value, p.value, p.value, p.value
    step = lambda mm: lib.tcar_mmr_rerank_step(C.byref(ctx), C.byref(bt), 0, C.byref(d), C.byref(r), mm, None)
    for mu in (-1.0, float("nan"), float("inf")):
        m.mu = mu
        assert step(C.byref(m)) == -1
    m.mu = 1.0
    assert step(None) == -1
    assert step(C.byref(m)) == -1                  # an empty context (no parameters): still before any launch
    assert lib.tcar_mmr_rerank_step_ragged(C.byref(ctx), C.byref(bt), None, 0, C.byref(d), C.byref(r), C.byref(m), None) == -1
    bt.B = 0
    assert step(C.byref(m)) == 0
