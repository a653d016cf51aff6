"""Host side of candidate-list scoring (include/tcar_cand.h): the bindings generated from the header, the argument checks that answer
before anything is launched, the numpy model the GPU tests compare with (against hand-worked cases and a brute-force pair loop),
host.metrics.impression_metrics, the command line's rules and the engine's validator — none of it needs a GPU."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import tcar_amd  # noqa: F401
from tcar_amd import _lib

from cand_ref import auc2_brute, rank_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = -np.inf


def test_the_cand_layer_is_bound_and_the_other_layers_are_where_they_were():
    lib = _lib.load()
    assert _lib.CAND_SYMBOLS == ["tcar_cand_abi_version", "tcar_cand_scores", "tcar_cand_rank", "tcar_cand_step"]
    assert lib.tcar_cand_abi_version() == _lib.CAND_ABI_VERSION == 1
    assert ("CAND", "tcar_cand.h") in _lib.ABI_LAYERS and _lib.CAND_HEADER in _lib.HEADERS and "cand.hip" in _lib.SOURCES
    assert _lib.ABI_VERSION == 30 and len(_lib.SYMBOLS) == 112 and len(_lib.Ctx._fields_) == 104 and len(_lib.Shard._fields_) == 25
    assert (_lib.SERVE_ABI_VERSION, _lib.WINDOW_ABI_VERSION, _lib.QUOTA_ABI_VERSION, _lib.SERVE_SHARD_ABI_VERSION) == (1, 1, 1, 1)
    assert (len(_lib.SERVE_SYMBOLS), len(_lib.WINDOW_SYMBOLS), len(_lib.QUOTA_SYMBOLS)) == (6, 3, 3)
    every = _lib.SYMBOLS + _lib.SERVE_SYMBOLS + _lib.WINDOW_SYMBOLS + _lib.QUOTA_SYMBOLS + _lib.SERVE_SHARD_SYMBOLS
    assert not set(_lib.CAND_SYMBOLS) & set(every)
    i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
    assert lib.tcar_cand_scores.argtypes == [i32, i32, i32, i32, vp, i64, vp, i64, vp, vp, i64, vp, vp, i64, i32, vp, i64, vp, i64, vp]
    assert lib.tcar_cand_rank.argtypes == [i32, i32, vp, i64, vp, i64, vp, i64, vp, vp, vp, vp, vp]
    assert lib.tcar_cand_step.argtypes == [C.POINTER(_lib.Ctx), C.POINTER(_lib.Batch), i32, C.POINTER(_lib.Cand), vp]


def test_cand_mirror_has_the_layout_the_compiler_gives_the_header(tmp_path):
    m = _lib.Cand
    assert [f[0] for f in m._fields_] == ["C", "cand", "ld_cand", "clicked", "score", "rank_of", "order", "counts", "metrics"]
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "tcar_cand.h"', 'int main() {', '  printf("%zu\\n", sizeof(tcar_cand_t));']
    lines += ['  printf("%%zu %%zu\\n", offsetof(tcar_cand_t, %s), sizeof(((tcar_cand_t*)0)->%s));' % (f[0], f[0]) for f in m._fields_]
    lines.append('  return 0;\n}')
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([_lib._hipcc(), "-x", "c++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = iter(subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE).stdout.decode().split("\n"))
    assert int(next(got)) == C.sizeof(m)
    for f in m._fields_:
        d = getattr(m, f[0])
        assert next(got).split() == [str(d.offset), str(d.size)], f[0]


def test_argument_errors_come_back_before_any_launch():
    lib = _lib.load()
    buf = (C.c_float * 4096)()                    # host memory: never dereferenced, an accepted call would have to launch
    p = C.cast(buf, C.c_void_p)
    names = ("B", "C", "N", "K", "att", "ld_att", "E", "ldE", "a_hi", "a_lo", "a_inner", "e_hi", "e_lo", "e_inner", "nsplit", "cand",
             "ld_cand", "out", "ld_out", "stream")
    f32 = dict(B=2, C=7, N=300, K=128, att=p, ld_att=128, E=p, ldE=128, a_hi=None, a_lo=None, a_inner=0, e_hi=None, e_lo=None, e_inner=0,
               nsplit=1, cand=p, ld_cand=7, out=p, ld_out=7, stream=None)
    planes = dict(f32, att=None, E=None, ld_att=0, ldE=0, a_hi=p, a_lo=p, e_hi=p, e_lo=p, a_inner=128, e_inner=128, nsplit=3)
    scores = lambda base, **kw: lib.tcar_cand_scores(*[dict(base, **kw)[a] for a in names])
    for base in (f32, planes):
        assert scores(base, C=0) == -1 and scores(base, C=1025, ld_cand=1025, ld_out=1025) == -1
        assert scores(base, K=126) == -1 and scores(base, K=0) == -1          # K % 4
        assert scores(base, ld_cand=6) == -1 and scores(base, ld_out=6) == -1
        assert scores(base, out=None) == -1 and scores(base, cand=None) == -1
        assert scores(base, N=0) == -1
        assert scores(base, B=0) == 0 and scores(base, B=0, out=None, cand=None) == 0
    assert scores(f32, att=C.c_void_p(p.value + 4)) == -1 and scores(f32, E=C.c_void_p(p.value + 8)) == -1      # misaligned fp32 operands
    assert scores(f32, att=None) == -1 and scores(f32, ld_att=126) == -1 and scores(f32, ldE=64) == -1
    assert scores(planes, nsplit=2) == -1 and scores(planes, nsplit=0) == -1
    assert scores(planes, e_hi=None) == -1 and scores(planes, a_lo=None) == -1 and scores(planes, e_lo=None) == -1
    assert scores(planes, a_inner=100) == -1 and scores(planes, e_inner=96) == -1              # inner % 32, inner < K

    rnames = ("B", "C", "score", "ld_score", "cand", "ld_cand", "clicked", "ld_clicked", "rank_of", "order", "counts", "metrics", "stream")
    rbase = dict(B=2, C=7, score=p, ld_score=7, cand=p, ld_cand=7, clicked=p, ld_clicked=7, rank_of=p, order=p, counts=p, metrics=p,
                 stream=None)
    rank = lambda **kw: lib.tcar_cand_rank(*[dict(rbase, **kw)[a] for a in rnames])
    assert rank(C=0) == -1 and rank(C=1025, ld_score=1025, ld_cand=1025, ld_clicked=1025) == -1
    assert rank(ld_score=6) == -1 and rank(ld_cand=6) == -1 and rank(ld_clicked=6) == -1
    assert rank(clicked=None, metrics=None) == -1 and rank(clicked=None, counts=None) == -1      # counts / metrics without clicked
    assert rank(score=None) == -1 and rank(cand=None) == -1
    assert rank(B=0) == 0 and rank(B=0, score=None, cand=None) == 0

    ctx, bt, d = _lib.Ctx(), _lib.Batch(), _lib.Cand()
    bt.B, bt.T = 2, 3
    d.C, d.cand, d.ld_cand, d.score = 7, p.value, 7, p.value
    step = lambda: lib.tcar_cand_step(C.byref(ctx), C.byref(bt), 0, C.byref(d), None)
    for bad in (0, 1025):
        d.C = bad
        assert step() == -1, bad
    d.C, d.ld_cand = 7, 6
    assert step() == -1
    d.ld_cand, d.score = 7, None
    assert step() == -1
    d.score, d.counts = p.value, p.value          # counts without clicked
    assert step() == -1
    d.counts = None
    assert step() == -1                           # an empty context (no parameters): still before any launch
    assert lib.tcar_cand_step(None, C.byref(bt), 0, C.byref(d), None) == -1
    assert lib.tcar_cand_step(C.byref(ctx), C.byref(bt), 0, None, None) == -1
    bt.B = 0
    assert step() == 0


HAND = [
    # (name, score, cand, clicked) -> rank_of, order, counts, metrics
    ("a two-slot tie goes to the larger id", [1.0, 1.0], [3, 7], [1, 0], [2, 1], [1, 0], (1, 1, 1), (0.5, 1 / np.log2(3), 1 / np.log2(3))),
    ("repeats of one id keep their slot order", [2.0, 2.0, 5.0], [4, 4, 1], [0, 1, 0], [2, 3, 1], [2, 0, 1], (1, 2, 1), (1 / 3, 0.5, 0.5)),
    ("an all-empty row", [NINF, NINF], [-1, -1], [1, 0], [0, 0], [-1, -1], (0, 0, 0), (0, 0, 0)),
    ("no positive", [1.0, 2.0], [1, 2], [0, 0], [2, 1], [1, 0], (0, 2, 0), (0, 0, 0)),
    ("no negative", [1.0, 2.0], [1, 2], [1, 1], [2, 1], [1, 0], (2, 0, 0), (0.75, 1.0, 1.0)),
    ("an empty slot by id and one by score", [3.0, 9.0, NINF, 1.0], [5, -1, 6, 2], [0, 1, 1, 1], [1, 0, 0, 2], [0, 3, -1, -1], (1, 1, 0),
     (0.5, 1 / np.log2(3), 1 / np.log2(3))),
]


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_the_numpy_model_on_hand_worked_cases(case):
    _, score, cand, clicked, rank_of, order, counts, metrics = case
    score, cand, clicked = np.asarray([score], np.float32), np.asarray([cand], np.int32), np.asarray([clicked], np.int32)
    r, o, c, m = rank_model(score, cand, clicked)
    assert r[0].tolist() == rank_of and o[0].tolist() == order and tuple(c[0].tolist()) == counts
    np.testing.assert_allclose(m[0], metrics, rtol=1e-12, atol=0)
    r2, o2, c2, m2 = rank_model(score, cand)                       # without clicked: the same order, no counts
    assert (r2 == r).all() and (o2 == o).all() and c2 is None and m2 is None


def _random_lists(seed, B, C):
    rng = np.random.RandomState(seed)
    score = (rng.randint(0, 8, (B, C)) / 4.0 - 1.0).astype(np.float32)
    cand = rng.randint(0, 40, (B, C)).astype(np.int32)
    empty = rng.rand(B, C) < 0.15
    cand[empty], score[empty] = -1, NINF
    return score, cand, (rng.rand(B, C) < 0.3).astype(np.int32)


def test_the_numpy_model_against_the_brute_force_pair_loop_and_as_a_permutation():
    for seed, (B, C) in enumerate(((4, 1), (4, 2), (5, 33), (3, 200))):
        score, cand, clicked = _random_lists(seed, B, C)
        rank_of, order, counts, metrics = rank_model(score, cand, clicked)
        live = (cand >= 0) & (score != NINF)
        assert (counts[:, 2] == auc2_brute(score, cand, clicked)).all()
        assert (counts[:, 0] == (live & (clicked != 0)).sum(1)).all() and (counts[:, 1] == (live & (clicked == 0)).sum(1)).all()
        for b in range(B):
            n = int(live[b].sum())
            assert sorted(rank_of[b][live[b]].tolist()) == list(range(1, n + 1)) and (rank_of[b][~live[b]] == 0).all()
            assert (order[b, n:] == -1).all() and (rank_of[b][order[b, :n]] == np.arange(1, n + 1)).all()
            s, i = score[b][order[b, :n]], cand[b][order[b, :n]]
            assert ((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & ((i[:-1] > i[1:]) | ((i[:-1] == i[1:]) & (order[b, :n - 1] < order[b, 1:n]))))).all()
        assert ((0 <= metrics) & (metrics <= 1)).all()


def test_impression_metrics_divide_the_counts_and_drop_sessions_without_both_classes():
    from tcar_amd.host import metrics as M
    rows = [rank_model(np.asarray([c[1]], np.float32), np.asarray([c[2]], np.int32), np.asarray([c[3]], np.int32)) for c in HAND]
    counts, metrics = np.concatenate([r[2] for r in rows]), np.concatenate([r[3] for r in rows])
    auc, mrr, n5, n10 = M.impression_metrics(counts, metrics.astype(np.float32))
    assert auc.dtype == np.float64 and auc.shape == (len(HAND),)
    np.testing.assert_array_equal(np.isnan(auc), [False, False, True, True, True, False])
    np.testing.assert_allclose(auc[[0, 1, 5]], [0.5, 0.25, 0.0])
    np.testing.assert_allclose(mrr, metrics[:, 0], rtol=1e-6)
    np.testing.assert_allclose(n5, metrics[:, 1], rtol=1e-6)
    np.testing.assert_allclose(n10, metrics[:, 2], rtol=1e-6)
    mean = M.impression_means(counts, metrics)
    assert mean["sessions"] == 3
    np.testing.assert_allclose([mean["auc"], mean["mrr"]], [0.25, (0.5 + 1 / 3 + 0.5) / 3])
    assert np.isnan(M.impression_means(counts[2:5], metrics[2:5])["auc"])


def test_eval_candidates_is_range_checked_and_refused_with_the_catalog_sharded_mode():
    from tcar_amd.host import cli
    from tcar_amd.host.model import Seq2SeqAttNN
    from tcar_amd.host.synth import SynthFold
    check = lambda gpus=1, **values: cli.check_eval_options(values, gpus=gpus)
    for bad in (1, -3, 1025):
        with pytest.raises(ValueError, match=r"--eval_candidates must be in \[2, 1024\]"):
            check(eval_candidates=bad, dp_mode="replica")
    with pytest.raises(ValueError, match="eval_candidates.*sharded"):
        check(eval_candidates=16, dp_mode="sharded")
    for ok in ((0, "sharded"), (0, "replica"), (2, "replica"), (1024, "replica")):
        check(eval_candidates=ok[0], dp_mode=ok[1])
    ap = cli.build_parser()
    assert ap.parse_args([]).eval_candidates == 0 and ap.parse_args(["--eval_candidates", "16"]).eval_candidates == 16
    fold = SynthFold(n_items=60, dim=8, n_train=40, n_test=10, seed=1)
    args = fold.model_args(batch_size=8, epoch=1, neg_num=2, hidden_size=8, time_hidden_size=4, lr=0.003, emb_stddev=0.3, stddev=0.1,
                           eval_candidates=16, dp_mode="sharded")
    with pytest.raises(ValueError, match="eval_candidates"):
        Seq2SeqAttNN(args)


def test_the_sampled_lists_hold_the_label_first_and_never_again():
    from tcar_amd.host.model import Seq2SeqAttNN
    m = Seq2SeqAttNN.__new__(Seq2SeqAttNN)
    m.candidate_n = 6                              # a catalog of five items
    lab = np.asarray([0, 4, 2, 2], np.int32)
    cand, clicked = m._label_among_sampled(lab, 64, np.random.RandomState(2))
    assert cand.shape == clicked.shape == (4, 64) and cand.dtype == np.int32
    assert (cand[:, 0] == lab).all() and (cand[:, 1:] != lab[:, None]).all() and cand.min() == 0 and cand.max() == 4
    assert (clicked[:, 0] == 1).all() and not clicked[:, 1:].any()
    assert all(set(cand[b, 1:].tolist()) == set(range(5)) - {int(lab[b])} for b in range(4))        # every other item is reachable


def test_the_engine_validates_a_request_before_any_launch():
    """TcarEngine._cand_request runs before the upload and the step; a sharded engine refuses at once (no engine is ever built)"""
    import torch
    from tcar_amd.engine import TcarEngine
    from tcar_amd.sharded import ShardedEngine
    ok = np.zeros((4, 5), np.int32)
    refused = [(dict(candidates=np.zeros((4, 0), np.int32)), "C must be in [1, 1024]"),
               (dict(candidates=np.zeros((4, 1025), np.int32)), "C must be in [1, 1024]"),
               (dict(candidates=np.zeros((3, 5), np.int32)), "candidates must be [B, C] with B = 4 sessions"),
               (dict(candidates=np.zeros(5, np.int32)), "candidates must be [B, C] with B = 4 sessions"),
               (dict(candidates=np.zeros((4, 5), np.float32)), "candidates must be an integer array"),
               (dict(candidates=ok, clicked=np.zeros((4, 5), np.float64)), "clicked must be an integer array"),
               (dict(candidates=ok, clicked=np.zeros((4, 4), np.int32)), "clicked must have the shape of candidates, [4, 5]")]
    for kw, text in refused:
        with pytest.raises(ValueError) as e:
            TcarEngine._cand_request(4, kw["candidates"], kw.get("clicked"))
        assert str(e.value) == text, kw
    cand, clk = TcarEngine._cand_request(2, torch.tensor([[3, -9, 2 ** 40], [0, 1, 2]]), [[5, 0, 0], [0, 0, 1]])
    assert cand.dtype == np.int32 and cand.tolist() == [[3, -1, -1], [0, 1, 2]] and clk.tolist() == [[1, 0, 0], [0, 0, 1]]
    assert TcarEngine._cand_request(4, ok, None)[1] is None
    eng = TcarEngine.__new__(TcarEngine)
    eng.shard, eng.geo = (0, 350), types.SimpleNamespace(N=700)
    with pytest.raises(_lib.TcarError, match="whole catalog on one engine"):
        eng.score_candidates({}, ok)
    with pytest.raises(_lib.TcarError, match="whole catalog on one engine"):
        ShardedEngine.__new__(ShardedEngine).score_candidates({}, ok)
