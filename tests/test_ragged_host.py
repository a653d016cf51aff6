"""Host side of ragged batches (include/tcar_ragged.h): the layout host.data.pack_sessions / SessionStore.ragged_arrays produce, the
engine's refusals — raised before anything is uploaded, on engines that were never built —, the binding of the layer, its argument
errors (returned before any launch, so without a device) and the --eval_mixed flag."""
import ctypes as C
import types

import numpy as np
import pytest

import tcar_amd  # noqa: F401
from tcar_amd import _lib
from tcar_amd.host.data import PER_ROW, pack_sessions, ragged_offsets

PER_B = ("cw", "ch", "label")


def _rect(rng, b, t, label=True):
    f = {"seq": rng.randint(1, 701, (b, t)), "pm": rng.randint(1, 13, (b, t)), "pd": rng.randint(1, 32, (b, t)),
         "pw": rng.randint(1, 8, (b, t)), "ph": rng.randint(1, 25, (b, t)), "pmi": rng.randint(1, 61, (b, t)),
         "gap": rng.randint(0, 12, (b, t)), "cw": rng.randint(0, 7, b), "ch": rng.randint(0, 24, b)}
    if label:
        f["label"] = rng.randint(0, 700, b)
    return {k: v.astype(np.int32) for k, v in f.items()}


def _loop_offsets(lens):
    off, pos = [0], []
    for n in lens:
        off.append(off[-1] + int(n))
        pos += list(range(int(n)))
    return off, pos


def test_pack_sessions_keeps_list_order_and_lays_every_feed_out_as_a_block():
    rng = np.random.RandomState(5)
    feeds = [_rect(rng, 3, 4), _rect(rng, 1, 1), _rect(rng, 5, 40), _rect(rng, 2, 4)]
    feeds[0]["neg"] = rng.randint(0, 700, (3, 6)).astype(np.int32)          # negatives are dropped
    rg = pack_sessions(feeds)
    assert "neg" not in rg and rg["len"].tolist() == [4] * 3 + [1] + [40] * 5 + [4] * 2 and rg["len"].dtype == np.int32
    R = 12 + 1 + 200 + 8
    assert all(rg[k].shape == (R,) and rg[k].dtype == np.int32 for k in PER_ROW) and all(rg[k].shape == (11,) for k in PER_B)
    off, pos = ragged_offsets(rg["len"])
    want_off, want_pos = _loop_offsets(rg["len"])
    assert off.tolist() == want_off and pos.tolist() == want_pos and off.dtype == pos.dtype == np.int32
    s0 = r0 = 0
    for f in feeds:                          # the sessions of a feed are contiguous, its flat rows are its [B_g, T_g] block
        b, t = f["seq"].shape
        for k in PER_ROW:
            assert (rg[k][r0:r0 + b * t].reshape(b, t) == f[k]).all(), k
        for k in PER_B:
            assert (rg[k][s0:s0 + b] == f[k]).all(), k
        s0, r0 = s0 + b, r0 + b * t
    # every session, against a plain loop over the sessions in list order
    flat = [(f, i) for f in feeds for i in range(f["seq"].shape[0])]
    for b, (f, i) in enumerate(flat):
        assert (rg["seq"][off[b]:off[b + 1]] == f["seq"][i]).all() and rg["label"][b] == f["label"][i]
    unl = pack_sessions([{k: v for k, v in f.items() if k != "label"} for f in feeds])
    assert "label" not in unl and (unl["seq"] == rg["seq"]).all()
    with pytest.raises(ValueError, match="label"):
        pack_sessions([feeds[0], {k: v for k, v in feeds[1].items() if k != "label"}])
    with pytest.raises(ValueError):
        pack_sessions([])


def test_ragged_arrays_of_any_lengths_and_of_one_length():
    from tcar_amd.host.synth import SynthFold
    store = SynthFold(n_items=60, dim=8, n_train=40, n_test=200, seed=1, active_t=True).test
    lens = np.unique(store.in_len)
    assert len(lens) >= 3
    idx = np.concatenate([np.where(store.in_len == n)[0][:3] for n in lens[::-1]])        # longest first: not sorted by length
    for mode in ("active_t", "delta"):
        rg = store.ragged_arrays(idx, mode)
        assert rg["len"].tolist() == store.in_len[idx].tolist()
        off, _ = _loop_offsets(rg["len"])
        for b, e in enumerate(idx):          # session by session, against batch_arrays of that one example
            one = store.batch_arrays(np.array([e]), mode)
            for k in PER_ROW:
                assert (rg[k][off[b]:off[b + 1]] == one[k][0]).all(), (k, b)
            for k in PER_B + ("cmo", "cd", "cmi"):
                assert rg[k][b] == one[k][0], (k, b)
        same = np.where(store.in_len == lens[1])[0][:5]
        rg, rect = store.ragged_arrays(same, mode), store.batch_arrays(same, mode)
        assert sorted(rg) == sorted(list(rect) + ["len"])
        for k in rect:
            assert rg[k].dtype == np.int32 and (rg[k] == rect[k].reshape(-1)).all(), k
    with pytest.raises(ValueError):
        store.ragged_arrays(np.array([], dtype=np.int64))


def _never_built():
    from tcar_amd.engine import TcarEngine
    eng = TcarEngine.__new__(TcarEngine)
    eng.shard, eng.geo, eng.pin = (0, 700), types.SimpleNamespace(N=700, Npad=768), None
    return eng


def test_the_engine_refuses_a_bad_ragged_feed_before_anything_is_uploaded():
    from tcar_amd.sharded import ShardedEngine
    rng = np.random.RandomState(7)
    good = pack_sessions([_rect(rng, 2, 3), _rect(rng, 1, 7)])
    eng = _never_built()
    seq0 = good["seq"].copy()
    seq0[4] = 0
    seq_big = good["seq"].copy()
    seq_big[0] = 701
    bad = [(dict(good, len=np.array([3, 3, 0], np.int32)), IndexError, r"session length outside \[1, 40\]"),
           (dict(good, len=np.array([3, 3, 41], np.int32)), IndexError, r"session length outside \[1, 40\]"),
           (dict(good, len=np.array([3, 3, 6], np.int32)), ValueError, r"sum\(len\) = 12, but seq holds 13 rows"),
           (dict(good, gap=good["gap"][:-1]), ValueError, r"sum\(len\) = 13, but gap holds 12 rows"),
           (dict(good, seq=seq0), IndexError, r"item id outside \[1, N\]"),
           (dict(good, seq=seq_big), IndexError, r"item id outside \[1, N\]"),
           (dict(good, neg=np.zeros((3, 4), np.int32)), ValueError, "a ragged feed carries no negatives"),
           (dict(good, cw=good["cw"][:-1]), ValueError, "cw must hold one entry per session"),
           (dict(good, len=np.zeros(0, np.int32)), ValueError, "len must be")]
    for feed, exc, text in bad:
        calls = [lambda: eng.upload(feed), lambda: eng.eval_step_streamed(feed), lambda: eng.recommend(feed),
                 lambda: eng.retrieve(feed, 64), lambda: eng.recommend_two_stage(feed),
                 lambda: eng.score_candidates(feed, np.zeros((len(feed["len"]), 4), np.int32))]
        for call in calls:
            with pytest.raises(exc, match=text):
                call()
    assert eng.pin is None                              # no staging buffer was ever allocated: nothing went up
    # the rectangular-only entry points refuse a GOOD ragged feed, and so does the catalog-sharded engine
    for call in (lambda: eng.train_step(good), lambda: eng.loss_and_grads(good), lambda: eng.eval_step(good)):
        with pytest.raises(ValueError, match="takes a rectangular feed"):
            call()
    sh = ShardedEngine.__new__(ShardedEngine)
    sh.geo = eng.geo
    for call in (lambda: sh.serve_pieces(good), lambda: sh.eval_step_streamed(good), lambda: sh.recommend(good)):
        with pytest.raises(ValueError, match="catalog-sharded engine takes rectangular feeds"):
            call()
    assert eng.pin is None
    assert eng.is_ragged(good) and not eng.is_ragged(_rect(rng, 2, 3)) and eng._sessions(good) == 3


def test_the_ragged_layer_is_bound_and_the_other_layers_are_where_they_were():
    lib = _lib.load()
    assert _lib.RAGGED_SYMBOLS == ["tcar_ragged_abi_version", "tcar_gather_clip_fwd_ragged", "tcar_attn_pool_fwd_ragged",
                                   "tcar_attn_pool_fwd_slabs_ragged", "tcar_ragged_forward", "tcar_serve_step_ragged",
                                   "tcar_cand_step_ragged", "tcar_retrieve_step_ragged", "tcar_retrieve_rerank_step_ragged"]
    assert lib.tcar_ragged_abi_version() == _lib.RAGGED_ABI_VERSION == 1
    assert ("RAGGED", "tcar_ragged.h") == _lib.ABI_LAYERS[-1] and _lib.RAGGED_HEADER in _lib.HEADERS
    assert [f[0] for f in _lib.Ragged._fields_] == ["R", "off", "pos"] and C.sizeof(_lib.Ragged) == 24
    i32, vp, P = C.c_int32, C.c_void_p, C.POINTER
    assert lib.tcar_ragged_forward.argtypes == [P(_lib.Ctx), P(_lib.Batch), P(_lib.Ragged), i32, vp]
    assert lib.tcar_serve_step_ragged.argtypes == [P(_lib.Ctx), P(_lib.Batch), P(_lib.Ragged), i32, P(_lib.Serve), P(_lib.Window),
                                                   P(_lib.Quota), vp]
    assert lib.tcar_retrieve_rerank_step_ragged.argtypes == [P(_lib.Ctx), P(_lib.Batch), P(_lib.Ragged), i32, P(_lib.Retrieve),
                                                             P(_lib.Rerank), vp]


def test_argument_errors_come_back_before_any_launch():
    lib = _lib.load()
    buf = (C.c_float * 4096)()                    # host memory: never dereferenced, an accepted call would have to launch
    p = C.cast(buf, C.c_void_p).value
    d, tab, bt, ctx = _lib.Dims(700, 250, 64, 256, 64), _lib.Tables(), _lib.Batch(), _lib.Ctx()
    bt.B, bt.T = 4, 40

    def rg(R=20, off=p, pos=p):
        r = _lib.Ragged()
        r.R, r.off, r.pos = R, off, pos
        return r
    gather = lambda r, b=bt: lib.tcar_gather_clip_fwd_ragged(C.byref(d), C.byref(tab), C.byref(b), C.byref(r) if r else None, p, p, p, p, None)
    pool = lambda r, B=4: lib.tcar_attn_pool_fwd_ragged(C.byref(d), B, C.byref(r) if r else None, p, p, p, p, p, p, p, p, p, None)
    slabs = lambda r, stride=20 * 256: lib.tcar_attn_pool_fwd_slabs_ragged(C.byref(d), 4, C.byref(r) if r else None, p, p, p, 7, p, 5, stride,
                                                                           p, p, p, p, p, p, p, None)
    head = lambda r, b=bt: lib.tcar_ragged_forward(C.byref(ctx), C.byref(b), C.byref(r) if r else None, 0, None)
    t41 = _lib.Batch()
    t41.B, t41.T = 4, 41
    t0 = _lib.Batch()
    t0.B, t0.T = 4, 0
    for call in (gather, pool, slabs, head):
        assert call(None) == -1                                      # NULL rg
        assert call(rg(off=None)) == -1 and call(rg(pos=None)) == -1     # NULL off / pos
        assert call(rg(R=3)) == -1 and call(rg(R=161)) == -1           # R < B, R > 40 B
    assert gather(rg(), t41) == -1 and gather(rg(), t0) == -1 and head(rg(), t41) == -1 and head(rg(), t0) == -1      # T outside 1 .. 40
    assert slabs(rg(), 20 * 256 - 1) == -1                           # a slab shorter than R rows
    assert head(rg()) == -1                                          # an empty context (no parameters): still before any launch
    # the steps: the ragged descriptor is checked like their rectangular twins' arguments, before the head runs
    s, c, r, rr = _lib.Serve(), _lib.Cand(), _lib.Retrieve(), _lib.Rerank()
    one = rg()
    assert lib.tcar_serve_step_ragged(C.byref(ctx), C.byref(bt), None, 0, C.byref(s), None, None, None) == -1
    assert lib.tcar_cand_step_ragged(C.byref(ctx), C.byref(bt), None, 0, C.byref(c), None) == -1
    assert lib.tcar_retrieve_step_ragged(C.byref(ctx), C.byref(bt), None, 0, C.byref(r), None) == -1
    assert lib.tcar_retrieve_rerank_step_ragged(C.byref(ctx), C.byref(bt), None, 0, C.byref(r), C.byref(rr), None) == -1
    assert lib.tcar_serve_step_ragged(C.byref(ctx), C.byref(bt), C.byref(one), 0, C.byref(s), None, None, None) == -1


def test_eval_mixed_is_refused_where_it_cannot_work_and_defaults_to_off():
    from tcar_amd.host import cli
    from tcar_amd.host.model import Seq2SeqAttNN
    from tcar_amd.host.synth import SynthFold
    ap = cli.build_parser()
    assert ap.parse_args([]).eval_mixed == 0 and ap.parse_args(["--eval_mixed", "1"]).eval_mixed == 1
    check = lambda gpus=1, **values: cli.check_eval_options(values, gpus=gpus)
    with pytest.raises(ValueError, match="eval_mixed needs --eval_panel"):
        check(eval_mixed=1, eval_panel=0, dp_mode="replica")
    with pytest.raises(ValueError, match="eval_mixed.*sharded"):
        check(eval_mixed=1, dp_mode="sharded")             # (with --eval_panel the refusal of --eval_panel comes first)
    with pytest.raises(ValueError, match="eval_mixed.*gpus"):
        check(eval_mixed=1, eval_panel=256, dp_mode="replica", gpus=2)
    with pytest.raises(ValueError, match="eval_mixed.*eval_candidates"):
        check(eval_mixed=1, eval_panel=256, dp_mode="replica", gpus=1, eval_candidates=50)
    with pytest.raises(ValueError, match="eval_mixed.*eval_shortlist"):
        check(eval_mixed=1, eval_panel=256, dp_mode="replica", gpus=1, eval_candidates=0, eval_shortlist=80)
    with pytest.raises(ValueError, match="eval_mixed must be 0 or 1"):
        check(eval_mixed=2, eval_panel=256, dp_mode="replica")
    # (off, it refuses nothing: eight ranks, and the candidate and two-stage passes beside the streamed evaluation)
    for ok in ((0, 0, "sharded", 8), (0, 256, "replica", 8, 50, 80), (1, 128, "replica"), (1, 49152, "replica", 1, 0, 0)):
        check(**dict(zip(("eval_mixed", "eval_panel", "dp_mode", "gpus", "eval_candidates", "eval_shortlist"), ok)))
    # it combines with --fresh_hours and --cat_cap: their own checks pass beside it
    check(fresh_hours=2.0, cat_cap=3, eval_mixed=1, eval_panel=256, dp_mode="replica", gpus=1, eval_candidates=0, eval_shortlist=0)
    fold = SynthFold(n_items=60, dim=8, n_train=40, n_test=10, seed=1)
    for kw in (dict(eval_mixed=1), dict(eval_mixed=1, eval_panel=128, eval_candidates=20), dict(eval_mixed=1, eval_panel=128, gpus=2),
               dict(eval_mixed=1, eval_panel=128, eval_shortlist=80)):
        args = fold.model_args(batch_size=8, epoch=1, neg_num=2, hidden_size=8, time_hidden_size=4, lr=0.003, emb_stddev=0.3, stddev=0.1,
                               **kw)
        with pytest.raises(ValueError, match="eval_mixed"):
            Seq2SeqAttNN(args)


def test_packs_hold_whole_feeds_and_at_most_batch_size_sessions():
    from tcar_amd.host.model import Seq2SeqAttNN
    m = Seq2SeqAttNN.__new__(Seq2SeqAttNN)
    m.batch_size = 8
    feeds = [{"seq": np.zeros((b, t), np.int32)} for b, t in ((8, 1), (3, 2), (5, 3), (1, 4), (8, 5), (2, 6), (2, 7), (2, 8), (3, 9))]
    sizes = lambda mixed: [[f["seq"].shape for f in p] for p in m._packs(iter(feeds), mixed)]
    assert sizes(False) == [[f["seq"].shape] for f in feeds]
    assert sizes(True) == [[(8, 1)], [(3, 2), (5, 3)], [(1, 4)], [(8, 5)], [(2, 6), (2, 7), (2, 8)], [(3, 9)]]
