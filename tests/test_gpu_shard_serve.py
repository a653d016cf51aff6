"""Streamed evaluation and recommendation of the catalog-sharded engine (ShardedEngine.eval_step_streamed / recommend,
include/tcar_serve_shard.h) on the inputs of serve_case and the bands of test_gpu_serve;
the engines, the split and the played collectives are those of shard_case.

W engines ShardedEngine(world=W, rank=r) run in ONE process without a process group; the test plays the three collectives of
ShardExchange.serve by concatenating the ranks' buffers between the pieces.  The variables are those after two training steps (trained on
a one-rank sharded engine and loaded into the W engines, whose candidate-time planes are then stale: the first evaluation has to rebuild
them).  The merged result is held against the numpy merge (select_ref) of the W shard states bit for bit, and against the fp64 oracle of
the trained variables in the bands of test_gpu_serve."""
import copy
import io
import os
import random
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401

from dist_util import launch
from gpu_util import _need_gpu, close
from select_ref import merge_states
from serve_case import B, N, T, TOPK, reference
from serve_shapes_ref import check_band
from shard_case import PANEL, engines, play, shard_states, split, trained

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("W", [2, 3])
@pytest.mark.parametrize("scoring", ["bf16x3-mixed", "bf16x3"])
def test_sharded_streamed_evaluation_and_recommendation(scoring, W):
    _need_gpu()
    r, t = reference(), trained(scoring)
    batch, lab, s, delta = r["batch"], r["batch"]["label"], t["s"], t["delta"]
    engs = engines(scoring, W)
    subs, edges, cap = split(batch, W)
    k = TOPK
    pcs = [e.serve_pieces(sub, k, True, panel=PANEL, cap=cap, T=T) for e, sub in zip(engs, subs)]
    head_all, states, outs = play(pcs)
    assert all(not e._time_dirty for e in engs)                # every shard rebuilt its candidate-time planes
    assert states.shape == (W, W * cap, 2 * k + 4) and head_all.shape[0] == W * cap
    per_shard = shard_states(engs[0], states, k)
    rank = np.zeros(B, np.int32)
    topk = np.zeros((B, k), np.int32)
    ce = np.zeros(B, np.float32)
    scores = np.zeros((B, k), np.float32)
    for rk, (e, out) in enumerate(zip(engs, outs)):
        a, b = edges[rk], edges[rk + 1]
        assert all(o.shape[0] == b - a for o in out)
        for j in range(b - a):
            row = rk * cap + j
            want = merge_states([per_shard[w][row] for w in range(W)], k)
            assert out[1][j].cpu().numpy().tolist() == want["ids"] and len(want["ids"]) == k, (rk, j)                # (i) the list
            assert out[3][j].cpu().numpy().tobytes() == want["scores"].tobytes(), (rk, j)                           # (i) its scores
            assert int(out[0][j]) == 1 + want["count"] == 1 + sum(per_shard[w][row]["count"] for w in range(W))      # (ii)
        rank[a:b], topk[a:b], ce[a:b], scores[a:b] = (o.cpu().numpy() for o in out)
    # (iii) against the fp64 oracle of the trained variables: (a)-(g) of test_gpu_serve
    assert np.isfinite(ce).all() and np.isfinite(scores).all()
    check_band(s, delta, topk, k, name="eval")
    sl = s[np.arange(B), lab]
    others = np.arange(N)[None, :] != lab[:, None]
    lo = 1 + (s > (sl + 2 * delta)[:, None]).sum(1)
    hi = 1 + ((s > (sl - 2 * delta)[:, None]) & others).sum(1)
    assert ((lo <= rank) & (rank <= hi)).all(), (rank, lo, hi)
    close(scores, np.take_along_axis(s, topk.astype(np.int64), 1), name="scores")
    close(ce, t["ce"], name="ce vs oracle")

    # (iv) recommendation: seen items and further ids excluded, a window per session, at most 2 items of one category
    feed = {n: v for n, v in batch.items() if n not in ("label", "neg")}
    rng = np.random.RandomState(31)
    w_lo = rng.randint(0, 300, B).astype(np.int64)
    w_hi = w_lo + rng.randint(300, 700, B)
    extra = np.full((B, 3), -1, np.int32)
    extra[:, 0], extra[:, 2] = topk[:, 0], topk[:, 5]
    fsubs, _, _ = split(feed, W)
    pcs = []
    for rk, (e, sub) in enumerate(zip(engs, fsubs)):
        a, b = edges[rk], edges[rk + 1]
        pcs.append(e.serve_pieces(sub, k, False, exclude_seen=True, exclude=extra[a:b], panel=PANEL, window=(w_lo[a:b], w_hi[a:b]),
                                  max_per_category=2, cap=cap, T=T))
    _, states, outs = play(pcs)
    per_shard = shard_states(engs[0], states, k)
    keys, cat = t["keys"], t["cat"]
    seen = (batch["seq"] - 1).astype(np.int64)
    for rk, out in enumerate(outs):
        a, b = edges[rk], edges[rk + 1]
        for j in range(b - a):
            g, row = a + j, rk * cap + j
            want = merge_states([per_shard[w][row] for w in range(W)], k, cat, 2)          # the capped walk over the merged shard lists
            tk = out[1][j].cpu().numpy()
            n = len(want["ids"])
            assert tk.tolist() == want["ids"] + [-1] * (k - n), (g, tk, want["ids"])
            assert out[3][j].cpu().numpy()[:n].tobytes() == want["scores"].tobytes(), g
            ids = tk[:n]
            gone = set(seen[g].tolist()) | set(extra[g][extra[g] >= 0].tolist())
            assert not set(ids.tolist()) & gone and ((w_lo[g] <= keys[ids]) & (keys[ids] < w_hi[g])).all(), g
            assert (np.bincount(cat[ids], minlength=12) <= 2).all() and n > 0, g
            # and it is the walk over the session's eligible items, in the bands of the oracle: nothing clearly better was left out
            ok = (w_lo[g] <= keys) & (keys < w_hi[g])
            ok[list(gone)] = False
            taken = np.bincount(cat[ids], minlength=12)
            worst = s[g, ids].min() if n == k else -np.inf
            left = ok.copy()
            left[ids] = False
            assert not (left & (taken[cat] < 2) & (s[g] > worst + 4 * delta[g])).any(), g
    # (v) no buffer of the catalog's width
    assert all(not hasattr(e, "ev_logits") for e in engs)


@pytest.mark.parametrize("scoring", ["bf16x3-mixed", "bf16x3"])
def test_one_rank_without_collectives_gives_the_bits_of_the_pieces_called_by_hand(scoring):
    _need_gpu()
    r, t = reference(), trained(scoring)
    (eng,) = engines(scoring, 1)
    rank, topk, ce = eng.eval_step_streamed(r["batch"], k=TOPK, panel=PANEL)
    got = [x.cpu().numpy().copy() for x in (rank, topk, ce, eng.last_scores)]
    assert eng.xch.order == [] and not eng.xch.collective        # nothing was exchanged
    _, _, (out,) = play([eng.serve_pieces(r["batch"], TOPK, True, panel=PANEL)])
    for a, b in zip(got, out):
        assert a.tobytes() == b.cpu().numpy().tobytes()
    check_band(t["s"], t["delta"], got[1], TOPK, name="world 1")
    close(got[2], t["ce"], name="ce vs oracle, world 1")
    assert eng.default_panel() == 768 and not hasattr(eng, "ev_logits")
    info = eng.exchange_info()
    assert info["serve_collectives"] == ("serve_rows", "serve_label_scores", "serve_states")
    feed = {n: v for n, v in r["batch"].items() if n not in ("label", "neg")}
    tk, sc = eng.recommend(feed, k=TOPK, exclude_seen=False, panel=PANEL)
    assert (tk.cpu().numpy() == got[1]).all() and sc.cpu().numpy().tobytes() == got[3].tobytes()


def _worker(rank, world, port, ret, scoring):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import tcar_amd  # noqa: F401
        from tcar_amd.sharded import ShardedEngine
        r = reference()
        subs, edges, cap = split(r["batch"], world)
        eng = ShardedEngine(r["params"], r["content"], r["mw"], max_grad=2.0, group=dist.group.WORLD, scoring=scoring)
        rk, tk, ce = eng.eval_step_streamed(subs[rank], k=TOPK, panel=PANEL, cap=cap, T=T)
        torch.cuda.synchronize()
        assert eng.xch.order == ["serve_rows", "serve_label_scores", "serve_states"]
        assert eng.exchange_info()["serve_bytes"]["serve_states"] == world * world * cap * (2 * TOPK + 4) * 4
        pc = eng._serve_pc
        flat = torch.cat([pc._head_all.reshape(-1).view(torch.int32), pc._states.reshape(-1), eng.sv_lab_score[:world * cap].view(torch.int32)])
        other = [torch.zeros_like(flat) for _ in range(world)]
        dist.all_gather(other, flat)
        assert torch.equal(other[0], other[1])                 # both ranks hold the same gathered rows, label scores and states
        ret[rank] = {"rank": rk.cpu().numpy().tobytes(), "topk": tk.cpu().numpy().tobytes(), "ce": ce.cpu().numpy().tobytes(),
                     "scores": eng.last_scores.cpu().numpy().tobytes(), "states": pc._states.cpu().numpy().tobytes()}
    except Exception as e:
        import traceback
        ret[rank] = "FAIL: " + repr(e) + "\n" + traceback.format_exc()
    finally:
        dist.destroy_process_group()


def test_two_ranks_over_gloo_give_the_bits_of_the_two_engines_in_one_process():
    _need_gpu()
    from tcar_amd.sharded import ShardedEngine
    scoring, world = "bf16x3-mixed", 2
    ret = launch(_worker, world, scoring, spawned_manager=True)
    for rk in range(world):
        assert isinstance(ret.get(rk), dict), ret.get(rk)
    r = reference()
    subs, edges, cap = split(r["batch"], world)
    engs = [ShardedEngine(r["params"], r["content"], r["mw"], max_grad=2.0, scoring=scoring, world=world, rank=rk) for rk in range(world)]
    _, states, outs = play([e.serve_pieces(sub, TOPK, True, panel=PANEL, cap=cap, T=T) for e, sub in zip(engs, subs)])
    for rk in range(world):
        got = ret[rk]
        assert got["states"] == states.cpu().numpy().tobytes(), rk
        for name, o in zip(("rank", "topk", "ce", "scores"), outs[rk]):
            assert got[name] == o.cpu().numpy().tobytes(), (rk, name)


def test_test_loop_with_shard_eval_panel_reports_the_metrics_of_the_materialised_one():
    _need_gpu()
    from tcar_amd.host.model import Seq2SeqAttNN, initial_variables
    from tcar_amd.host.synth import SynthFold
    from tcar_amd.sharded import ShardedEngine
    fold = SynthFold(n_items=400, dim=32, n_train=2500, n_test=400, seed=17, active_t=True)
    tr = fold.to_dicts(fold.train, with_active=True)
    te = fold.to_dicts(fold.test, with_active=True)
    np.random.seed(3)
    init = initial_variables(400, 32, 16, 0.3, 0.1)
    args = fold.model_args(batch_size=64, epoch=1, neg_num=8, hidden_size=32, time_hidden_size=16, lr=0.003,
                           initial_variables=init, emb_stddev=0.3, stddev=0.1, scoring="bf16x3", dp_mode="sharded", shard_eval_panel=128)
    random.seed(5)
    np.random.seed(5)
    model = Seq2SeqAttNN(args)
    assert isinstance(model.engine, ShardedEngine) and model.engine.world == 1
    got = {}
    with redirect_stdout(io.StringIO()):
        model.train(None, fold.item_dict, (copy.deepcopy(tr[0]), tr[1], tr[2]), {0: [0]}, args,
                    (copy.deepcopy(te[0]), te[1], te[2]), None)
        for panel in (0, 128):
            model.test(None, (copy.deepcopy(te[0]), te[1], te[2]), dict(args, shard_eval_panel=panel))
            got[panel] = dict(model.last_metrics)
    a, b = got[0], got[128]
    assert abs(a["recall"] - b["recall"]) <= 0.002 + 1e-12, (a, b)
    assert abs(a["mrr"] - b["mrr"]) <= 1e-3 * a["mrr"] + 1.0 / 400, (a, b)
    assert abs(a["loss"] - b["loss"]) <= 1e-3 * a["loss"], (a, b)
    assert b["coverage"] > 0 and np.isfinite(b["ild"]) and np.isfinite(b["unexp"])
    idx = np.where(fold.test.in_len == 3)[0][:4]
    rec, sc = model.recommend({n: v for n, v in fold.test.batch_arrays(idx, "active_t").items() if n not in ("label", "neg")}, k=5,
                              max_per_category=2)
    assert tuple(rec.shape) == (len(idx), 5) and tuple(sc.shape) == (len(idx), 5) and len(idx) > 0
