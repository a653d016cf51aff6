"""Retrieval, candidate scoring and the two-stage call of the catalog-sharded engine (ShardedEngine.shard_retrieve /
shard_recommend_two_stage / shard_score_candidates, include/tcar_retrieve_shard.h) on the inputs of serve_case and the helpers and
split sizes of shard_case: W engines ShardedEngine(world=W, rank=r) in ONE process without a process group, the collectives of
ShardExchange.retrieve / .candidates played by hand (all-gather = concatenation in rank order, all-to-all = every rank takes its own
rows of every rank's buffer), the variables those after two training steps.

The merged shortlist is held against the numpy merge (retrieve_merge_ref) of the W shard states bit for bit, the combined exact scores
against the owners' parts bit for bit, and both against the fp64 oracle of the trained variables in the bands of
test_gpu_retrieve_serve: its coarse band (serve_case.beta_of_operands, `_beta` here) is taken as it is, over the operands read back
from the W engines, with the logits gate delta_b of the TRAINED variables' oracle in the place of the untrained one's.

No bit equality is asserted between different W or against TcarEngine: a rank's session forward runs at its local batch size, and
the projections change their split-K form with the row count, so attout may differ in the last bit."""
import ctypes as C
import io
import os
import random
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401

from cand_ref import rank_model
from dist_util import launch
from gpu_util import _kb32_index, _need_gpu, _np, close
from retrieve_merge_ref import merge_shortlists
from serve_case import B, N, T, TOPK, _feed, reference
from serve_case import beta_of_operands as _beta
from serve_shapes_ref import check_band
from shard_case import PANEL, engines, play_candidates, play_retrieve, split, trained

pytestmark = pytest.mark.gpu

CS = (64, 200, 1024)
METRIC_RTOL = 1e-4           # >= C 2^-24 at C = 1024: the bound of an fp32 sum of C positive terms (test_gpu_cand_rank)


def finished(eng, state, C_):
    """a state [rows, 2C+4] read back through tcar_retrieve_finish -> numpy (ids, scores)"""
    rows = state.shape[0]
    st = state.contiguous()
    ids = torch.empty(rows, C_, dtype=torch.int32, device="cuda")
    sc = torch.empty(rows, C_, device="cuda")
    assert eng.lib.tcar_retrieve_finish(rows, C_, C.c_void_p(st.data_ptr()), C.c_void_p(ids.data_ptr()), C.c_void_p(sc.data_ptr()), None) == 0
    torch.cuda.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy()


def operands(engs, edges):
    """the operands the engines scored, read back: A = the local sessions' fp32 attout rows in batch order, E = hi + lo of every
    shard's planes in catalog order (as the `mixed` fixture of test_gpu_retrieve_serve reads them)"""
    A = np.concatenate([e.attout[:edges[r + 1] - edges[r]].cpu().numpy().astype(np.float64) for r, e in enumerate(engs)])
    E = []
    for e in engs:
        idx = torch.tensor(_kb32_index(e.e16h.shape[0], e.geo.ek)[:e.nl], device=e.dev)
        E.append((e.e16h.flatten()[idx].double() + e.e16l.flatten()[idx].double()).cpu().numpy())
    return {"A": A, "E": np.concatenate(E)}


def band(engs, edges, t):
    """the coarse band of test_gpu_retrieve_serve (`_beta`) over the read-back operands, its logits gate that of the trained variables' oracle"""
    return _beta(operands(engs, edges)) - reference()["delta"][:, None] + t["delta"][:, None]


def gather_local(per_rank, edges, cap):
    """the ranks' [cap, x] results -> [B, x] in batch order (numpy)"""
    return np.concatenate([a[:edges[r + 1] - edges[r]] for r, a in enumerate(per_rank)])


@pytest.mark.parametrize("W", [2, 3])
@pytest.mark.parametrize("scoring", ["bf16x3-mixed", "bf16x3"])
def test_sharded_retrieval_merges_exactly_and_holds_the_oracles_band(scoring, W):
    _need_gpu()
    t = trained(scoring)
    s = t["s"]
    engs = engines(scoring, W)
    fsubs, edges, cap = split(_feed(), W)
    seen = reference()["batch"]["seq"].astype(np.int64) - 1
    beta = None
    for C_ in CS:
        seen_out = C_ == 1024                                   # C > pool: seen items excluded, every other item listed once
        pcs = [e.retrieve_pieces(sub, C_, None, exclude_seen=seen_out, panel=PANEL, cap=cap, T=T) for e, sub in zip(engs, fsubs)]
        states, short, _, _ = play_retrieve(pcs, False)
        assert all(not e._time_dirty for e in engs) and states.shape == (W, W * cap, 2 * C_ + 4)
        # (1) the merged shortlist is the numpy merge of the W shard states, bit for bit; padding rows and the session-less rank: -1 / -inf
        per_shard = [finished(engs[0], states[w], C_) for w in range(W)]
        for r in range(W):
            rows = slice(r * cap, (r + 1) * cap)
            want_ids, want_sc = merge_shortlists([(i[rows], c[rows]) for i, c in per_shard], C_)
            ids, coarse = _np(*short[r])
            assert (ids == want_ids).all() and coarse.tobytes() == want_sc.tobytes(), (C_, r)
            nloc = edges[r + 1] - edges[r]
            assert (ids[nloc:] == -1).all() and np.isneginf(coarse[nloc:]).all(), (C_, r)
            for w in range(W):                                  # a padding session cost its shard nothing: its state is a reset one
                assert (per_shard[w][0][rows][nloc:] == -1).all(), (C_, r, w)
        ids = gather_local([_np(i)[0] for i, _ in short], edges, cap)
        coarse = gather_local([_np(c)[0] for _, c in short], edges, cap)
        if beta is None:
            beta = band(engs, edges, t)
            close(operands(engs, edges)["A"] @ operands(engs, edges)["E"].T, s, name="A E^T")      # the band is built from what was scored
        # (2) against the fp64 oracle of the trained variables: rules (b) and (c) of test_gpu_retrieve_serve
        for b in range(B):
            if seen_out:
                pool = np.setdiff1d(np.arange(N), seen[b])
                n = len(pool)
                assert sorted(ids[b, :n].tolist()) == pool.tolist(), b
                assert (ids[b, n:] == -1).all() and (coarse[b, n:] == -np.inf).all() and np.isfinite(coarse[b, :n]).all(), b
            else:
                n = C_
                tb = ids[b].astype(np.int64)
                assert (tb >= 0).all() and len(set(tb.tolist())) == C_, b
                cth = np.sort(s[b])[-C_]
                must = np.where(s[b] > cth + 2 * beta[b])[0]
                assert set(must.tolist()) <= set(tb.tolist()), (C_, b, sorted(set(must.tolist()) - set(tb.tolist())))
                assert (s[b, tb] >= cth - 2 * beta[b, tb]).all(), (C_, b)
                err = np.abs(coarse[b].astype(np.float64) - s[b, tb])
                assert (err <= beta[b, tb]).all(), (C_, b, float((err / beta[b, tb]).max()))
            assert (coarse[b, :n - 1] >= coarse[b, 1:n]).all(), (C_, b)
            ties = coarse[b, :n - 1] == coarse[b, 1:n]
            assert (ids[b, :n - 1][ties] > ids[b, 1:n][ties]).all(), (C_, b)
    assert all(not hasattr(e, "ev_logits") for e in engs)      # no buffer of the catalog's width


@pytest.mark.parametrize("W", [2, 3])
@pytest.mark.parametrize("scoring", ["bf16x3-mixed", "bf16x3"])
def test_sharded_two_stage_lists_take_every_slot_from_its_owner(scoring, W):
    _need_gpu()
    t = trained(scoring)
    s, delta = t["s"], t["delta"]
    engs = engines(scoring, W)
    fsubs, edges, cap = split(_feed(), W)
    k, S = TOPK, engs[0].S
    beta = None
    for C_ in (64, 200):
        pcs = [e.retrieve_pieces(sub, C_, k, exclude_seen=False, panel=PANEL, cap=cap, T=T) for e, sub in zip(engs, fsubs)]
        _, short, parts, outs = play_retrieve(pcs, True)
        parts = parts.cpu().numpy()
        tops, top_scs = [], []
        for r in range(W):
            ids = _np(short[r][0])[0]
            topk, top_sc, exact = _np(*outs[r])
            nloc = edges[r + 1] - edges[r]
            assert topk.shape == (nloc, k) and topk.dtype == np.int32
            # (3) every slot: the bits of its owner's part; the other shards wrote -inf there
            own = np.clip(ids, 0, None) // S
            mine = parts[:, r * cap:(r + 1) * cap]
            want = np.where(ids >= 0, np.take_along_axis(mine, own[None], 0)[0], -np.inf).astype(np.float32)
            assert exact.tobytes() == want.tobytes(), (C_, r)
            for w in range(W):
                assert np.isneginf(mine[w][(own != w) | (ids < 0)]).all(), (C_, r, w)
            # (d) of test_gpu_retrieve_serve: the first k of the list order of the exact scores over the shortlist
            for j in range(nloc):
                order = np.lexsort((ids[j], exact[j]))[::-1][:k]
                assert (topk[j] == ids[j, order]).all() and top_sc[j].tobytes() == exact[j, order].tobytes(), (C_, r, j)
            tops.append(topk)
            top_scs.append(top_sc)
        top, top_sc = np.concatenate(tops), np.concatenate(top_scs)
        if beta is None:
            beta = band(engs, edges, t)
        # (e) of test_gpu_retrieve_serve: the band of the streamed lists, the sessions left out whose oracle gap between the k-th and
        # the C-th best score is within the coarse band
        srt = -np.sort(-s, 1)
        keep = srt[:, k - 1] - srt[:, C_ - 1] > 2 * beta.max(1)
        print("C = %d: %d of %d sessions kept" % (C_, keep.sum(), B))
        assert (~keep).mean() <= 0.10, (C_, (~keep).mean())
        check_band(s[keep], delta[keep], top[keep], k, name="two-stage")
        close(top_sc[keep], np.take_along_axis(s, top.astype(np.int64), 1)[keep], name="two-stage scores")
    # last_shortlist / last_exact of the engine call's own names are set by the call itself (world 1 below)

    # (4) seen items and further ids excluded, a window per session: on the shortlist and on the list
    rng = np.random.RandomState(31)
    keys = t["keys"]
    w_lo = rng.randint(0, 300, B).astype(np.int64)
    w_hi = w_lo + rng.randint(300, 700, B)
    extra = np.full((B, 3), -1, np.int32)
    extra[:, 0], extra[:, 2] = top[:, 0], top[:, 5]
    seen = reference()["batch"]["seq"].astype(np.int64) - 1
    C_ = 200
    pcs = []
    for r, (e, sub) in enumerate(zip(engs, fsubs)):
        a, b = edges[r], edges[r + 1]
        pcs.append(e.retrieve_pieces(sub, C_, k, exclude_seen=True, exclude=extra[a:b], panel=PANEL, window=(w_lo[a:b], w_hi[a:b]),
                                     cap=cap, T=T))
    _, short, _, outs = play_retrieve(pcs, True)
    ids = gather_local([_np(i)[0] for i, _ in short], edges, cap)
    top = np.concatenate([_np(o[0])[0] for o in outs])
    for g in range(B):
        gone = set(seen[g].tolist()) | set(extra[g][extra[g] >= 0].tolist())
        ok = (w_lo[g] <= keys) & (keys < w_hi[g])
        ok[list(gone)] = False
        listed = ids[g][ids[g] >= 0]
        assert ok[listed].all() and len(set(listed.tolist())) == len(listed) == min(C_, int(ok.sum())), g
        tk = top[g][top[g] >= 0]
        assert set(tk.tolist()) <= set(listed.tolist()) and len(tk) == min(k, len(listed)), g


@pytest.mark.parametrize("W", [2, 3])
def test_sharded_candidate_scoring_ranks_what_the_owners_scored(W):
    _need_gpu()
    scoring = "bf16x3-mixed"
    t = trained(scoring)
    s = t["s"]
    engs = engines(scoring, W)
    fsubs, edges, cap = split(_feed(), W)
    S, C_ = engs[0].S, 37
    rng = np.random.RandomState(41)
    cand = rng.randint(0, N, (B, C_)).astype(np.int32)
    cand[:, 30:33] = np.take_along_axis(cand, rng.randint(0, 30, (B, 3)), 1)                        # repeats
    cand[:, 33:] = [-1, N, S - 1, min(S, N - 1)]                                                     # empty slots, a shard border
    clicked = (rng.rand(B, C_) < 0.15).astype(np.int32)
    clicked[:, 0] = 1
    pcs = []
    for r, (e, sub) in enumerate(zip(engs, fsubs)):
        a, b = edges[r], edges[r + 1]
        pcs.append(e.cand_pieces(sub, cand[a:b] if sub is not None else None, clicked[a:b] if sub is not None else None, cap=cap, T=T,
                                 C=C_))
    lists, parts, outs = play_candidates(pcs)
    lists = lists.cpu().numpy()
    for r in range(W):
        a, b = edges[r], edges[r + 1]
        assert (lists[r * cap:r * cap + b - a] == cand[a:b]).all() and (lists[r * cap + b - a:(r + 1) * cap] == -1).all()
    if W == 3:
        assert all(o is None or o.shape[0] == 0 for o in outs[1])                                    # the rank without sessions
    scores = np.concatenate([_np(o[0])[0] for o in outs])
    got = [np.concatenate([_np(o[i])[0] for o in outs if o[i] is not None]) for i in range(1, 5)]
    live = (cand >= 0) & (cand < N)
    assert np.isneginf(scores[~live]).all()
    want = np.take_along_axis(s, np.where(live, cand, 0).astype(np.int64), 1)
    close(scores[live], want[live], name="scores")                                                   # the logits gate of the oracle
    # the owner's bits, slot by slot
    parts = parts.cpu().numpy()
    for r in range(W):
        a, b = edges[r], edges[r + 1]
        own = np.clip(cand[a:b], 0, N - 1) // S
        mine = np.take_along_axis(parts[:, r * cap:r * cap + b - a], own[None], 0)[0]
        assert np.where(live[a:b], mine, -np.inf).astype(np.float32).tobytes() == scores[a:b].tobytes(), r
    w_rank, w_order, w_counts, w_metrics = rank_model(scores, np.where(live, cand, -1), clicked)
    assert (got[0] == w_rank).all() and (got[1] == w_order).all() and (got[2] == w_counts).all()
    np.testing.assert_allclose(got[3], w_metrics, rtol=METRIC_RTOL, atol=0)
    # without clicked: no counts, no metrics, the same scores and ranks
    pcs = [e.cand_pieces(sub, cand[edges[r]:edges[r + 1]] if sub is not None else None, cap=cap, T=T, C=C_)
           for r, (e, sub) in enumerate(zip(engs, fsubs))]
    _, _, outs2 = play_candidates(pcs)
    assert all(o[3] is None and o[4] is None for o in outs2)
    assert np.concatenate([_np(o[0])[0] for o in outs2]).tobytes() == scores.tobytes()
    assert (np.concatenate([_np(o[1])[0] for o in outs2]) == w_rank).all()


@pytest.mark.parametrize("scoring", ["bf16x3-mixed", "bf16x3"])
def test_one_rank_without_collectives_gives_the_bits_of_the_pieces_called_by_hand(scoring):
    _need_gpu()
    from tcar_amd import _lib
    (eng,) = engines(scoring, 1)
    feed = _feed()
    C_, k = 200, TOPK
    ids, coarse = _np(*eng.shard_retrieve(feed, C_, panel=PANEL))
    assert eng.xch.order == [] and not eng.xch.collective        # nothing was exchanged
    top, top_sc = _np(*eng.shard_recommend_two_stage(feed, k=k, shortlist=C_, panel=PANEL))
    last_ids, last_exact = _np(eng.last_shortlist, eng.last_exact)
    assert eng.xch.order == [] and (last_ids == ids).all() and last_exact.shape == (B, C_)
    _, short, _, outs = play_retrieve([eng.retrieve_pieces(feed, C_, k, panel=PANEL)], True)
    for a, b in zip((ids, coarse, top, top_sc, last_exact), (short[0][0][:B], short[0][1][:B], outs[0][0], outs[0][1], outs[0][2][:B])):
        assert a.tobytes() == b.cpu().numpy().tobytes()
    cand = np.concatenate([ids[:, :30], np.full((B, 2), -1, np.int32)], 1)
    clicked = (np.arange(32)[None, :] % 5 == 0).astype(np.int32).repeat(B, 0)
    res = [None if x is None else x.cpu().numpy().copy() for x in eng.shard_score_candidates(feed, cand, clicked)]
    assert eng.xch.order == []
    _, _, (out,) = play_candidates([eng.cand_pieces(feed, cand, clicked)])
    for a, b in zip(res, out):
        assert a.tobytes() == b.cpu().numpy().tobytes()
    assert res[0][:, :30].tobytes() == last_exact[:, :30].tobytes()          # the same kernel, the same operands: the same bits
    info = eng.exchange_info()
    assert info["serve_collectives"] == ("serve_rows", "serve_label_scores", "serve_states")
    assert info["retrieve_collectives"] == ("serve_rows", "retrieve_states", "retrieve_shortlists", "cand_parts")
    assert info["cand_collectives"] == ("serve_rows", "cand_lists", "cand_parts")
    assert set(info["retrieve_bytes"]) == set(info["retrieve_collectives"]) and set(info["cand_bytes"]) == set(info["cand_collectives"])
    for call in (lambda: eng.retrieve(feed, 64), lambda: eng.recommend_two_stage(feed), lambda: eng.score_candidates(feed, cand)):
        with pytest.raises(_lib.TcarError, match="whole catalog on one engine"):
            call()                                                # the single-engine names still refuse
    assert not hasattr(eng, "ev_logits")


C_GLOO = 200


def _gloo_lists():
    rng = np.random.RandomState(43)
    cand = rng.randint(-1, N + 1, (B, 19)).astype(np.int32)
    return cand, (rng.rand(B, 19) < 0.2).astype(np.int32)


def _worker(rank, world, port, ret, scoring):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import tcar_amd  # noqa: F401
        from tcar_amd.sharded import ShardedEngine
        r = reference()
        fsubs, edges, cap = split(_feed(), world)
        a, b = edges[rank], edges[rank + 1]
        eng = ShardedEngine(r["params"], r["content"], r["mw"], max_grad=2.0, group=dist.group.WORLD, scoring=scoring)
        out = {}
        ids, coarse = eng.shard_retrieve(fsubs[rank], C_GLOO, panel=PANEL, cap=cap, T=T)
        out["ids"], out["coarse"] = (x.cpu().numpy().tobytes() for x in (ids, coarse))
        assert eng.xch.order == ["serve_rows", "retrieve_states"]
        top, sc = eng.shard_recommend_two_stage(fsubs[rank], k=TOPK, shortlist=C_GLOO, panel=PANEL, cap=cap, T=T)
        torch.cuda.synchronize()
        assert eng.xch.order == ["serve_rows", "retrieve_states", "retrieve_shortlists", "cand_parts"]
        info = eng.exchange_info()
        assert info["retrieve_bytes"]["retrieve_states"] == world * cap * (2 * C_GLOO + 4) * 4        # per rank SENT
        assert info["retrieve_bytes"]["cand_parts"] == world * cap * C_GLOO * 4
        assert info["retrieve_bytes"]["retrieve_shortlists"] == world * cap * C_GLOO * 4             # an all-gather: received
        assert info["all_to_all"] in ("all-to-all (gloo)", "all-gather + slice (gloo)")              # the second: the documented fallback
        out.update(top=top.cpu().numpy().tobytes(), sc=sc.cpu().numpy().tobytes(), exact=eng.last_exact.cpu().numpy().tobytes(),
                   short=eng.last_shortlist.cpu().numpy().tobytes(), path=info["all_to_all"])
        cand, clicked = _gloo_lists()
        res = eng.shard_score_candidates(fsubs[rank], cand[a:b], clicked[a:b], cap=cap, T=T)
        torch.cuda.synchronize()
        assert eng.xch.order == ["serve_rows", "cand_lists", "cand_parts"]
        out["cand"] = [x.cpu().numpy().tobytes() for x in res]
        ret[rank] = out
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
    print("all_to_all_rows over gloo on device tensors: %s" % ret[0]["path"])
    r = reference()
    fsubs, edges, cap = split(_feed(), world)
    engs = [ShardedEngine(r["params"], r["content"], r["mw"], max_grad=2.0, scoring=scoring, world=world, rank=rk) for rk in range(world)]
    pcs = [e.retrieve_pieces(sub, C_GLOO, TOPK, panel=PANEL, cap=cap, T=T) for e, sub in zip(engs, fsubs)]
    _, short, _, outs = play_retrieve(pcs, True)
    cand, clicked = _gloo_lists()
    pcs = [e.cand_pieces(sub, cand[edges[rk]:edges[rk + 1]], clicked[edges[rk]:edges[rk + 1]], cap=cap, T=T)
           for rk, (e, sub) in enumerate(zip(engs, fsubs))]
    _, _, couts = play_candidates(pcs)
    for rk in range(world):
        got, nloc = ret[rk], edges[rk + 1] - edges[rk]
        want = {"ids": short[rk][0][:nloc], "coarse": short[rk][1][:nloc], "short": short[rk][0][:nloc], "top": outs[rk][0], "sc": outs[rk][1],
                "exact": outs[rk][2][:nloc]}
        for name, w in want.items():
            assert got[name] == w.cpu().numpy().tobytes(), (rk, name)
        for a, b in zip(got["cand"], couts[rk]):
            assert a == b.cpu().numpy().tobytes(), rk


def test_the_model_in_sharded_mode_reaches_all_three_calls_and_test_prints_the_two_stage_line():
    _need_gpu()
    import copy
    from tcar_amd import _lib
    from tcar_amd.host.model import Seq2SeqAttNN, initial_variables
    from tcar_amd.host.synth import SynthFold
    from tcar_amd.sharded import ShardedEngine
    fold = SynthFold(n_items=400, dim=32, n_train=300, n_test=200, seed=17, active_t=True)
    te = fold.to_dicts(fold.test, with_active=True)
    np.random.seed(3)
    args = fold.model_args(batch_size=64, epoch=1, neg_num=8, hidden_size=32, time_hidden_size=16, lr=0.003,
                           initial_variables=initial_variables(400, 32, 16, 0.3, 0.1), emb_stddev=0.3, stddev=0.1, scoring="bf16x3",
                           dp_mode="sharded", shard_eval_panel=128)
    with redirect_stdout(io.StringIO()):
        model = Seq2SeqAttNN(args)
    assert isinstance(model.engine, ShardedEngine) and model.engine.world == 1
    idx = np.where(fold.test.in_len == 3)[0][:4]
    assert len(idx) > 0
    feed = {n: v for n, v in fold.test.batch_arrays(idx, "active_t").items() if n not in ("label", "neg")}
    ids, coarse = _np(*model.retrieve(feed, 70))
    assert ids.shape == coarse.shape == (len(idx), 70) and all(len(set(r.tolist())) == 70 for r in ids) and ids.min() >= 0
    top, sc = _np(*model.recommend(feed, k=5, shortlist=70))
    want, want_sc = _np(*model.engine.shard_recommend_two_stage(feed, k=5, shortlist=70))
    assert top.shape == (len(idx), 5) and (top == want).all() and sc.tobytes() == want_sc.tobytes()
    assert all(set(t.tolist()) <= set(r.tolist()) for t, r in zip(top, ids))
    res = model.score_candidates(feed, ids[:, :9], np.ones((len(idx), 9), np.int32))
    assert tuple(res.scores.shape) == (len(idx), 9) and res.counts[:, 0].tolist() == [9] * len(idx)
    assert res.scores.cpu().numpy().tobytes() == model.engine.last_exact[:, :9].cpu().numpy().tobytes()
    plain, plain_sc = _np(*model.recommend(feed, k=5))                         # no shortlist: the streamed selection, as before
    eng_top, eng_sc = _np(*model.engine.recommend(feed, k=5))
    assert (plain == eng_top).all() and plain_sc.tobytes() == eng_sc.tobytes()
    for call in (lambda: model.engine.retrieve(feed, 70), lambda: model.engine.recommend_two_stage(feed, k=5, shortlist=70),
                 lambda: model.engine.score_candidates(feed, ids[:, :9])):
        with pytest.raises(_lib.TcarError, match="whole catalog on one engine"):
            call()
    out = {}
    for short in (0, 80):
        buf = io.StringIO()
        random.seed(5)                                                         # (the sampler shuffles: the same batches in both runs)
        np.random.seed(5)
        with redirect_stdout(buf):
            model.test(None, (copy.deepcopy(te[0]), te[1], te[2]), dict(args, shard_eval_shortlist=short))
        out[short] = (buf.getvalue().splitlines(), dict(model.last_metrics))
    (plain, m0), (lines, m1) = out[0], out[80]
    new = [i for i, l in enumerate(lines) if l.startswith("two-stage lists (shortlist 80): Recall@20: ")]
    assert len(new) == 1 and lines[new[0] - 1].startswith("MRR@20: ")
    assert lines[:new[0]] + lines[new[0] + 1:] == plain                    # every other line, byte for byte
    tw = m1.pop("two_stage")
    assert m1 == m0 and sorted(tw) == ["agreement", "recall", "shortlist"] and tw["shortlist"] == 80
    assert 0.0 <= tw["recall"] <= 1.0 and 0.0 < tw["agreement"] <= 1.0
    assert lines[new[0]] == "two-stage lists (shortlist 80): Recall@20: {}, agreement with the streamed lists: {}".format(
        tw["recall"], tw["agreement"])
    with pytest.raises(ValueError, match="shard_eval_shortlist"):
        model.test(None, (copy.deepcopy(te[0]), te[1], te[2]), dict(args, shard_eval_shortlist=80, shard_eval_panel=0))
