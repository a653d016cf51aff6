"""What the GPU tests of the catalog-sharded engine's serving calls share (test_gpu_shard_serve.py, test_gpu_shard_retrieve.py,
test_gpu_catalog_shard.py), on the inputs of serve_case.py: the panel and the split of the 41 sessions over W ranks, the variables
after two training steps with the fp64 oracle's logits / CE of them, W engines ShardedEngine(world=W, rank=r) in ONE process without a
process group, and the collectives of ShardExchange.serve / .retrieve / .candidates played by hand (all-gather = concatenation in
rank order, all-to-all = every rank takes its own rows of every rank's buffer)."""
import ctypes as C

import numpy as np
import torch

from serve_case import N, reference

PANEL = 128                                     # shards of 384 / 316 rows (W = 2) and 256 / 256 / 188 (W = 3): several panels each, the last partial
SPLITS = {2: ([25, 16], 27), 3: ([20, 0, 21], 23)}       # sessions per rank (uneven, one rank with none at W = 3), cap > the largest


_TRAINED = {}


def trained(scoring):
    """the variables after two training steps on identical batches + the fp64 oracle's logits / CE of them: computed once per scoring
    mode, shared, never written"""
    if scoring not in _TRAINED:
        from oracle.tcar_oracle import TcarOracle
        from tcar_amd.sharded import ShardedEngine
        r = reference()
        eng = ShardedEngine(r["params"], r["content"], r["mw"], max_grad=2.0, scoring=scoring, world=1, rank=0)
        for _ in range(2):
            eng.train_step(r["batch"])
        state = eng.export_state()
        params = eng.export_params()
        logits, ce = TcarOracle(params, r["content"], r["mw"]).eval_batch(r["batch"])
        s, ce = logits.numpy().astype(np.float64), ce.numpy().astype(np.float64)
        rng = np.random.RandomState(23)
        keys = rng.randint(0, 1000, N).astype(np.int32)
        cat = rng.randint(0, 12, N).astype(np.int32)
        for a in (s, ce, keys, cat):
            a.setflags(write=False)
        _TRAINED[scoring] = dict(state=state, s=s, ce=ce, delta=1e-3 * np.abs(s).max(1), keys=keys, cat=cat)
    return _TRAINED[scoring]


def engines(scoring, W):
    from tcar_amd.sharded import ShardedEngine
    r, t = reference(), trained(scoring)
    out = []
    for rank in range(W):
        e = ShardedEngine(r["params"], r["content"], r["mw"], max_grad=2.0, scoring=scoring, world=W, rank=rank)
        e.load_state(t["state"])
        assert e._time_dirty, ("rank", rank)                  # the candidate-time planes of the shard are stale
        e.set_item_keys(t["keys"])
        e.set_categories(t["cat"])
        out.append(e)
    return out


def split(batch, W, splits=SPLITS):
    """the sessions of `batch` dealt to W ranks by splits[W] = (sessions per rank, cap) -> (the ranks' feeds, None for a rank
    without sessions; the edges [W + 1]; cap)"""
    sizes, cap = splits[W]
    edges = np.r_[0, np.cumsum(sizes)]
    subs = [({k: v[a:b] for k, v in batch.items()} if b > a else None) for a, b in zip(edges[:-1], edges[1:])]
    return subs, edges, cap


def play(pcs):
    """ShardExchange.serve with the collectives played by hand: all-gather = concatenation of the ranks' buffers in rank order"""
    head_all = torch.cat([pc.begin().clone() for pc in pcs])
    parts = [pc.prepare(head_all) for pc in pcs]
    if pcs[0].labelled:
        parts_all = torch.stack([p.clone() for p in parts])
        for pc in pcs:
            pc.label_scores(parts_all)
    states = torch.stack([pc.fold().clone() for pc in pcs])
    outs = [tuple(o.clone() for o in pc.finish(states)) for pc in pcs]
    torch.cuda.synchronize()
    return head_all, states, outs


def shard_states(eng, states, k):
    """every shard's state of every gathered session, read through tcar_select_finish -> select_ref states [W][Bq]"""
    W, Bq, rw = states.shape
    out = []
    for w in range(W):
        topk = torch.empty(Bq, k, dtype=torch.int32, device="cuda")
        score = torch.zeros(Bq, k, device="cuda")
        rank = torch.zeros(Bq, dtype=torch.int32, device="cuda")
        st = states[w].contiguous()
        rc = eng.lib.tcar_select_finish(Bq, k, C.c_void_p(st.data_ptr()), None, C.c_void_p(topk.data_ptr()), C.c_void_p(score.data_ptr()),
                                        C.c_void_p(rank.data_ptr()), None, None)
        assert rc == 0, ("tcar_select_finish", rc, Bq, k)
        torch.cuda.synchronize()
        tk, sc, cnt = topk.cpu().numpy(), score.cpu().numpy(), rank.cpu().numpy() - 1
        ms = st[:, 2 * k + 1:2 * k + 3].contiguous().view(torch.float32).cpu().numpy()
        row = []
        for b in range(Bq):
            n = int((tk[b] >= 0).sum())
            assert (tk[b, n:] == -1).all(), ("shard", w, "session", b, tk[b])
            row.append({"ids": tk[b, :n].tolist(), "scores": sc[b, :n].copy(), "count": int(cnt[b]), "m": float(ms[b, 0]), "s": float(ms[b, 1])})
        out.append(row)
    return out


def _rows(t, r, cap):
    """what rank r receives of an all-to-all over the ranks' buffers t [W, W*cap, x]: its own rows of every rank's buffer"""
    return t[:, r * cap:(r + 1) * cap].contiguous()


def play_retrieve(pcs, rerank):
    """ShardExchange.retrieve with the collectives played by hand -> (states [W, W*cap, 2C+4], the W shortlists (ids, coarse) over
    all cap rows, parts [W, W*cap, C] or None, per rank (topk, scores, exact [cap, C]) or None)"""
    cap = pcs[0].cap
    head_all = torch.cat([pc.begin().clone() for pc in pcs])
    for pc in pcs:
        pc.prepare(head_all)
    states = torch.stack([pc.fold().clone() for pc in pcs])
    ids = [pc.merge(_rows(states, r, cap)).clone() for r, pc in enumerate(pcs)]
    short = [(i, pc.eng.rs_scores[:cap].clone()) for i, pc in zip(ids, pcs)]
    parts = outs = None
    if rerank:
        lists = torch.cat(ids)
        parts = torch.stack([pc.scores(lists).clone() for pc in pcs])
        outs = []
        for r, pc in enumerate(pcs):
            topk, sc = pc.rerank(_rows(parts, r, cap))
            outs.append((topk.clone(), sc.clone(), pc.eng.rs_exact[:cap].clone()))
    torch.cuda.synchronize()
    return states, short, parts, outs


def play_candidates(pcs):
    cap = pcs[0].cap
    head_all = torch.cat([pc.begin().clone() for pc in pcs])
    for pc in pcs:
        pc.prepare(head_all)
    lists = torch.cat([pc.lists().clone() for pc in pcs])
    parts = torch.stack([pc.scores(lists).clone() for pc in pcs])
    outs = [tuple(None if o is None else o.clone() for o in pc.rank(_rows(parts, r, cap))) for r, pc in enumerate(pcs)]
    torch.cuda.synchronize()
    return lists, parts, outs
