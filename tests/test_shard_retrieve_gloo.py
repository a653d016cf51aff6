"""The exchanges of retrieval and candidate scoring over catalog shards on CPU, worlds 2 and 3 over gloo: the PRODUCT's collective
schedules (tcar_amd.sharded.ShardExchange.retrieve / .candidates — the objects ShardedEngine drives with the HIP entry points) with
fp64 torch / numpy pieces built on tests/retrieve_ref.py and tests/retrieve_merge_ref.py, against the single-process answer over the
whole catalog.  No GPU, no HIP library: this pins the sequencing, the buffer shapes with uneven / empty shards of the batch and a short
last shard of the catalog, the all-to-all (each rank receives its own sessions' slice of every shard's result) and the owner-takes-all
combine.

Operands sit on a dyadic grid, so every score is exact in fp64 and in fp32 whatever the order of its sum: the shards' scores ARE the
single process's, ties included.  The coarse scores of the first stage drop the low bits of the grid, the exact ones keep them."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from dist_util import launch  # noqa: E402

SPLITS = {2: [5, 2], 3: [4, 0, 3]}            # the 7 sessions over the ranks: uneven, one rank with none at world 3
CAPS = {2: 6, 3: 5}                           # rows every rank contributes: more than the largest local batch


def _worker(rank, world, port, ret, N=300, B=7):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import tcar_amd  # noqa: F401
        from tcar_amd.sharded import ShardExchange, shard_rows
        from retrieve_merge_ref import merge_shortlists
        from retrieve_ref import shortlist
        rng = np.random.RandomState(3)
        ek, C_, k, X = 24, 40, 9, 4
        rw = 2 * C_ + 4
        E = rng.randint(-8, 9, (N, ek)) / 8.0
        E_hi = np.trunc(E * 2) / 2                                  # the coarse operand: the grid's low bits dropped
        att = rng.randint(-4, 5, (B, ek)) / 4.0
        key = rng.randint(0, 1000, N)
        lo = rng.randint(0, 400, B)
        hi = lo + rng.randint(200, 700, B)
        lo[2], hi[2] = 100, 140                                     # a pool below C: -1 / -inf tails
        lo[3], hi[3] = 2000, 2000                                   # an empty window
        x = (att @ E.T).astype(np.float32)                          # [B, N] exact scores
        xc = (att @ E_hi.T).astype(np.float32)                      # [B, N] coarse scores
        assert ((att @ E.T) == x).all() and ((att @ E_hi.T) == xc).all()
        excl = np.full((B, X), -1, np.int64)
        order = np.argsort(-xc, axis=1, kind="stable")
        excl[:, 0], excl[:, 2] = order[:, 0], order[:, 3]
        S = shard_rows(N, world)
        n0 = min(N, rank * S)
        nl = min(N, n0 + S) - n0
        assert S == (256 if world == 2 else 128) and (rank < world - 1 or nl == 44)       # a SHORT last shard
        sizes, cap = SPLITS[world], CAPS[world]
        b0 = sum(sizes[:rank])
        nloc = sizes[rank]
        Bq = world * cap
        ld = ek + 2 + 2 + X + 2                                     # [attout | live marker | - | lo | hi | X ids | pad]
        st = {}

        class Head:
            def begin(self):
                head = torch.zeros(cap, ld, dtype=torch.float64)
                head[:, ek] = -1
                head[:, ek + 2:ek + 4 + X] = -1                     # padding sessions: marker -1, an empty window, no exclusions
                sl = slice(b0, b0 + nloc)
                head[:nloc, :ek] = torch.from_numpy(att[sl])
                head[:nloc, ek] = 0
                if self.filtered:
                    head[:nloc, ek + 2] = torch.from_numpy(lo[sl].astype(np.float64))
                    head[:nloc, ek + 3] = torch.from_numpy(hi[sl].astype(np.float64))
                    head[:nloc, ek + 4:ek + 4 + X] = torch.from_numpy(excl[sl].astype(np.float64))
                return head

            def prepare(self, head_all):
                assert head_all.shape == (Bq, ld)
                st["att"] = head_all[:, :ek].numpy()
                st["live"] = head_all[:, ek].long().numpy()
                st["lo"], st["hi"] = head_all[:, ek + 2].long().numpy(), head_all[:, ek + 3].long().numpy()
                st["excl"] = head_all[:, ek + 4:ek + 4 + X].long().numpy()
                st["x"] = (st["att"] @ E[n0:n0 + nl].T).astype(np.float32)          # the shard's exact scores of EVERY session

            def scores(self, lists):
                assert lists.shape == (Bq, self.C) and lists.dtype == torch.int32
                ids = lists.numpy().astype(np.int64)
                own = (ids >= n0) & (ids < n0 + nl)
                part = np.where(own, st["x"][np.arange(Bq)[:, None], np.clip(ids - n0, 0, nl - 1)], -np.inf).astype(np.float32)
                return torch.from_numpy(part)

            def combine(self, parts, cand):
                assert parts.shape == (world, cap, self.C)
                owner = np.clip(cand, 0, None) // S
                inside = (cand >= 0) & (cand < N)
                got = parts.numpy()[np.clip(owner, 0, world - 1), np.arange(cap)[:, None], np.arange(self.C)[None, :]]
                return np.where(inside, got, -np.inf).astype(np.float32)

        class Retrieve(Head):
            filtered, C = True, C_

            def fold(self):
                """the shard's coarse scores -> a state per gathered session: score[C] | id[C] | held | threshold words (unused here)"""
                sc = (st["att"] @ E_hi[n0:n0 + nl].T).astype(np.float32)
                whole = np.full((Bq, N), np.nan, np.float32)                       # global ids; the other shards' columns are not there
                whole[:, n0:n0 + nl] = sc
                whole[st["live"] < 0] = np.nan                                     # a padding session folds nothing
                ids, s = shortlist(whole, C_, excl=st["excl"], key=key, lo=st["lo"], hi=st["hi"])
                t = torch.zeros(Bq, rw, dtype=torch.float64)
                t[:, :C_], t[:, C_:2 * C_] = torch.from_numpy(s.astype(np.float64)), torch.from_numpy(ids.astype(np.float64))
                t[:, 2 * C_] = torch.from_numpy((ids >= 0).sum(1).astype(np.float64))
                return t

            def merge(self, states):
                assert states.shape == (world, cap, rw)
                lists = [(states[w, :, C_:2 * C_].numpy().astype(np.int32), states[w, :, :C_].numpy().astype(np.float32))
                         for w in range(world)]
                st["ids"], st["coarse"] = merge_shortlists(lists, C_)
                return torch.from_numpy(st["ids"])

            def shortlist(self):
                return st["ids"][:nloc], st["coarse"][:nloc]

            def rerank(self, parts):
                exact = self.combine(parts, st["ids"])
                topk = np.full((cap, k), -1, np.int32)
                for b in range(cap):
                    live = np.where(st["ids"][b] >= 0)[0]
                    o = live[np.lexsort((st["ids"][b, live], exact[b, live]))][::-1][:k]
                    topk[b, :len(o)] = st["ids"][b, o]
                return topk[:nloc], exact[:nloc]

        class Cand(Head):
            filtered, C = False, 11

            def lists(self):
                t = torch.full((cap, self.C), -1, dtype=torch.int32)
                t[:nloc] = torch.from_numpy(cand[b0:b0 + nloc])
                st["cand"] = t.numpy()
                return t

            def rank(self, parts):
                return self.combine(parts, st["cand"])[:nloc]

        xch = ShardExchange(dist.group.WORLD)
        assert xch.world == world and xch.rank == rank
        # ---- the known-answer check of preflight covers the all-to-all: it answers rightly, or the backend has none (reported, not fatal)
        from tcar_amd import dp
        caps = {}
        assert dp.known_answers(dp._GroupOps(dist.group.WORLD), world, rank, torch.device("cpu"), caps) is None
        assert caps["all_to_all"] in (True, False) and (caps["all_to_all"] or "all_to_all_error" in caps)
        info = dp.preflight(dist.group.WORLD, "cpu", verbose=False)
        assert info["all_to_all"] == caps["all_to_all"]

        class NoAllToAll(dp._GroupOps):
            def all_to_all(self, send, recv):
                raise NotImplementedError("no all-to-all here")

        class WrongAllToAll(dp._GroupOps):
            def all_to_all(self, send, recv):
                recv.zero_()
        caps = {}
        assert dp.known_answers(NoAllToAll(dist.group.WORLD), world, rank, torch.device("cpu"), caps) is None and caps["all_to_all"] is False
        assert dp.known_answers(WrongAllToAll(dist.group.WORLD), world, rank, torch.device("cpu")).startswith("all_to_all: returned")
        # ---- all_to_all_rows is all-gather + slice, byte for byte (fp32 with NaN payloads and int32)
        for t in (torch.from_numpy(rng.randint(-2 ** 31, 2 ** 31, (Bq, 5)).astype(np.int32)) + rank,
                  torch.from_numpy(rng.randint(-2 ** 31, 2 ** 31, (Bq, 3)).astype(np.int32) ^ rank).view(torch.float32)):
            got = xch.all_to_all_rows(t.clone(), cap, "a2a")
            want = xch.all_gather(t)[:, rank * cap:(rank + 1) * cap]
            assert got.shape == (world, cap, t.shape[1]) and got.dtype == t.dtype
            assert got.contiguous().numpy().tobytes() == want.contiguous().numpy().tobytes()
            assert xch.bytes_moved["a2a"] == Bq * t.shape[1] * 4
        assert xch.all_to_all_path in ("all-to-all (gloo)", "all-gather + slice (gloo)")       # the second: the documented fallback
        forced = ShardExchange(dist.group.WORLD, all_to_all=False)
        t = torch.arange(Bq * 2, dtype=torch.float32).view(Bq, 2) + 1000 * rank
        got = forced.all_to_all_rows(t, cap, "a2a")
        assert forced.all_to_all_path == "all-gather + slice (gloo)"
        assert all(torch.equal(got[r], torch.arange(Bq * 2, dtype=torch.float32).view(Bq, 2)[rank * cap:(rank + 1) * cap] + 1000 * r)
                   for r in range(world))

        # ---- a retrieval: two collectives
        want_ids, want_sc = shortlist(xc, C_, excl=excl, key=key, lo=lo, hi=hi)
        ids, sc = xch.retrieve(Retrieve(), cap, rerank=False)
        assert xch.order == ["serve_rows", "retrieve_states"]
        assert xch.bytes_moved["retrieve_states"] == Bq * rw * 8
        sl = slice(b0, b0 + nloc)
        assert ids.shape == (nloc, C_) and (ids == want_ids[sl]).all() and sc.tobytes() == want_sc[sl].tobytes()
        assert (st["ids"][nloc:] == -1).all() and np.isneginf(st["coarse"][nloc:]).all()               # padding sessions
        if nloc > 3:
            assert (ids[2] >= 0).sum() < C_ and (ids[3] == -1).all()
        # ---- the two-stage call: four collectives
        topk, exact = xch.retrieve(Retrieve(), cap, rerank=True)
        assert xch.order == ["serve_rows", "retrieve_states", "retrieve_shortlists", "cand_parts"]
        assert xch.bytes_moved["retrieve_shortlists"] == world * cap * C_ * 4 and xch.bytes_moved["cand_parts"] == Bq * C_ * 4
        for j in range(nloc):
            b = b0 + j
            live = want_ids[b] >= 0
            assert exact[j][live].tobytes() == x[b, want_ids[b][live]].tobytes() and np.isneginf(exact[j][~live]).all(), b
            items = want_ids[b][live]
            o = items[np.lexsort((items, x[b, items]))][::-1][:k]
            assert topk[j].tolist() == o.tolist() + [-1] * (k - len(o)), b
        # ---- candidate lists: three collectives
        cand = rng.randint(0, N, (B, Cand.C)).astype(np.int32)
        cand[:, 2], cand[:, 5], cand[:, 7] = -1, N + 4, cand[:, 0]
        cand[:, 8], cand[:, 9] = S - 1, min(S, N - 1)                                                 # both sides of a shard border
        got = xch.candidates(Cand(), cap)
        assert xch.order == ["serve_rows", "cand_lists", "cand_parts"]
        inside = (cand >= 0) & (cand < N)
        want = np.where(inside, np.take_along_axis(x, np.clip(cand, 0, N - 1).astype(np.int64), 1), -np.inf).astype(np.float32)
        assert got.shape == (nloc, Cand.C) and got.tobytes() == want[sl].tobytes()
        ret[rank] = "ok"
    except Exception as e:
        import traceback
        ret[rank] = "FAIL: " + repr(e) + "\n" + traceback.format_exc()
    finally:
        dist.destroy_process_group()


def _run(world):
    ret = launch(_worker, world)
    for r in range(world):
        assert ret.get(r) == "ok", ret.get(r)


def test_retrieve_and_candidate_exchanges_two_ranks_gloo():
    _run(2)


def test_retrieve_and_candidate_exchanges_three_ranks_one_without_sessions_gloo():
    _run(3)
