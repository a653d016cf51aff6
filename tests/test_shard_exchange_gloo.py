"""The exchange of the catalog-sharded streamed selection on CPU, worlds 2 and 3 over gloo: the PRODUCT's collective schedule
(tcar_amd.sharded.ShardExchange.serve — the same object ShardedEngine drives with the HIP entry points) with numpy / torch pieces built
on the model of tests/select_ref.py, against the single-process model of the whole catalog (no GPU, no HIP library: this pins the
sequencing, the buffer shapes of uneven / empty shards of the batch and a short last shard of the catalog, the label score taken from
the label's owner, and the algebra of the state merge with windows, exclusions and a cap in the packed rows).

Operands sit on a dyadic grid, so every score is exact in fp64 and in fp32 whatever the order of its sum: the shards' scores ARE the
single process's, ties included."""
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
        from select_ref import finish, fold_state, merge_states
        rng = np.random.RandomState(3)
        ek, k, X = 24, 20, 4
        rw = 2 * k + 4
        E = rng.randint(-8, 9, (N, ek)) / 8.0
        att = rng.randint(-4, 5, (B, ek)) / 4.0
        lab = rng.randint(0, N, B)
        key = rng.randint(0, 1000, N)
        lo = rng.randint(0, 400, B)
        hi = lo + rng.randint(200, 700, B)
        lo[2], hi[2] = 2000, 2000                                  # an empty window: the pool of session 2 is its label alone
        cat = rng.randint(0, 6, N).astype(np.int32)
        x = (att @ E.T).astype(np.float32)                          # [B, N], exact
        assert ((att @ E.T) == x).all()
        excl = np.full((B, X), -1, np.int64)
        order = np.argsort(-x, axis=1, kind="stable")
        excl[:, 0], excl[:, 2] = order[:, 0], order[:, 3]           # the best item and another one; slots 1 and 3 stay empty
        S = shard_rows(N, world)
        n0 = min(N, rank * S)
        nl = min(N, n0 + S) - n0
        assert S == (256 if world == 2 else 128) and (rank < world - 1 or nl == 44)       # a SHORT last shard
        sizes, cap = SPLITS[world], CAPS[world]
        b0 = sum(sizes[:rank])
        nloc = sizes[rank]
        Bq = world * cap
        ld = ek + 2 + 2 + X + 2                                     # [attout | label | - | lo | hi | X ids | pad]
        st = {}

        def pack64(states):
            t = torch.zeros(len(states), rw, dtype=torch.float64)
            t[:, :k], t[:, k:2 * k] = -np.inf, -1
            for b, s in enumerate(states):
                n = len(s["ids"])
                t[b, :n] = torch.from_numpy(s["scores"].astype(np.float64))
                t[b, k:k + n] = torch.tensor(s["ids"], dtype=torch.float64)
                t[b, 2 * k], t[b, 2 * k + 1], t[b, 2 * k + 2] = s["count"], s["m"], s["s"]
            return t

        def unpack64(row):
            ids = row[k:2 * k].long().numpy()
            n = int((ids >= 0).sum())
            return {"ids": ids[:n].tolist(), "scores": row[:n].numpy().astype(np.float32), "count": int(row[2 * k]),
                    "m": float(row[2 * k + 1]), "s": float(row[2 * k + 2])}

        class Pieces:
            def __init__(self, labelled, cap_m):
                self.labelled, self.cap_m = labelled, cap_m

            def begin(self):
                head = torch.zeros(cap, ld, dtype=torch.float64)
                head[:, ek] = -1
                head[:, ek + 2:ek + 4 + X] = -1                     # padding sessions: label -1, an empty window, no exclusions
                sl = slice(b0, b0 + nloc)
                head[:nloc, :ek] = torch.from_numpy(att[sl])
                head[:nloc, ek] = torch.from_numpy(lab[sl].astype(np.float64))
                head[:nloc, ek + 2] = torch.from_numpy(lo[sl].astype(np.float64))
                head[:nloc, ek + 3] = torch.from_numpy(hi[sl].astype(np.float64))
                head[:nloc, ek + 4:ek + 4 + X] = torch.from_numpy(excl[sl].astype(np.float64))
                return head

            def prepare(self, head_all):
                assert head_all.shape == (Bq, ld)
                st["att"] = head_all[:, :ek].numpy()
                st["lab"] = head_all[:, ek].long().numpy()
                st["lo"], st["hi"] = head_all[:, ek + 2].long().numpy(), head_all[:, ek + 3].long().numpy()
                st["excl"] = head_all[:, ek + 4:ek + 4 + X].long().numpy()
                st["x"] = (st["att"] @ E[n0:n0 + nl].T).astype(np.float32)          # the shard's scores of EVERY session
                if not self.labelled:
                    return None
                here = (st["lab"] >= n0) & (st["lab"] < n0 + nl)                    # (a padding session's -1 is nowhere)
                part = np.where(here, st["x"][np.arange(Bq), np.clip(st["lab"] - n0, 0, nl - 1)], np.float32(0))
                return torch.from_numpy(part.astype(np.float32))

            def label_scores(self, parts_all):
                assert self.labelled and parts_all.shape == (world, Bq)
                owner = np.clip(st["lab"], 0, None) // S
                st["ls"] = parts_all.numpy()[owner, np.arange(Bq)]

            def fold(self):
                ids = np.arange(n0, n0 + nl)
                states = []
                for b in range(Bq):
                    pool = (key[ids] >= st["lo"][b]) & (key[ids] < st["hi"][b])
                    kw = dict(label=int(st["lab"][b]), lab_score=st["ls"][b]) if self.labelled else {}
                    ex = st["excl"][b]
                    states.append(fold_state(ids, st["x"][b], k, pool=pool, excl=ex[ex >= 0], cat=cat, cap=self.cap_m, **kw))
                return pack64(states)

            def finish(self, states):
                assert states.shape == (world, Bq, rw)
                out = []
                for b in range(rank * cap, rank * cap + nloc):
                    m = merge_states([unpack64(states[w, b]) for w in range(world)], k, cat, self.cap_m)
                    out.append((m, finish(m, k, st["ls"][b] if self.labelled else None)))
                return out

        def whole(b, labelled, cap_m):
            ids = np.arange(N)
            pool = (key >= lo[b]) & (key < hi[b])
            kw = dict(label=int(lab[b]), lab_score=x[b, lab[b]]) if labelled else {}
            ex = excl[b]
            return fold_state(ids, x[b], k, pool=pool, excl=ex[ex >= 0], cat=cat, cap=cap_m, **kw)

        xch = ShardExchange(dist.group.WORLD)
        assert xch.world == world and xch.rank == rank
        # ---- evaluation: three collectives
        got = xch.serve(Pieces(True, None), cap, labelled=True)
        assert xch.order == ["serve_rows", "serve_label_scores", "serve_states"]
        assert xch.bytes_moved == {"serve_rows": Bq * ld * 8, "serve_label_scores": world * Bq * 4, "serve_states": world * Bq * rw * 8}
        assert len(got) == nloc
        for j, (m, (tk, rk, ce)) in enumerate(got):
            b = b0 + j
            w = whole(b, True, None)
            tk_w, rk_w, ce_w = finish(w, k, x[b, lab[b]])
            assert tk == tk_w and m["scores"].tobytes() == w["scores"].tobytes() and rk == rk_w, (b, tk, tk_w, rk, rk_w)
            assert abs(ce - ce_w) <= 1e-12 * max(1.0, abs(ce_w)), (b, ce, ce_w)
            assert not set(tk) & set(excl[b][excl[b] >= 0].tolist())
            assert all(i < 0 or (lo[b] <= key[i] < hi[b]) or i == lab[b] for i in tk)
            if b == 2:
                assert tk_w[:1] == [int(lab[2])] or int(lab[2]) in excl[2]          # the label alone
                assert rk == 1 and ce == 0.0
        # ---- recommendation with a cap: two collectives, no label anywhere
        got = xch.serve(Pieces(False, 2), cap, labelled=False)
        assert xch.order == ["serve_rows", "serve_states"]
        for j, (m, (tk, rk, ce)) in enumerate(got):
            b = b0 + j
            w = whole(b, False, 2)
            assert m["ids"] == w["ids"] and m["scores"].tobytes() == w["scores"].tobytes() and rk is None, b
            assert all(np.bincount(cat[m["ids"]], minlength=6) <= 2) if m["ids"] else True
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


def test_serve_exchange_two_ranks_gloo():
    _run(2)


def test_serve_exchange_three_ranks_one_without_sessions_gloo():
    _run(3)
