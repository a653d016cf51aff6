"""The collective layer of both exchanges (tcar_amd.dp.Collectives) and the agreement of the direct RCCL path (rccl.make_direct)
at world size 2 over gloo on CPU: known answers of every collective the schedules use, the sim shapes, `force` on a one-rank
group, a rank that does not match the group, the two agreements of make_direct with one rank failing (a monkeypatched local check,
a stand-in communicator that answers wrongly) and close()."""
import ctypes as C
import datetime
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dist_util import launch  # noqa: E402

ENV = ("TCAR_FORCE_COLLECTIVES", "TCAR_RCCL_DIRECT", "TCAR_SIM_WORLD")


def _worker(rank, world, port, ret):
    for k in ENV:
        os.environ.pop(k, None)
    import tcar_amd  # noqa: F401
    from tcar_amd import dp, rccl
    cpu = torch.device("cpu")
    try:
        # ---- sim: TCAR_SIM_WORLD on a process without a process group = the shapes of rank 0 of a W-rank job, no collective
        os.environ["TCAR_SIM_WORLD"] = "4"
        sim = dp.Collectives(sim=None)
        assert (sim.world, sim.rank, sim.sim, sim.collective) == (4, 0, True, False)
        assert not dp.Collectives().sim                                   # (sim=False: the variable is not read)
        x = torch.arange(6.0).view(2, 3)
        assert torch.equal(sim.all_gather(x, "a"), x.expand(4, 2, 3))
        assert torch.equal(sim.reduce_scatter_rows(torch.arange(8.0).view(4, 2), 1, "b"), torch.tensor([[0.0, 1.0]]))
        assert torch.equal(sim.all_reduce(x.clone(), "c"), x)
        sim.share_rows(torch.zeros(4, 2, 3), lambda st: (_ for _ in ()).throw(AssertionError("installed")))
        sim.wait_rows()
        assert sim.order == [] and sim.bytes_moved == {}
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        # (a rank that skipped or added a collective fails at the time-out instead of hanging the suite)
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
        group = dist.group.WORLD
        assert not dp.Collectives(group, sim=None).sim                    # a live group: TCAR_SIM_WORLD does not apply
        os.environ.pop("TCAR_SIM_WORLD")
        # ---- the known-answer check of preflight and of the direct self-test, through the process group
        assert dp.known_answers(dp._GroupOps(group), world, rank, cpu) is None
        # ---- the layer's collectives against their known answers
        xc = dp.Collectives(group)
        assert xc.collective and (xc.world, xc.rank, xc.backend) == (world, rank, "gloo")
        assert xc.direct is None and not xc.use_reduce_scatter
        t = torch.arange(6.0).view(2, 3) + 10 * rank
        got = xc.all_gather(t, "ag")
        assert got.shape == (world, 2, 3) and all(torch.equal(got[r], torch.arange(6.0).view(2, 3) + 10 * r) for r in range(world))
        full = torch.arange(8.0).view(4, 2) * (rank + 1)                 # [W * cap, C], cap 2: all-reduce + slice on gloo
        rows = xc.reduce_scatter_rows(full, 2, "rs")
        assert torch.equal(rows, (torch.arange(8.0).view(4, 2) * 3)[2 * rank:2 * rank + 2])
        a = torch.full((5,), float(rank + 1))
        assert xc.all_reduce(a, "ar") is a and torch.equal(a, torch.full((5,), 3.0))
        stage = torch.zeros(world, 3, 4)
        stage[rank] = rank + 1.0
        installed = []
        xc.share_rows(stage, installed.append)
        assert installed == []                                            # asynchronous: installed by wait_rows
        xc.wait_rows()
        assert len(installed) == 1 and all(bool((installed[0][r] == r + 1.0).all()) for r in range(world))
        assert xc.order == ["ag", "rs", "ar", "item_rows"]
        assert xc.bytes_moved == {"ag": world * 6 * 4, "rs": 8 * 4, "ar": 5 * 4, "item_rows": world * 12 * 4}
        n = len(xc.order)
        xc.all_reduce(torch.ones(2))                                      # no key: not counted
        assert len(xc.order) == n and xc.collective_ms() == {}
        # ---- one-rank group: collectives short-circuit unless forced (argument or TCAR_FORCE_COLLECTIVES)
        solo = [dist.new_group([r]) for r in range(world)][rank]
        assert not dp.Collectives(solo).collective and dp.Collectives(solo).all_gather(x).shape == (1, 2, 3)
        forced = dp.Collectives(solo, force=True)
        assert forced.collective and (forced.world, forced.rank, forced.backend) == (1, 0, "gloo")
        assert torch.equal(forced.all_gather(x, "ag")[0], x) and forced.order == ["ag"]
        assert torch.equal(forced.reduce_scatter_rows(torch.arange(4.0).view(2, 2), 2, "rs"), torch.arange(4.0).view(2, 2))
        os.environ["TCAR_FORCE_COLLECTIVES"] = "1"
        assert dp.Collectives(solo).collective and not dp.Collectives(solo, force=False).collective
        os.environ.pop("TCAR_FORCE_COLLECTIVES")
        # ---- a rank / world that is not the group's, with live collectives, is refused
        for w, r in ((world, 1 - rank), (world + 2, rank)):
            try:
                dp.Collectives(group, world=w, rank=r)
                raise AssertionError("rank %d of %d accepted" % (r, w))
            except ValueError:
                pass
        assert not dp.Collectives(solo, world=1, rank=0).collective      # (no collective: the shape is the caller's)
        # ---- make_direct: every rank takes the same branch
        made = []
        wrong = {"rank": None}

        class FakeComm(rccl.RcclComm):
            """RCCL's three calls over the gloo group (rank wrong["rank"] answers its all-reduce wrongly); the REAL destroy()
            against a library that counts ncclCommDestroy"""

            def __init__(self, group, device):
                made.append(self)
                self.world, self.rank, self.dev = dist.get_world_size(group), dist.get_rank(group), device
                self.comm, self._lib, self.destroyed = C.c_void_p(1), self, 0
                self.pg = dp._GroupOps(group)
                self.all_gather, self.reduce_scatter = self.pg.all_gather, self.pg.reduce_scatter

            def all_reduce(self, t):
                self.pg.all_reduce(t)
                if wrong["rank"] == self.rank:
                    t += 1

            def ncclCommDestroy(self, comm):
                self.destroyed += 1

        rccl.RcclComm = FakeComm
        # (1) one rank's local check fails: NO rank enters the id broadcast / ncclCommInitRank
        rccl._local_check = lambda want: None if rank == 0 else "monkeypatched"
        assert rccl.make_direct(group, device=cpu, verbose=False) is None and made == []
        # (2) every local check passes, rank 1's communicator answers wrongly: both fall back, both communicators destroyed
        rccl._local_check = lambda want: None
        wrong["rank"] = 1
        assert rccl.make_direct(group, device=cpu, verbose=False) is None
        assert len(made) == 1 and made[0].destroyed == 1
        # (3) every rank passes: every rank gets its communicator; close() destroys it once, however often it is called
        wrong["rank"] = None
        comm = rccl.make_direct(group, device=cpu, verbose=False)
        assert comm is made[-1] and comm.destroyed == 0
        xc.direct = xc.ops = comm
        xc.close()
        xc.close()
        assert comm.destroyed == 1 and not comm.comm.value
        forced.close()
        forced.close()
        ret[rank] = "ok"
    except Exception as e:
        import traceback
        ret[rank] = "FAIL: " + repr(e) + "\n" + traceback.format_exc()
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_collectives_layer_world2_gloo():
    world = 2
    ret = launch(_worker, world)
    for r in range(world):
        assert ret.get(r) == "ok", ret.get(r)
