"""Two data-parallel ranks on ONE GPU (gloo backend moving CUDA tensors through the host): exercises the complete
DPEngine path on the real kernels — rank-local forward/backward from the C++ driver, emit-rows gather backward, the
GradExchange collective schedule, scatter of the all-gathered rows, clip + Adam — against a single engine that sees the
concatenated batch.  (RCCL itself needs >1 GPU; the driver's scaling run covers it.)"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from dist_util import launch  # noqa: E402
from step_cases import _case  # noqa: E402

pytestmark = pytest.mark.gpu


def _worker(rank, world, port, ret, scoring):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import tcar_amd  # noqa: F401
        from tcar_amd.dp import DPEngine, shard_bounds
        from tcar_amd.engine import TcarEngine
        N, H, Ht, B, T, K = 1000, 250, 64, 37, 4, 6          # 37 sessions: uneven shards (19 + 18)
        params, content, mw, batch = _case(N, H, Ht, B, T, K, seed=5)
        lo, hi, cap = shard_bounds(B, world, rank)
        sub = {k: v[lo:hi] for k, v in batch.items()}
        eng = DPEngine(params, content, mw, max_grad=2.0, group=dist.group.WORLD, scoring=scoring)
        for _ in range(3):
            eng.train_step(sub, cap_rows=cap * T)
        torch.cuda.synchronize()
        assert eng.async_exchanges == 3          # the collectives really ran on the communication stream (overlapped path)
        got = eng.export_params()
        if rank == 0:
            ref = TcarEngine(params, content, mw, max_grad=2.0, scoring=scoring)
            for _ in range(3):
                ref.train_step(batch)
            want = ref.export_params()
            for k in want:
                d = np.abs(got[k] - want[k]).max()
                # same kernels, different summation order (float atomics, reduction trees): Adam bound as in test_gpu_parity
                assert d <= 1e-3 * np.abs(want[k]).max() + 0.25 * 1e-3 * 3, (k, d)
        # replicas agree with each other
        flat = torch.cat([torch.tensor(v).reshape(-1) for v in got.values()])
        other = [torch.zeros_like(flat) for _ in range(world)]
        dist.all_gather(other, flat)
        assert float((other[0] - other[1]).abs().max()) <= 2e-4
        ret[rank] = "ok"
    except Exception as e:
        import traceback
        ret[rank] = "FAIL: " + repr(e) + "\n" + traceback.format_exc()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("scoring", ["f32", "bf16x3"])
def test_two_ranks_match_single_engine(scoring):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    world = 2
    ret = launch(_worker, world, scoring, spawned_manager=True)
    for r in range(world):
        assert ret.get(r) == "ok", ret.get(r)


def _cli_worker(rank, world, port, ret, argv):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), TCAR_DIST_BACKEND="gloo", TCAR_SAME_DEVICE="1")
    try:
        import io
        from contextlib import redirect_stdout
        import tcar_amd  # noqa: F401
        from tcar_amd.host.cli import main
        with redirect_stdout(io.StringIO()):
            model = main(argv + ["--gpus", str(world)])
        ret[rank] = dict(model.last_metrics, sessions=model.train_sessions)
    except Exception as e:
        import traceback
        ret[rank] = "FAIL: " + repr(e) + "\n" + traceback.format_exc()


@pytest.mark.parametrize("extra", [[], ["--dp_mode", "sharded"], ["--dp_mode", "sharded", "--device_sampler", "1"]])
def test_cli_two_ranks_shard_batches_and_agree_with_one_rank(extra):
    """main.py --gpus 2: both ranks form the same batches, train on their contiguous shards (DPEngine, or the catalog-sharded
    ShardedEngine with --dp_mode sharded) and evaluate their shards; the all-reduced metrics equal the single-process run's
    up to float-atomic noise."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import io
    from contextlib import redirect_stdout
    argv = ["--synthetic", "700", "--synthetic_train", "3000", "--synthetic_test", "600", "--epoch", "2",
            "--hidden_size", "48", "--time_hidden_size", "16", "--batch_size", "128", "--gap_mode", "click_delta"]
    ret = launch(_cli_worker, 2, argv + extra, spawned_manager=True)
    for r in range(2):
        assert isinstance(ret.get(r), dict), ret.get(r)
    assert ret[0] == ret[1]                                   # every rank reports the same all-reduced numbers
    import tcar_amd  # noqa: F401
    from tcar_amd.host.cli import main
    with redirect_stdout(io.StringIO()):
        one = main(argv)
    m1, m2 = one.last_metrics, ret[0]
    assert m2["sessions"] == one.train_sessions               # every session was trained on exactly once
    dev_neg = "--device_sampler" in extra                     # other negative stream than the host-sampled reference run
    assert abs(m1["loss"] - m2["loss"]) <= (2e-2 if dev_neg else 2e-3) * abs(m1["loss"])
    for k in ("recall", "mrr", "ndcg"):
        assert abs(m1[k] - m2[k]) <= (0.03 if dev_neg else 0.01), (k, m1[k], m2[k])
