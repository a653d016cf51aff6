"""bench.py on the GPU: a plain run times exactly --steps steps and measures nothing beside the headline (everything else is
behind --full); --dump-outputs writes the last timed step's results as float32 .npy files, equal for equal arguments."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, env=e, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _load(d):
    return {os.path.basename(f)[:-4]: np.load(f) for f in sorted(glob.glob(os.path.join(d, "*.npy")))}


def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    runs = []
    for tag in ("a", "b"):
        d = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / tag)])
        assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
        assert d["unit"] == "sessions/s" and d["higher_is_better"] is True and d["dtype"]
        # value = sessions per second of the same timed steps that ms_per_step divides
        assert abs(d["value"] * d["ms_per_step"] / 1e3 - 512) < 512 * 2e-3
        for k in ("roofline", "cpu_baseline", "end_to_end_sessions_per_s", "gather_roofline", "ms_per_step_by_T",
                  "device_step_sessions_per_s", "ms_per_step_with_kernel_events"):
            assert d[k] is None, k                   # measured with --full only
        runs.append(_load(str(tmp_path / tag)))
    a, b = runs
    assert {"loss", "item_emb_rows", "var.dec_pos", "var.attout_pt_trans.w1"} <= set(a)
    assert a["loss"].shape == (512,) and a["item_emb_rows"].shape[1] == 250
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for k, v in a.items():
        assert v.dtype == np.float32 and np.isfinite(v).all(), k
        # same arguments, same inputs: two runs agree (bit for bit where the step's sums are ordered)
        np.testing.assert_allclose(v, b[k], rtol=1e-5, atol=1e-6, err_msg=k)
    assert abs(float(a["loss"].mean()) - d["last_loss"]) < 1e-3
