"""Streamed evaluation and recommendation at the engine level (TcarEngine.eval_step_streamed / recommend, tcar_serve_step) against
the fp64 oracle.  The engine's scores differ from the oracle's by rounding, so lists and ranks are checked in BANDS of
delta_b = 1e-3 * max_n |s[b, n]| — the project's logits gate — in which no session and no item is left out."""
import copy
import io
import random
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401

from gpu_util import _need_gpu, close
from serve_case import B, N, PANEL, TOPK, reference
from serve_shapes_ref import check_band  # rules (a)-(d)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("scoring", ["f32", "bf16x3-mixed"])
def test_streamed_evaluation_and_recommendation_match_the_oracle_in_bands(scoring):
    _need_gpu()
    from tcar_amd.engine import TcarEngine
    r = reference()
    s, delta, batch, lab = r["s"], r["delta"], r["batch"], r["batch"]["label"]
    eng = TcarEngine(r["params"], r["content"], r["mw"], max_grad=2.0, scoring=scoring)
    _, _, ce_e = eng.eval_step(batch, k=TOPK)
    ce_e = ce_e.cpu().numpy().copy()
    eng.logits.fill_(float("nan"))
    rank, topk, ce = eng.eval_step_streamed(batch, k=TOPK, panel=PANEL)
    rank, topk, ce, scores = rank.cpu().numpy().copy(), topk.cpu().numpy().copy(), ce.cpu().numpy().copy(), eng.last_scores.cpu().numpy().copy()
    assert bool(torch.isnan(eng.logits).all())                    # the step neither needs nor writes the [B, N] matrix
    assert np.isfinite(ce).all() and np.isfinite(scores).all()
    assert topk.shape == (B, TOPK) and topk.dtype == np.int32 and rank.shape == (B,)
    check_band(s, delta, topk, TOPK, name="eval")
    sl = s[np.arange(B), lab]
    others = np.arange(N)[None, :] != lab[:, None]
    lo = 1 + (s > (sl + 2 * delta)[:, None]).sum(1)
    hi = 1 + ((s > (sl - 2 * delta)[:, None]) & others).sum(1)
    assert ((lo <= rank) & (rank <= hi)).all(), (rank, lo, hi)                                              # (e)
    close(scores, np.take_along_axis(s, topk.astype(np.int64), 1), name="scores")                           # (f)
    close(ce, r["ce"], name="ce vs oracle")                                                                 # (g)
    close(ce, ce_e, name="ce vs eval_step")
    # the default panel (one panel here: another launch geometry of the GEMM, so the same bands, not the same bits)
    assert eng.default_panel() == 768
    rank1, topk1, ce1 = eng.eval_step_streamed(batch, k=TOPK)
    check_band(s, delta, topk1.cpu().numpy(), TOPK, name="eval, default panel")
    rank1 = rank1.cpu().numpy()
    assert ((lo <= rank1) & (rank1 <= hi)).all(), (rank1, lo, hi)
    close(ce1.cpu().numpy(), r["ce"], name="ce vs oracle, default panel")

    # recommendation: no label, no negatives in the feed
    feed = {n: v for n, v in batch.items() if n not in ("label", "neg")}
    tk, sc = eng.recommend(feed, k=TOPK, exclude_seen=False, panel=PANEL)
    assert (tk.cpu().numpy() == topk).all() and sc.cpu().numpy().tobytes() == scores.tobytes()
    seen = (batch["seq"] - 1).astype(np.int64)
    tk, sc = eng.recommend(feed, k=TOPK, panel=PANEL)
    tk, sc = tk.cpu().numpy().copy(), sc.cpu().numpy().copy()
    for b in range(B):
        assert not set(tk[b].tolist()) & set(seen[b].tolist()), b
        assert (sc[b, :-1] >= sc[b, 1:]).all(), b
        ties = sc[b, :-1] == sc[b, 1:]
        assert (tk[b, :-1][ties] > tk[b, 1:][ties]).all(), b
    check_band(s, delta, tk, TOPK, gone=seen, name="recommend")
    extra = np.full((B, 5), -1, np.int32)
    extra[:, 0], extra[:, 2], extra[:, 3] = tk[:, 0], tk[:, 7], tk[:, 0]          # the winner (twice) and one from the middle
    tk2, sc2 = eng.recommend(feed, k=TOPK, exclude=extra, panel=PANEL)
    tk2 = tk2.cpu().numpy().copy()
    gone = np.concatenate([seen, extra.astype(np.int64)], 1)
    for b in range(B):
        assert not set(tk2[b].tolist()) & set(gone[b][gone[b] >= 0].tolist()), b
    check_band(s, delta, tk2, TOPK, gone=gone, name="recommend + exclude")
    assert np.isfinite(sc2.cpu().numpy()).all()
    eng.check_forks()


def test_test_loop_with_eval_panel_reports_the_metrics_of_the_materialised_one():
    _need_gpu()
    from tcar_amd.host.model import Seq2SeqAttNN, initial_variables
    from tcar_amd.host.synth import SynthFold
    fold = SynthFold(n_items=400, dim=32, n_train=2500, n_test=400, seed=17, active_t=True)
    tr = fold.to_dicts(fold.train, with_active=True)
    te = fold.to_dicts(fold.test, with_active=True)
    np.random.seed(3)
    init = initial_variables(400, 32, 16, 0.3, 0.1)
    args = fold.model_args(batch_size=64, epoch=1, neg_num=8, hidden_size=32, time_hidden_size=16, lr=0.003,
                           initial_variables=init, emb_stddev=0.3, stddev=0.1, scoring="bf16x3")
    random.seed(5)
    np.random.seed(5)
    model = Seq2SeqAttNN(args)
    got = {}
    with redirect_stdout(io.StringIO()):
        model.train(None, fold.item_dict, (copy.deepcopy(tr[0]), tr[1], tr[2]), {0: [0]}, args,
                    (copy.deepcopy(te[0]), te[1], te[2]), None)
        for panel in (0, 128):
            model.test(None, (copy.deepcopy(te[0]), te[1], te[2]), dict(args, eval_panel=panel))
            got[panel] = dict(model.last_metrics)
    a, b = got[0], got[128]
    assert abs(a["recall"] - b["recall"]) <= 0.002 + 1e-12, (a, b)
    assert abs(a["mrr"] - b["mrr"]) <= 1e-3 * a["mrr"] + 1.0 / 400, (a, b)
    assert abs(a["loss"] - b["loss"]) <= 1e-3 * a["loss"], (a, b)
    assert b["coverage"] > 0 and np.isfinite(b["ild"]) and np.isfinite(b["unexp"])       # the diversity metrics run on the streamed lists
    idx = np.where(fold.test.in_len == 3)[0][:4]
    rec, sc = model.recommend({n: v for n, v in fold.test.batch_arrays(idx, "active_t").items() if n not in ("label", "neg")}, k=5)
    assert tuple(rec.shape) == (len(idx), 5) and tuple(sc.shape) == (len(idx), 5) and len(idx) > 0


def test_eval_panel_with_the_catalog_sharded_mode_is_refused():
    from tcar_amd.host import cli
    from tcar_amd.host.model import Seq2SeqAttNN
    from tcar_amd.host.synth import SynthFold
    check = lambda gpus=1, **values: cli.check_eval_options(values, gpus=gpus)
    with pytest.raises(ValueError, match="eval_panel"):
        check(eval_panel=128, dp_mode="sharded")
    with pytest.raises(ValueError, match="eval_panel"):
        check(eval_panel=100, dp_mode="replica")
    check(eval_panel=0, dp_mode="sharded")
    check(eval_panel=256, dp_mode="replica")
    fold = SynthFold(n_items=60, dim=8, n_train=40, n_test=10, seed=1)
    args = fold.model_args(batch_size=8, epoch=1, neg_num=2, hidden_size=8, time_hidden_size=4, lr=0.003, emb_stddev=0.3, stddev=0.1,
                           eval_panel=128, dp_mode="sharded")
    with pytest.raises(ValueError, match="eval_panel"):
        Seq2SeqAttNN(args)
