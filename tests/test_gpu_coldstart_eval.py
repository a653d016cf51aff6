"""test() with --eval_coldstart on the GPU (host/eval_passes.py: ColdStart; include/tcar_warm.h): a SynthFold of 400 items, two models
trained for a few steps from the same seeds.  Model A runs the plain streamed test(), then test() with eval_coldstart 0.25 and 8
donors; model B the plain test() twice.  Then both take one training step.

  * the line and last_metrics["coldstart"] exist; A / K are the sampled / requested counts, and the sample is cold_sample of the
    split's labels and the model's seed;
  * the "trained" figures are the normal pass restricted to the sessions whose label is sampled — recomputed here from the ranks of
    eval_step_streamed over the same feeds;
  * every buffer the pass wrote — E, the planes, Mi / Vi — and the whole exported state hold the bytes they held before;
  * nothing else of test() moves: the core metrics with the option are those without it;
  * the training step of A gives the bits of the training step of B: loss and exported state.
No accuracy ordering between zeroed and warm-started rows is asserted on synthetic data: the number belongs to a real fold."""
import copy
import io
import random
import re
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401

from gpu_util import _need_gpu

pytestmark = pytest.mark.gpu

FRAC, DONORS, PANEL = 0.25, 8, 128
CORE = ["mrr", "recall", "ndcg", "loss", "ild", "unexp", "coverage", "eval_calls", "sessions"]
_RUN = {}


def _model(fold, tr):
    from tcar_amd.host.model import Seq2SeqAttNN, initial_variables
    np.random.seed(3)
    init = initial_variables(400, 32, 16, 0.3, 0.1)
    own = [t.astype("datetime64[s]").item() for t in fold.publish_ts]
    args = fold.model_args(batch_size=64, epoch=1, neg_num=8, hidden_size=32, time_hidden_size=16, lr=0.003, initial_variables=init,
                           emb_stddev=0.3, stddev=0.1, scoring="bf16x3", eval_panel=PANEL, publish_time=own, seed=77)
    random.seed(5)
    np.random.seed(5)
    model = Seq2SeqAttNN(args)
    with redirect_stdout(io.StringIO()):
        model.train(None, fold.item_dict, (copy.deepcopy(tr[0]), tr[1], tr[2]), {0: [0]}, args, None, None)
    return model, args


def _test(model, te, args):
    random.seed(11)                               # the sampler shuffles: the same batches in every run
    out = io.StringIO()
    with redirect_stdout(out):
        model.test(None, (copy.deepcopy(te[0]), te[1], te[2]), args)
    return dict(model.last_metrics), out.getvalue()


def _buffers(eng):
    eng.flush()
    return {n: getattr(eng, n).cpu().view(-1).view(torch.uint8).numpy().copy() for n in ("E", "e16h", "e16l", "Mi", "Vi")}


def _ranks(model, te):
    """the streamed evaluation of every feed of the split, as test() draws them -> (ranks, labels) per session"""
    random.seed(11)
    sampler = model._sampler((copy.deepcopy(te[0]), te[1], te[2]))
    ranks, labels = [], []
    while sampler.has_next():
        feed = sampler.next_batch_arrays()
        rank, _, _ = model.engine.eval_step_streamed(None, k=20, bt=model.engine.upload(feed), panel=PANEL)
        ranks.append(rank.cpu().numpy().copy())
        labels.append(np.asarray(feed["label"], dtype=np.int64).reshape(-1))
    return np.concatenate(ranks), np.concatenate(labels)


def _run():
    if not _RUN:
        _need_gpu()
        from tcar_amd.host.synth import SynthFold
        fold = SynthFold(n_items=400, dim=32, n_train=320, n_test=200, seed=17, active_t=True)
        tr, te = fold.to_dicts(fold.train, with_active=True), fold.to_dicts(fold.test, with_active=True)
        (a, args), (b, _) = _model(fold, tr), _model(fold, tr)
        step = a._sampler((copy.deepcopy(tr[0]), tr[1], tr[2]), {0: [0]}, fold.item_dict, 8)
        random.seed(2)
        np.random.seed(2)
        batch = step.next_batch_arrays()
        ranks, labels = _ranks(a, te)
        plain, plain_text = _test(a, te, args)
        before, state_before = _buffers(a.engine), a.engine.export_state()
        cold, text = _test(a, te, dict(args, coldstart=FRAC, coldstart_donors=DONORS))
        after, state_after = _buffers(a.engine), a.engine.export_state()
        _test(b, te, args)
        _test(b, te, args)
        la, lb = a.engine.train_step(batch).cpu().numpy().copy(), b.engine.train_step(batch).cpu().numpy().copy()
        a.engine.flush()
        b.engine.flush()
        _RUN.update(model=a, plain_text=plain_text, ranks=ranks, labels=labels, plain=plain, cold=cold, text=text, before=before, after=after,
                    state_before=state_before, state_after=state_after, la=la, lb=lb, sa=a.engine.export_state(), sb=b.engine.export_state())
        a.engine.check_forks()
        b.engine.check_forks()
    return _RUN


def test_the_line_and_the_metrics_name_the_sample_and_the_donors():
    from tcar_amd.host.eval_passes import cold_sample
    r = _run()
    lines = [ln for ln in r["text"].splitlines() if ln.startswith("cold start")]
    assert len(lines) == 1 and r["text"].splitlines()[-1] == lines[0]                       # one more line, behind every other
    m = re.match(r"^cold start \((\d+) articles, (\d+) donors\): Recall@20 trained (\S+), zeroed (\S+), warm-started (\S+); "
                 r"MRR@20 (\S+), (\S+), (\S+)$", lines[0])
    assert m, lines[0]
    c = r["cold"]["coldstart"]
    sample = cold_sample(r["labels"], FRAC, r["model"].seed)
    distinct = len(np.unique(r["labels"]))
    assert int(m.group(1)) == c["articles"] == len(sample) == int(round(FRAC * distinct)) and int(m.group(2)) == c["donors"] == DONORS
    assert c["sample"] == sample.tolist() and c["sessions"] == int(np.isin(r["labels"], sample).sum()) > 0
    got = [float(x) for x in m.groups()[2:]]
    assert got == [c["recall"][n] for n in ("trained", "zeroed", "warm")] + [c["mrr"][n] for n in ("trained", "zeroed", "warm")]
    assert all(0.0 <= v <= 1.0 for v in got)
    assert "coldstart" not in r["plain"] and "cold start" not in r["plain_text"]
    assert r["text"].splitlines()[:-1] == r["plain_text"].splitlines()                     # every other line is the plain loop's


def test_the_trained_figures_are_the_normal_pass_restricted_to_the_sampled_sessions():
    from tcar_amd.host import metrics as M
    from tcar_amd.host.eval_passes import cold_sample
    r = _run()
    sample = cold_sample(r["labels"], FRAC, r["model"].seed)
    hits, mrr, _ = M.metrics_from_ranks(r["ranks"][np.isin(r["labels"], sample)], 20)
    c = r["cold"]["coldstart"]
    assert c["recall"]["trained"] == pytest.approx(float(np.mean(hits)), rel=1e-12, abs=0)
    assert c["mrr"]["trained"] == pytest.approx(float(np.mean(mrr)), rel=1e-12, abs=0)
    # and the whole pass is the plain loop's: the option changes nothing else of test()
    hits_all, mrr_all, _ = M.metrics_from_ranks(r["ranks"], 20)
    assert r["plain"]["recall"] == pytest.approx(float(np.mean(hits_all)), rel=1e-12) and r["plain"]["sessions"] == len(r["ranks"])
    assert [r["cold"][k] for k in CORE] == [r["plain"][k] for k in CORE]
    assert list(r["cold"]) == list(r["plain"]) + ["coldstart"]


def test_the_engine_is_left_byte_for_byte_as_found():
    r = _run()
    for name in ("E", "e16h", "e16l", "Mi", "Vi"):
        assert r["before"][name].tobytes() == r["after"][name].tobytes(), name
    assert r["before"]["Mi"].any() and r["before"]["E"].any()                              # (a trained engine: there was something to keep)
    assert sorted(r["state_before"]) == sorted(r["state_after"])
    differ = [k for k in r["state_before"] if np.asarray(r["state_before"][k]).tobytes() != np.asarray(r["state_after"][k]).tobytes()]
    assert not differ, differ


def test_a_training_step_after_it_is_the_step_without_the_option():
    r = _run()
    assert r["la"].tobytes() == r["lb"].tobytes()
    assert sorted(r["sa"]) == sorted(r["sb"])
    differ = [k for k in r["sa"] if np.asarray(r["sa"][k]).tobytes() != np.asarray(r["sb"][k]).tobytes()]
    assert not differ, differ
