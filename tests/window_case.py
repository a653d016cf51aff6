"""What the tests of publish-time windows and of per-category caps share (test_gpu_window_serve.py, test_gpu_quota_serve.py,
test_gpu_ragged_serve.py): the N = 700 serving case with item keys and per-session windows and the fp64 oracle's logits of it, the
band checks restricted to a session's POOL — the items whose key lies in its window, and its label — and two small trained models
with the test loop run on them.  Computed once, shared, never written."""
import copy
import datetime
import io
import random
from contextlib import redirect_stdout

import numpy as np

from gpu_util import close

N, H, Ht, B, T, K = 700, 250, 64, 41, 3, 5
PANEL, TOPK = 256, 20                             # three panels, the last one partial
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


_REF = {}


def reference():
    """inputs, item keys, windows and the oracle's fp64 logits: computed once, shared, never written"""
    if not _REF:
        from oracle.tcar_oracle import TcarOracle, init_params_numpy
        rng = np.random.RandomState(17)
        params = init_params_numpy(N, H, Ht, 0.35, 0.12, rng)
        content = (rng.standard_normal((N + 1, H)) * 0.5).astype(np.float32)
        content[0] = 0
        mw = np.stack([rng.randint(1, 13, N), rng.randint(1, 32, N), rng.randint(1, 8, N), rng.randint(1, 25, N),
                       rng.randint(1, 61, N)], -1).astype(np.int32)
        b = {"seq": rng.randint(1, N + 1, (B, T)), "label": rng.randint(0, N, B), "pm": rng.randint(1, 13, (B, T)),
             "pd": rng.randint(1, 32, (B, T)), "pw": rng.randint(1, 8, (B, T)), "ph": rng.randint(1, 25, (B, T)),
             "pmi": rng.randint(1, 61, (B, T)), "cw": rng.randint(0, 7, B), "ch": rng.randint(0, 24, B),
             "gap": rng.randint(0, 12, (B, T)), "neg": rng.randint(0, N, (B, K))}
        b = {k: v.astype(np.int32) for k, v in b.items()}
        b["seq"][0, 1] = b["seq"][0, 0]
        logits, _ = TcarOracle(params, content, mw).eval_batch(b)
        s = logits.numpy().astype(np.float64)
        key = (np.random.RandomState(3).permutation(N) * 3 - 1000).astype(np.int32)      # distinct, a third of them negative
        # session b takes window b % 4: the whole catalog | about a third of it | seven items | none
        srt = np.sort(key)
        kinds = [(I32_MIN, I32_MAX), (int(srt[200]), int(srt[433])), (int(srt[300]), int(srt[307])), (40, 40)]
        lo = np.array([kinds[i % 4][0] for i in range(B)], np.int64)
        hi = np.array([kinds[i % 4][1] for i in range(B)], np.int64)
        win = (lo[:, None] <= key[None, :]) & (key[None, :] < hi[:, None])
        assert win[0].sum() == N and win[1].sum() == 233 and win[2].sum() == 7 and win[3].sum() == 0, ("pool sizes", win[:4].sum(1))
        for a in list(b.values()) + [s, key, lo, hi, win]:
            a.setflags(write=False)
        _REF.update(params=params, content=content, mw=mw, batch=b, s=s, delta=1e-3 * np.abs(s).max(1), key=key, lo=lo, hi=hi, win=win)
    return _REF


def check_band(s, delta, topk, k, pool, name=""):
    """(a)-(d) of serve_shapes_ref.check_band inside the pool: min(k, |pool|) distinct pool items and then -1 only, sorted within
    2 delta, everything clearly above the k-th pool score in, nothing clearly below"""
    for b in range(s.shape[0]):
        row, d2 = np.where(pool[b], s[b], -np.inf), 2 * delta[b]
        n = min(k, int(pool[b].sum()))
        t = topk[b, :n].astype(np.int64)
        assert (topk[b, n:] == -1).all() and (t >= 0).all() and len(set(t.tolist())) == n and pool[b][t].all(), (name, b, topk[b])   # (a)
        if n == 0:
            continue
        assert (row[t[:-1]] >= row[t[1:]] - d2).all(), (name, b)                                            # (b)
        kth = np.sort(row)[-n]
        assert set(np.where(row > kth + d2)[0].tolist()) <= set(t.tolist()), (name, b)                      # (c)
        assert (row[t] >= kth - d2).all(), (name, b)                                                        # (d)


def check_eval(r, pool, rank, topk, ce, scores, name):
    s, delta, lab = r["s"], r["delta"], r["batch"]["label"]
    assert np.isfinite(ce).all(), name
    check_band(s, delta, topk, TOPK, pool, name=name)
    sl = s[np.arange(B), lab]
    others = np.arange(N)[None, :] != lab[:, None]
    lo = 1 + ((s > (sl + 2 * delta)[:, None]) & pool).sum(1)
    hi = 1 + ((s > (sl - 2 * delta)[:, None]) & others & pool).sum(1)
    assert ((lo <= rank) & (rank <= hi)).all(), (name, rank, lo, hi)                                        # (e)
    valid = topk >= 0
    close(scores[valid], np.take_along_axis(s, np.maximum(topk, 0).astype(np.int64), 1)[valid], name=name + " scores")      # (f)
    sp = np.where(pool, s, -np.inf)
    lse = np.log(np.exp(sp - sp.max(1, keepdims=True)).sum(1)) + sp.max(1)
    close(ce, lse - sl, name=name + " ce vs the oracle's log-sum-exp over the pool")                        # (g)


_TRAINED = {}


def trained():
    """a small SynthFold (400 items) and two models trained on it for one epoch from the same seeds: one whose items are all published
    before the first click (publish times moved back 20 days), one with the fold's own publish times"""
    if not _TRAINED:
        from tcar_amd.host.model import Seq2SeqAttNN, initial_variables
        from tcar_amd.host.synth import SynthFold
        fold = SynthFold(n_items=400, dim=32, n_train=1500, n_test=300, seed=17, active_t=True)
        tr = fold.to_dicts(fold.train, with_active=True)
        te = fold.to_dicts(fold.test, with_active=True)
        own = [t.astype("datetime64[s]").item() for t in fold.publish_ts]
        early = [t - datetime.timedelta(days=20) for t in own]
        assert max(early) < min(d["click_t"] for tl in te[2].values() for d in tl), ("an item is published after the first click", max(early))
        models = {}
        for name, times in (("early", early), ("own", own)):
            np.random.seed(3)
            init = initial_variables(400, 32, 16, 0.3, 0.1)
            args = fold.model_args(batch_size=64, epoch=1, neg_num=8, hidden_size=32, time_hidden_size=16, lr=0.003,
                                   initial_variables=init, emb_stddev=0.3, stddev=0.1, scoring="bf16x3", eval_panel=128,
                                   publish_time=times)
            random.seed(5)
            np.random.seed(5)
            model = Seq2SeqAttNN(args)
            with redirect_stdout(io.StringIO()):
                model.train(None, fold.item_dict, (copy.deepcopy(tr[0]), tr[1], tr[2]), {0: [0]}, args, None, None)
            models[name] = (model, args)
        _TRAINED.update(fold=fold, te=te, models=models, own=own)
    return _TRAINED


def run_test(model, te, args):
    random.seed(11)                               # the sampler shuffles: the same batches in every run
    out = io.StringIO()
    with redirect_stdout(out):
        model.test(None, (copy.deepcopy(te[0]), te[1], te[2]), args)
    return dict(model.last_metrics), out.getvalue()
