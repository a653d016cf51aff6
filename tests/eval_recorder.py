"""A recording stand-in for the engine under `Seq2SeqAttNN.test()`: every engine call the evaluation loop makes is written down as
one line — the method and the arguments that tell one call from another — and answered with CPU tensors of the right shapes and
deterministic values.  With a model built by `__new__` over a small synthetic fold this shows the ORDER of the loop's engine calls
on a machine without a GPU (tests/test_eval_passes_host.py)."""
import copy
import random
from collections import namedtuple

import numpy as np
import torch

K = 20
_Bt = namedtuple("_Bt", "B lens")
_Cand = namedtuple("_Cand", "counts metrics")
_Sections = namedtuple("_Sections", "topk scores")


def _win(window):
    return "none" if window is None else "[%d]" % len(np.asarray(window[0]).reshape(-1))


def _feed(feed):
    if "len" in feed:
        return "ragged B=%d R=%d" % (len(feed["len"]), len(feed["seq"]))
    return "B=%d T=%d" % tuple(np.asarray(feed["seq"]).shape)


class RecordingEngine:
    """the engine calls of test() for dp_world == 1, recorded in `calls`"""
    dev = "cpu"

    def __init__(self, n_items, content):
        self.N, self._content, self.calls, self._n = int(n_items), content, [], 0

    def _lists(self, B, k=K):
        """[B, k] int32 lists of k distinct items each, different from call to call"""
        self._n += 1
        step = max(self.N // k, 1)
        return torch.from_numpy(((np.arange(k)[None, :] * step + np.arange(B)[:, None] + 7 * self._n) % self.N).astype(np.int32))

    def set_item_keys(self, keys):
        self.calls.append("set_item_keys")

    def set_categories(self, cat):
        self.calls.append("set_categories")

    def reset_coverage(self):
        self.calls.append("reset_coverage")

    def upload(self, feed):
        self.calls.append("upload " + _feed(feed))
        return _Bt(len(feed["label"]), feed.get("len"))

    def eval_step(self, batch, k=K, bt=None):
        self.calls.append("eval_step B=%d" % bt.B)
        return self._streamed(bt.B, k)

    def eval_step_streamed(self, batch, k=K, bt=None, panel=None, window=None, max_per_category=None):
        self.calls.append("eval_step_streamed B=%d panel=%s window=%s max_per_category=%s" % (bt.B, panel, _win(window), max_per_category))
        return self._streamed(bt.B, k)

    def _streamed(self, B, k):
        topk = self._lists(B, k)
        rank = torch.from_numpy(((np.arange(B) * 5 + self._n) % 31 + 1).astype(np.int32))
        return rank, topk, torch.from_numpy((0.25 * np.arange(B) + self._n).astype(np.float32))

    def eval_diversity(self, bt, topk, block=None):
        self.calls.append("eval_diversity lists=%d block=%s" % (topk.shape[0], None if block is None else tuple(int(v) for v in block)))
        B = topk.shape[0]
        return (torch.arange(B, dtype=torch.int32) % 7 + 300, torch.arange(B, dtype=torch.int32) % 5, torch.full((B,), K, dtype=torch.int32))

    def score_candidates(self, batch, candidates, clicked=None, bt=None):
        B, C = candidates.shape
        assert (candidates[:, 0] >= 0).all() and clicked[:, 0].all() and int(clicked.sum()) == B
        self.calls.append("score_candidates B=%d C=%d" % (B, C))
        self._n += 1
        counts = np.stack([np.ones(B), np.full(B, C - 1), (np.arange(B) + self._n) % (2 * C - 1)], 1).astype(np.int32)
        return _Cand(torch.from_numpy(counts), torch.from_numpy(np.tile([0.5, 0.25, 0.125], (B, 1)).astype(np.float32) / self._n))

    def recommend_two_stage(self, batch, k=K, shortlist=256, exclude_seen=True, panel=None, window=None, diversity=None):
        assert "label" not in batch and "neg" not in batch
        self.calls.append("recommend_two_stage %s shortlist=%d exclude_seen=%s panel=%s window=%s diversity=%s"
                          % (_feed(batch), shortlist, exclude_seen, panel, _win(window), diversity))
        B = np.asarray(batch["seq"]).shape[0]
        return self._lists(B, k), torch.zeros(B, k)

    def recommend_sections(self, batch, sections, k=10, exclude_seen=True, panel=None, window=None):
        assert "label" not in batch and "neg" not in batch
        self.calls.append("recommend_sections %s G=%d k=%d exclude_seen=%s panel=%s window=%s"
                          % (_feed(batch), len(sections), k, exclude_seen, panel, _win(window)))
        B = len(batch["len"]) if "len" in batch else np.asarray(batch["seq"]).shape[0]
        topk = torch.stack([self._lists(B, k) for _ in range(len(sections))], 1)
        return _Sections(topk, torch.zeros(topk.shape))

    def similar_items(self, ids=None, k=K):
        self.calls.append("similar_items Q=%d k=%d" % (len(ids), k))
        return self._lists(len(ids), k), torch.full((len(ids), k), 0.5)

    def check_forks(self):
        self.calls.append("check_forks")

    def coverage(self):
        self.calls.append("coverage")
        return 17


def fold_and_data(n_long=10, n_short=5):
    """a 60-item fold and, of its test sessions, `n_long` of one length and `n_short` of another in the dict form test() takes:
    with a batch size of 8 the feeds hold 8, 2 and 5 sessions, so eval_mixed has two of them to pack"""
    from tcar_amd.host.synth import SynthFold
    fold = SynthFold(n_items=60, dim=8, n_train=40, n_test=60, seed=1, n_categories=6)
    lens = fold.test.in_len
    a, b = [int(t) for t in np.unique(lens)[:2]]
    rows = np.where(lens == a)[0][:n_long].tolist() + np.where(lens == b)[0][:n_short].tolist()
    assert len(rows) == n_long + n_short
    return fold, fold.to_dicts(fold.test, examples=rows)


def recorded_test(model_cls, fold, data, seed=3, **flags):
    """model_cls.test() over `data` on a RecordingEngine, the model built with __new__ -> (engine calls, last_metrics, return value)"""
    m = model_cls.__new__(model_cls)
    times = [t.astype("datetime64[s]").item() for t in fold.publish_ts]
    a = fold.model_args(publish_time=times, batch_size=8, **flags)
    m.candidate_n, m.publish_time, m._keys, m._key_t0 = fold.n_items + 1, times, None, None
    m.batch_size, m.seed, m.curEpoch = 8, 2020, 0
    m.reverse_item, m.category_id, m._cat, m.gap_mode, m.neg_mode, m.neg_fast = a["reverse_item"], a["category_id"], None, "active_t", "uniform", False
    m.dp_world, m.dp_rank, m.dp_group = 1, 0, None
    m.engine = RecordingEngine(fold.n_items, fold.content)
    random.seed(seed)                              # (the sampler shuffles its batches with the global stream, and its lists in place)
    recall = m.test(None, copy.deepcopy(data), a)
    return m.engine.calls, m.last_metrics, recall
