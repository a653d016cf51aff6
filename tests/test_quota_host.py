"""Host side of the per-category caps (include/tcar_quota.h): the bindings generated from the header, the argument checks, which answer
before anything is launched, the trainer's refusals, the accuracy of a list from the label's place in it, and the numpy model of the
capped walk that the GPU tests compare with — none of it needs a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tcar_amd  # noqa: F401
from tcar_amd import _lib

from select_ref import capped_walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOTYPE = r"^((?:const )?\w+\*?) (tcar_\w+)\(([^)]*)\)\s*;"


def test_the_quota_header_is_parsed_and_bound():
    with open(os.path.join(ROOT, "include", "tcar_quota.h")) as f:
        header = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    lib = _lib.load()
    assert lib.tcar_quota_abi_version() == _lib.QUOTA_ABI_VERSION == 1
    assert _lib.QUOTA_HEADER in _lib.HEADERS                       # the header enters the build id
    protos = re.findall(PROTOTYPE, header, flags=re.M)
    assert [name for _, name, _ in protos] == _lib.QUOTA_SYMBOLS == ["tcar_quota_abi_version", "tcar_select_panel_quota",
                                                                      "tcar_serve_step_quota"]
    assert not set(_lib.QUOTA_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.SERVE_SYMBOLS) | set(_lib.WINDOW_SYMBOLS))
    i32, vp = C.c_int32, C.c_void_p
    assert lib.tcar_select_panel_quota.argtypes == lib.tcar_select_panel_window.argtypes + [vp, i32]
    assert lib.tcar_serve_step_quota.argtypes == [C.POINTER(_lib.Ctx), C.POINTER(_lib.Batch), i32, C.POINTER(_lib.Serve),
                                                  C.POINTER(_lib.Window), C.POINTER(_lib.Quota), vp]
    assert lib.tcar_select_panel_quota.restype is C.c_int and lib.tcar_serve_step_quota.restype is C.c_int
    m = _lib.Quota
    assert [f[0] for f in m._fields_] == ["cat", "cap"]
    assert (m.cat.offset, m.cat.size, m.cap.offset, m.cap.size, C.sizeof(m)) == (0, 8, 8, 4, 16)
    # everything new lives in tcar_quota.h: the other headers' numbers are where they were
    assert _lib.ABI_VERSION == 30 and _lib.SERVE_ABI_VERSION == 1 and _lib.WINDOW_ABI_VERSION == 1
    assert len(_lib.SYMBOLS) == 112 and len(_lib.SERVE_SYMBOLS) == 6 and len(_lib.WINDOW_SYMBOLS) == 3


def test_cap_argument_errors_come_back_before_any_launch():
    lib = _lib.load()
    buf = (C.c_float * 4096)()                    # host memory: never dereferenced, an accepted call would have to launch
    p = C.cast(buf, C.c_void_p)
    names = ("B", "n0", "n", "panel", "ld", "k", "label", "lab_score", "excl", "X", "state", "stream", "key", "lo", "hi", "cat", "cap")
    base = dict(B=2, n0=0, n=128, panel=p, ld=128, k=20, label=None, lab_score=None, excl=None, X=0, state=p, stream=None,
                key=None, lo=None, hi=None, cat=p, cap=2)
    panel = lambda **kw: lib.tcar_select_panel_quota(*[dict(base, **kw)[a] for a in names])
    assert panel(cap=0) == -1 and panel(cap=-1) == -1             # a table with no cap
    assert panel(cat=None) == -1 and panel(cat=None, cap=20) == -1         # a cap with no table
    assert panel(B=0, cap=0) == -1 and panel(B=0, cat=None) == -1          # (an argument error is one at B == 0 too)
    assert panel(B=0) == 0 and panel(B=0, cat=None, cap=0) == 0
    for win in (dict(), dict(key=p, lo=p, hi=p)):                  # the errors of the uncapped call, with a cap
        call = lambda **kw: panel(**dict(win, **kw))
        assert call(k=65) == -1 and call(k=0) == -1 and call(ld=130) == -1 and call(ld=64) == -1 and call(n0=-1) == -1
        assert call(state=None) == -1 and call(panel=None) == -1 and call(lab_score=p) == -1 and call(excl=p, X=0) == -1
    assert panel(key=p) == -1                                      # key without lo / hi

    ctx, bt, s, q = _lib.Ctx(), _lib.Batch(), _lib.Serve(), _lib.Quota()
    bt.B, bt.T = 2, 3
    s.k, s.panel, s.panel_buf, s.state, s.state_bytes, s.topk = 20, 256, p.value, p.value, 4096 * 4, p.value
    step = lambda: lib.tcar_serve_step_quota(C.byref(ctx), C.byref(bt), 0, C.byref(s), None, C.byref(q), None)
    for cat, cap in ((p.value, 0), (p.value, -3), (None, 2), (None, 0)):           # a descriptor names a table AND a cap >= 1
        q.cat, q.cap = cat, cap
        assert step() == -1, (cat, cap)
        bt.B = 0
        assert step() == -1, (cat, cap)
        bt.B = 2
    q.cat, q.cap = p.value, 2
    assert step() == -1                                            # an empty context (no parameters): still before any launch
    bt.B = 0
    assert step() == 0


def test_cat_cap_is_refused_where_it_cannot_work():
    from tcar_amd.host import cli
    from tcar_amd.host.model import Seq2SeqAttNN
    from tcar_amd.host.synth import SynthFold
    check = lambda gpus=1, **values: cli.check_eval_options(values, gpus=gpus)
    with pytest.raises(ValueError, match="cat_cap"):
        check(cat_cap=-1, eval_panel=128, dp_mode="replica")
    with pytest.raises(ValueError, match="eval_panel"):
        check(cat_cap=2, eval_panel=0, dp_mode="replica")
    with pytest.raises(ValueError, match="sharded"):
        check(cat_cap=2, eval_panel=128, dp_mode="sharded")
    check(cat_cap=0, eval_panel=0, dp_mode="sharded")
    check(cat_cap=0, eval_panel=0, dp_mode="replica")
    check(cat_cap=2, eval_panel=128, dp_mode="replica")
    assert cli.build_parser().parse_args([]).cat_cap == 0
    a = cli.build_parser().parse_args(["--cat_cap", "3", "--eval_panel", "128", "--fresh_hours", "48"])
    assert a.cat_cap == 3 and a.fresh_hours == 48
    fold = SynthFold(n_items=60, dim=8, n_train=40, n_test=10, seed=1)
    small = dict(batch_size=8, epoch=1, neg_num=2, hidden_size=8, time_hidden_size=4, lr=0.003, emb_stddev=0.3, stddev=0.1)
    with pytest.raises(ValueError, match="eval_panel"):
        Seq2SeqAttNN(fold.model_args(cat_cap=2, **small))
    with pytest.raises(ValueError, match="sharded"):
        Seq2SeqAttNN(fold.model_args(cat_cap=2, eval_panel=128, dp_mode="sharded", **small))


def test_list_metrics_from_the_place_of_the_label():
    from tcar_amd.host import metrics as M
    topk = np.full((4, 20), -1, np.int64)
    topk[0] = np.arange(100, 120)
    topk[1] = np.arange(100, 120)
    topk[2] = np.arange(100, 120)
    topk[3, :3] = [7, 8, 9]                                        # a short list
    labels = np.array([100, 119, 5, 9])
    ranks = M.list_ranks(topk, labels, 20)
    assert ranks.tolist() == [1, 20, 21, 3]                        # place 0, place 19, absent, place 2 of a short list
    hit, mrr, ndcg = M.metrics_from_ranks(ranks, 20)
    assert hit.tolist() == [True, True, False, True]
    assert mrr.tolist() == [1.0, 1.0 / 20, 0.0, 1.0 / 3]
    assert ndcg.tolist() == [1.0, 1.0 / np.log2(21.0), 0.0, 0.5]
    assert M.list_ranks(np.full((1, 20), -1), np.array([0]), 20).tolist() == [21]


def test_capped_walk_on_hand_made_rows():
    # the threshold example: the three best share category a, so the list reaches below the k-th best score
    scores = np.array([10, 9, 8, 1, 0.5], np.float32)
    cat = np.array([7, 7, 7, -2, 2 ** 31 - 1], np.int32)
    assert capped_walk(scores, cat, 3, 1) == [0, 3, 4]
    assert capped_walk(scores, cat, 3, 2) == [0, 1, 3]
    assert capped_walk(scores, cat, 3, 3) == [0, 1, 2] == capped_walk(scores, cat, 3, 99)
    assert capped_walk(scores, cat, 1, 1) == [0]
    # ties go by id, descending, and the cap counts along that order
    scores = np.array([1, 1, 1, 1, 1, 2], np.float32)
    cat = np.array([0, 1, 0, 1, 0, 1], np.int32)
    assert capped_walk(scores, cat, 4, 1) == [5, 4]                # category 1 is spent by item 5, category 0 by item 4
    assert capped_walk(scores, cat, 4, 2) == [5, 4, 3, 2]
    assert capped_walk(scores, cat, 6, 3) == [5, 4, 3, 2, 1, 0]
    # a short list when #categories * m < k
    cat = np.array([0, 0, 0, 5, 5, 5], np.int32)
    scores = np.array([6, 5, 4, 3, 2, 1], np.float32)
    assert capped_walk(scores, cat, 5, 2) == [0, 1, 3, 4]
    assert capped_walk(scores, cat, 5, 1) == [0, 3]
    # items that are not eligible do not exist: they consume no quota
    assert capped_walk(scores, cat, 5, 1, eligible=[False, True, True, False, False, True]) == [1, 5]
    assert capped_walk(scores, cat, 5, 2, eligible=np.zeros(6, bool)) == []
