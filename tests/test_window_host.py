"""Host side of the publish-time windows (include/tcar_window.h): the bindings generated from the header, the layout of the struct
mirror, the argument checks, which answer before anything is launched, and the trainer's refusals — none of it needs a GPU."""
import ctypes as C
import datetime
import os
import re
import subprocess

import pytest

import tcar_amd  # noqa: F401
from tcar_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOTYPE = r"^((?:const )?\w+\*?) (tcar_\w+)\(([^)]*)\)\s*;"


def _header():
    with open(os.path.join(ROOT, "include", "tcar_window.h")) as f:
        return re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)


def test_every_prototype_of_the_window_header_is_bound():
    lib = _lib.load()
    protos = re.findall(PROTOTYPE, _header(), flags=re.M)
    assert [name for _, name, _ in protos] == _lib.WINDOW_SYMBOLS
    assert _lib.WINDOW_SYMBOLS == ["tcar_window_abi_version", "tcar_select_panel_window", "tcar_serve_step_window"]
    assert not set(_lib.WINDOW_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.SERVE_SYMBOLS))
    for ret, name, params in protos:
        f = getattr(lib, name)
        n = 0 if params.strip() == "void" else params.count(",") + 1
        assert f.argtypes is not None and len(f.argtypes) == n, (name, n)
        assert f.restype is C.c_int and ret == "int", name
    i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
    assert lib.tcar_select_panel_window.argtypes == lib.tcar_select_panel.argtypes + [vp, vp, vp]
    assert lib.tcar_select_panel_window.argtypes == [i32, i32, i32, vp, i64, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp]
    assert lib.tcar_serve_step_window.argtypes == [C.POINTER(_lib.Ctx), C.POINTER(_lib.Batch), i32, C.POINTER(_lib.Serve),
                                                   C.POINTER(_lib.Window), vp]


def test_window_abi_version_and_the_unchanged_other_abis():
    lib = _lib.load()
    assert lib.tcar_window_abi_version() == _lib.WINDOW_ABI_VERSION == 1
    assert _lib.WINDOW_HEADER in _lib.HEADERS                      # the header enters the build id
    # everything new lives in tcar_window.h: the other two headers' numbers are where they were
    assert _lib.ABI_VERSION == 30 and len(_lib.SYMBOLS) == 112 and _lib.SERVE_ABI_VERSION == 1 and len(_lib.SERVE_SYMBOLS) == 6


def test_window_mirror_has_the_layout_the_compiler_gives_the_header(tmp_path):
    """a host-only C++ program that includes the header prints sizeof / offsetof of every field the parser named"""
    m = _lib.Window
    assert [f[0] for f in m._fields_] == ["key", "lo", "hi"]
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "tcar_window.h"', 'int main() {',
             '  printf("%zu\\n", sizeof(tcar_window_t));']
    lines += ['  printf("%%zu %%zu\\n", offsetof(tcar_window_t, %s), sizeof(((tcar_window_t*)0)->%s));' % (f[0], f[0]) for f in m._fields_]
    lines.append('  return 0;\n}')
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([_lib._hipcc(), "-x", "c++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = iter(subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE).stdout.decode().split("\n"))
    assert int(next(got)) == C.sizeof(m)
    for f in m._fields_:
        d = getattr(m, f[0])
        assert next(got).split() == [str(d.offset), str(d.size)], f[0]


def test_argument_errors_come_back_before_any_launch():
    lib = _lib.load()
    buf = (C.c_float * 4096)()                    # host memory: never dereferenced, an accepted call would have to launch
    p = C.cast(buf, C.c_void_p)
    B, k = 2, 20
    names = ("B", "n0", "n", "panel", "ld", "k", "label", "lab_score", "excl", "X", "state", "stream", "key", "lo", "hi")
    base = dict(B=B, n0=0, n=128, panel=p, ld=128, k=k, label=None, lab_score=None, excl=None, X=0, state=p, stream=None,
                key=p, lo=p, hi=p)
    panel = lambda **kw: lib.tcar_select_panel_window(*[dict(base, **kw)[a] for a in names])
    # the window's own errors: key without lo / hi, and the reverse
    assert panel(lo=None) == -1 and panel(hi=None) == -1 and panel(lo=None, hi=None) == -1
    assert panel(key=None) == -1 and panel(key=None, lo=None) == -1 and panel(key=None, hi=None) == -1
    # every error of the unwindowed call, with a window and without one
    for win in (dict(), dict(key=None, lo=None, hi=None)):
        call = lambda **kw: panel(**dict(win, **kw))
        assert call(k=65) == -1 and call(k=0) == -1
        assert call(n=49153, ld=49156) == -1
        assert call(ld=130) == -1                    # ld % 4
        assert call(ld=64) == -1                     # ld < n
        assert call(n0=-1) == -1
        assert call(state=None) == -1
        assert call(panel=None) == -1
        assert call(lab_score=p) == -1               # lab_score without label
        assert call(excl=p, X=0) == -1
        assert call(X=-1) == -1
        # B == 0: nothing to do
        assert call(B=0) == 0 and call(B=0, state=None, panel=None) == 0
    assert panel(B=0, lo=None) == -1                 # (an argument error is one at B == 0 too)

    ctx, bt, s, w = _lib.Ctx(), _lib.Batch(), _lib.Serve(), _lib.Window()
    bt.B, bt.T = B, 3
    s.k, s.panel, s.panel_buf, s.state, s.state_bytes, s.topk = k, 256, p.value, p.value, 4096 * 4, p.value
    w.key, w.lo, w.hi = p.value, p.value, p.value
    for win in (C.byref(w), None):
        step = lambda: lib.tcar_serve_step_window(C.byref(ctx), C.byref(bt), 0, C.byref(s), win, None)
        for bad in (100, 0, -128, 49152 + 128):       # panel % 128, panel out of range
            s.panel = bad
            assert step() == -1, bad
        s.panel = 256
        s.k = 65
        assert step() == -1
        s.k = k
        s.state_bytes = B * (2 * k + 4) * 4 - 1
        assert step() == -1
        s.state_bytes = 4096 * 4
        s.state = None
        assert step() == -1
        s.state = p.value
        bt.label = p.value                            # evaluation needs the lab_score workspace
        assert step() == -1
        bt.label = None
        assert step() == -1                           # an empty context (no parameters): still before any launch
        assert lib.tcar_serve_step_window(None, C.byref(bt), 0, C.byref(s), win, None) == -1
        bt.B = 0
        assert step() == 0
        bt.B = B
    step = lambda: lib.tcar_serve_step_window(C.byref(ctx), C.byref(bt), 0, C.byref(s), C.byref(w), None)
    for field in ("key", "lo", "hi"):                 # a window descriptor with a hole, also at B == 0
        setattr(w, field, None)
        assert step() == -1, field
        bt.B = 0
        assert step() == -1, field
        bt.B = B
        setattr(w, field, p.value)


def test_fresh_hours_is_refused_where_it_cannot_work():
    from tcar_amd.host import cli
    from tcar_amd.host.model import Seq2SeqAttNN
    from tcar_amd.host.synth import SynthFold
    check = lambda gpus=1, **values: cli.check_eval_options(values, gpus=gpus)
    with pytest.raises(ValueError, match="eval_panel"):
        check(fresh_hours=48, eval_panel=0, dp_mode="replica")
    with pytest.raises(ValueError, match="sharded"):
        check(fresh_hours=48, eval_panel=128, dp_mode="sharded")
    with pytest.raises(ValueError, match="fresh_hours"):
        check(fresh_hours=-1, eval_panel=128, dp_mode="replica")
    check(fresh_hours=0, eval_panel=0, dp_mode="sharded")
    check(fresh_hours=48, eval_panel=128, dp_mode="replica")
    assert cli.build_parser().parse_args([]).fresh_hours == 0
    assert cli.build_parser().parse_args(["--fresh_hours", "48", "--eval_panel", "128"]).fresh_hours == 48
    fold = SynthFold(n_items=60, dim=8, n_train=40, n_test=10, seed=1)
    small = dict(batch_size=8, epoch=1, neg_num=2, hidden_size=8, time_hidden_size=4, lr=0.003, emb_stddev=0.3, stddev=0.1)
    with pytest.raises(ValueError, match="eval_panel"):
        Seq2SeqAttNN(fold.model_args(fresh_hours=48, **small))
    with pytest.raises(ValueError, match="sharded"):
        Seq2SeqAttNN(fold.model_args(fresh_hours=48, eval_panel=128, dp_mode="sharded", **small))


class _NoEngine:
    """what the two refusals below may touch of an engine: nothing is uploaded or launched before they raise"""
    def set_item_keys(self, keys):
        self.keys = keys

    def set_categories(self, cat):
        pass

    def reset_coverage(self):
        pass


def _model_without_engine(fold, **args):
    """a Seq2SeqAttNN whose engine is never built (that needs the GPU): the checks under test come before the first device call"""
    from tcar_amd.host.model import Seq2SeqAttNN
    m = Seq2SeqAttNN.__new__(Seq2SeqAttNN)
    a = fold.model_args(**args)
    m.candidate_n, m.publish_time, m._keys, m._key_t0 = fold.n_items + 1, a["publish_time"], None, None
    m.fresh_hours, m.eval_panel, m.batch_size = float(a.get("fresh_hours", 0)), int(a.get("eval_panel", 0)), 8
    m.reverse_item, m.category_id, m._cat, m.gap_mode, m.neg_mode, m.neg_fast = a["reverse_item"], a["category_id"], None, "active_t", "uniform", False
    m.dp_world, m.dp_rank = 1, 0
    m.engine = _NoEngine()
    return m, a


def test_a_window_needs_every_publish_time_and_the_session_times():
    from tcar_amd.host.synth import SynthFold
    fold = SynthFold(n_items=60, dim=8, n_train=40, n_test=10, seed=1)
    # SynthFold hands out publish_time = [None] * n: asking for a window says so
    m, _ = _model_without_engine(fold)
    with pytest.raises(ValueError, match="publish_time"):
        m.recommend({}, k=5, window=(0, 10))
    times = [t.astype("datetime64[s]").item() for t in fold.publish_ts]
    assert isinstance(times[0], datetime.datetime)
    m, _ = _model_without_engine(fold, publish_time=times[:-1] + [None])
    with pytest.raises(ValueError, match="None"):
        m._item_keys()
    # all of them there: minutes since the earliest one, int32, installed on the engine once
    m, a = _model_without_engine(fold, publish_time=times, fresh_hours=48, eval_panel=128)
    keys = m._item_keys()
    assert keys.dtype.name == "int32" and keys.min() == 0 and m.engine.keys is keys and m._item_keys() is keys
    want = [(t - min(times)).total_seconds() // 60 for t in times]
    assert keys.tolist() == want
    assert m.minute_of(min(times) + datetime.timedelta(minutes=7, seconds=59)) == 7
    # a fold without session_time_dict cannot say when the label was clicked
    ld, sd, _ = fold.to_dicts(fold.test)
    with pytest.raises(ValueError, match="session_time_dict"):
        m.test(None, (ld, sd, None), a)
