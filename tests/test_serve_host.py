"""Host side of the streamed score-and-select (include/tcar_serve.h): the bindings generated from the header, the layout of the
struct mirror and the argument checks, which answer before anything is launched — none of it needs a GPU."""
import ctypes as C
import os
import re
import subprocess
import types

import pytest

import tcar_amd  # noqa: F401
from tcar_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOTYPE = r"^((?:const )?\w+\*?) (tcar_\w+)\(([^)]*)\)\s*;"


def _header():
    with open(os.path.join(ROOT, "include", "tcar_serve.h")) as f:
        return re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)


def test_every_prototype_of_the_serve_header_is_bound():
    lib = _lib.load()
    protos = re.findall(PROTOTYPE, _header(), flags=re.M)
    assert [name for _, name, _ in protos] == _lib.SERVE_SYMBOLS and len(protos) == 6
    assert not set(_lib.SERVE_SYMBOLS) & set(_lib.SYMBOLS)
    for ret, name, params in protos:
        f = getattr(lib, name)
        n = 0 if params.strip() == "void" else params.count(",") + 1
        assert f.argtypes is not None and len(f.argtypes) == n, (name, n)
        assert f.restype is {"int": C.c_int, "int64_t": C.c_int64}[ret], name
    i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
    assert lib.tcar_select_panel.argtypes == [i32, i32, i32, vp, i64, i32, vp, vp, vp, i32, vp, vp]
    assert lib.tcar_serve_step.argtypes == [C.POINTER(_lib.Ctx), C.POINTER(_lib.Batch), i32, C.POINTER(_lib.Serve), vp]


def test_serve_abi_version_and_the_unchanged_core_abi():
    lib = _lib.load()
    assert lib.tcar_serve_abi_version() == _lib.SERVE_ABI_VERSION == 1
    # the core header's numbers are where they were: everything new lives in tcar_serve.h
    assert _lib.ABI_VERSION == 30 and len(_lib.SYMBOLS) == 112 and len(_lib.Ctx._fields_) == 104 and len(_lib.Shard._fields_) == 25
    assert _lib.SERVE_HEADER in _lib.HEADERS and "select.hip" in _lib.SOURCES           # both enter the build id


def test_serve_mirror_has_the_layout_the_compiler_gives_the_header(tmp_path):
    """a host-only C++ program that includes the header prints sizeof / offsetof of every field the parser named"""
    m = _lib.Serve
    assert [f[0] for f in m._fields_] == ["k", "panel", "panel_buf", "state", "state_bytes", "lab_score", "excl", "X", "topk", "score",
                                          "rank", "ce"]
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "tcar_serve.h"', 'int main() {',
             '  printf("%zu\\n", sizeof(tcar_serve_t));']
    lines += ['  printf("%%zu %%zu\\n", offsetof(tcar_serve_t, %s), sizeof(((tcar_serve_t*)0)->%s));' % (f[0], f[0]) for f in m._fields_]
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
    assert lib.tcar_select_state_bytes(B, k) == B * (2 * k + 4) * 4 and lib.tcar_select_state_bytes(B, 64) > 0
    assert lib.tcar_select_state_bytes(B, 65) < 0 and lib.tcar_select_state_bytes(B, 0) < 0
    names = ("B", "n0", "n", "panel", "ld", "k", "label", "lab_score", "excl", "X", "state", "stream")
    base = dict(B=B, n0=0, n=128, panel=p, ld=128, k=k, label=None, lab_score=None, excl=None, X=0, state=p, stream=None)
    panel = lambda **kw: lib.tcar_select_panel(*[dict(base, **kw)[a] for a in names])
    assert panel(k=65) == -1 and panel(k=0) == -1
    assert panel(n=49153, ld=49156) == -1
    assert panel(ld=130) == -1                    # ld % 4
    assert panel(ld=64) == -1                     # ld < n
    assert panel(state=None) == -1
    assert panel(panel=None) == -1
    assert panel(lab_score=p) == -1               # lab_score without label
    assert panel(excl=p, X=0) == -1
    assert lib.tcar_select_reset(B, 65, p, None) == -1 and lib.tcar_select_reset(B, k, None, None) == -1
    assert lib.tcar_select_finish(B, 65, p, None, p, None, None, None, None) == -1
    assert lib.tcar_select_finish(B, k, None, None, p, None, None, None, None) == -1
    assert lib.tcar_select_finish(B, k, p, None, None, None, None, None, None) == -1
    assert lib.tcar_select_finish(B, k, p, None, p, None, None, p, None) == -1          # ce without lab_score
    # B == 0: nothing to do
    assert panel(B=0) == 0 and panel(B=0, state=None, panel=None) == 0
    assert lib.tcar_select_reset(0, k, None, None) == 0
    assert lib.tcar_select_finish(0, k, None, None, None, None, None, None, None) == 0

    ctx, bt, s = _lib.Ctx(), _lib.Batch(), _lib.Serve()
    bt.B, bt.T = B, 3
    s.k, s.panel, s.panel_buf, s.state, s.state_bytes, s.topk = k, 256, p.value, p.value, 4096 * 4, p.value
    step = lambda: lib.tcar_serve_step(C.byref(ctx), C.byref(bt), 0, C.byref(s), None)
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
    assert lib.tcar_serve_step(None, C.byref(bt), 0, C.byref(s), None) == -1
    bt.B = 0
    assert step() == 0


@pytest.mark.parametrize("sharded", [False, True])
def test_a_request_is_refused_by_one_rule_on_both_engines(sharded):
    """TcarEngine._serve and ShardedEngine.serve_pieces normalise (k, panel, window, max_per_category) through ONE method: the same
    ValueError, word for word, on both classes, before anything of the device is touched (the engines are never built)"""
    from tcar_amd.engine import TcarEngine
    from tcar_amd.sharded import ShardedEngine
    cls = ShardedEngine if sharded else TcarEngine
    assert cls._serve_request is TcarEngine._serve_request
    eng = cls.__new__(cls)
    eng.geo, eng.nl, eng._cat = types.SimpleNamespace(N=700, Npad=768), 700, None
    width = 768
    refused = [(dict(k=0), "k must be in [1, 64]"), (dict(k=65), "k must be in [1, 64]"),
               (dict(panel=100), "panel must be a positive multiple of 128, at most 49152"),
               (dict(panel=49152 + 128), "panel must be a positive multiple of 128, at most 49152"),
               (dict(max_per_category=0), "max_per_category must be an int >= 1 (None: no cap)"),
               (dict(max_per_category=True), "max_per_category must be an int >= 1 (None: no cap)"),
               (dict(window=(0, 10)), "a window compares item keys: call set_item_keys(keys) first")]
    for kw, text in refused:
        req = dict(dict(k=20, panel=None, window=None, max_per_category=None), **kw)
        with pytest.raises(ValueError) as e:
            eng._serve_request(req["k"], req["panel"], req["window"], req["max_per_category"], width)
        assert str(e.value) == text, kw
    # and what it lets through: the default panel, a named one clipped to the scored width
    assert eng._serve_request(20, None, None, None, width) == (20, 768, None)
    assert eng._serve_request(64, 49152, None, None, width) == (64, 768, None)
    assert eng._serve_request(1, 128, None, None, width) == (1, 128, None)
