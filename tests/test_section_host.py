"""Host side of sectioned selection (include/tcar_sections.h): the bindings generated from the header, the argument checks, which
answer before anything is launched, the engine's and the trainer's refusals, the numpy model against itself, the section choice of
test() and the arithmetic of its line — none of it needs a GPU."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

import tcar_amd  # noqa: F401
from tcar_amd import _lib

from section_case import I32_MAX, I32_MIN, section_lists
from select_ref import fold_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOTYPE = r"^((?:const )?\w+\*?) (tcar_\w+)\(([^)]*)\)\s*;"
FIELDS = ["k", "G", "sections", "cat", "panel", "panel_buf", "state", "state_bytes", "excl", "X", "topk", "score", "window", "overall"]


def test_the_sections_header_is_parsed_and_bound():
    with open(os.path.join(ROOT, "include", "tcar_sections.h")) as f:
        header = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    lib = _lib.load()
    assert lib.tcar_sections_abi_version() == _lib.SECTIONS_ABI_VERSION == 1
    assert _lib.SECTIONS_HEADER in _lib.HEADERS and "sections.hip" in _lib.SOURCES          # both enter the build id
    protos = re.findall(PROTOTYPE, header, flags=re.M)
    assert [name for _, name, _ in protos] == _lib.SECTIONS_SYMBOLS == ["tcar_sections_abi_version", "tcar_section_panel",
                                                                         "tcar_sections_step", "tcar_sections_step_ragged"]
    layers = [p for p, _ in _lib.ABI_LAYERS]
    assert layers[layers.index("QUOTA") + 1] == "SECTIONS" and ("SECTIONS", "tcar_sections.h") in _lib.ABI_LAYERS
    every = [s for p in layers if p != "SECTIONS" for s in getattr(_lib, _lib._name(p, "SYMBOLS"))]
    assert not set(_lib.SECTIONS_SYMBOLS) & set(every)
    i32, i64, vp, P = C.c_int32, C.c_int64, C.c_void_p, C.POINTER
    assert lib.tcar_section_panel.argtypes == [i32, i32, i32, vp, i64, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp]
    assert lib.tcar_sections_step.argtypes == [P(_lib.Ctx), P(_lib.Batch), i32, P(_lib.Sections), vp]
    # the layer is bound before RAGGED, so the ragged descriptor is a plain pointer here — and byref() of the mirror satisfies it
    assert lib.tcar_sections_step_ragged.argtypes == [P(_lib.Ctx), P(_lib.Batch), vp, i32, P(_lib.Sections), vp]
    assert all(f.restype is C.c_int for f in (lib.tcar_section_panel, lib.tcar_sections_step, lib.tcar_sections_step_ragged))
    bt = _lib.Batch()
    assert lib.tcar_sections_step_ragged(None, C.byref(bt), C.byref(_lib.Ragged()), 0, None, None) == -1      # accepted by ctypes
    # everything new lives in tcar_sections.h: the pinned numbers and places of the other layers are where they were
    assert _lib.ABI_LAYERS[0] == ("", "tcar_hip.h") and _lib.ABI_LAYERS[-1] == ("RAGGED", "tcar_ragged.h")
    assert _lib.ABI_LAYERS[-2] == ("RETRIEVE_SHARD", "tcar_retrieve_shard.h")
    assert layers[layers.index("CATALOG") + 1] == "CATALOG_SHARD"
    assert _lib.ABI_VERSION == 30 and len(_lib.SYMBOLS) == 112 and len(_lib.Ctx._fields_) == 104 and len(_lib.Shard._fields_) == 25
    assert len(_lib.SERVE_SYMBOLS) == 6 and len(_lib.WINDOW_SYMBOLS) == 3 and len(_lib.QUOTA_SYMBOLS) == 3
    assert len(_lib.CAND_SYMBOLS) == 4 and len(_lib.RETRIEVE_SYMBOLS) == 7
    assert "tcar_serve_step_ragged" in _lib.RAGGED_SYMBOLS and "tcar_sections_step_ragged" not in _lib.RAGGED_SYMBOLS


def test_the_mirror_has_the_layout_the_compiler_gives_the_header(tmp_path):
    m = _lib.Sections
    assert [f[0] for f in m._fields_] == FIELDS
    assert (m.sections.offset, m.sections.size, m.cat.offset) == (8, 64, 72)
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "tcar_sections.h"', 'int main() {',
             '  printf("%zu\\n", sizeof(tcar_sections_t));']
    lines += ['  printf("%%zu %%zu\\n", offsetof(tcar_sections_t, %s), sizeof(((tcar_sections_t*)0)->%s));' % (f, f) for f in FIELDS]
    lines.append('  return 0;\n}')
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([_lib._hipcc(), "-x", "c++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = iter(subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE).stdout.decode().split("\n"))
    assert int(next(got)) == C.sizeof(m)
    for f in FIELDS:
        d = getattr(m, f)
        assert next(got).split() == [str(d.offset), str(d.size)], f


def _codes(*v):
    return (C.c_int32 * len(v))(*v)


def test_argument_errors_come_back_before_any_launch():
    lib = _lib.load()
    buf = (C.c_float * 4096)()                    # host memory: never dereferenced, an accepted call would have to launch
    p = C.cast(buf, C.c_void_p)
    names = ("B", "n0", "n", "panel", "ld", "k", "G", "sections", "cat", "excl", "X", "key", "lo", "hi", "state", "stream")
    base = dict(B=2, n0=0, n=100, panel=p, ld=128, k=20, G=3, sections=_codes(5, -1, I32_MAX), cat=p, excl=None, X=0, key=None, lo=None,
                hi=None, state=p, stream=None)
    fold = lambda **kw: lib.tcar_section_panel(*[dict(base, **kw)[a] for a in names])
    assert fold(G=0) == -1 and fold(G=-1) == -1 and fold(G=17, sections=_codes(*range(17))) == -1
    assert fold(sections=_codes(5, -1, 5)) == -1 and fold(G=2, sections=_codes(I32_MIN, I32_MIN)) == -1        # two equal codes
    assert fold(sections=None) == -1 and fold(cat=None) == -1
    for win in (dict(), dict(key=p, lo=p, hi=p)):                  # everything check_fold_args refuses
        call = lambda **kw: fold(**dict(win, **kw))
        assert call(k=0) == -1 and call(k=65) == -1 and call(B=-1) == -1
        assert call(n=49153, ld=49156) == -1 and call(n=-1) == -1 and call(n0=-1) == -1 and call(n0=2 ** 31 - 50) == -1
        assert call(ld=126) == -1 and call(ld=96) == -1                                       # ld % 4, ld < n
        assert call(panel=C.c_void_p(p.value + 4)) == -1 and call(panel=None) == -1 and call(state=None) == -1
        assert call(state=C.c_void_p(p.value + 2)) == -1 and call(excl=p, X=0) == -1 and call(X=-1) == -1
    assert fold(key=p) == -1 and fold(key=p, lo=p) == -1 and fold(lo=p, hi=p) == -1            # a window is all three or none
    assert fold(B=0) == 0 and fold(n=0) == 0 and fold(B=0, panel=None, state=None) == 0
    assert fold(G=16, sections=_codes(*range(-8, 8)), B=0) == 0
    assert fold(B=0, G=0) == -1 and fold(B=0, cat=None) == -1 and fold(n=0, sections=_codes(1, 1, 2)) == -1      # an error at B == 0 too
    assert fold(B=0, sections=None) == -1 and fold(B=0, k=65) == -1

    ctx, bt, d, o = _lib.Ctx(), _lib.Batch(), _lib.Sections(), _lib.Serve()
    rg = _lib.Ragged()
    bt.B, bt.T = 2, 3
    rows = 2 * 3 * (2 * 20 + 4) * 4                                 # B G rows of 2 k + 4 words
    good = dict(k=20, G=3, cat=p.value, panel=128, panel_buf=p.value, state=p.value, state_bytes=rows, excl=None, X=0, topk=p.value,
                score=p.value, window=None, overall=None)
    step = lambda: lib.tcar_sections_step(C.byref(ctx), C.byref(bt), 0, C.byref(d), None)
    twin = lambda: lib.tcar_sections_step_ragged(C.byref(ctx), C.byref(bt), C.byref(rg), 0, C.byref(d), None)

    def install(codes=(7, I32_MIN, I32_MAX), **kw):
        for f, v in dict(good, **kw).items():
            setattr(d, f, v)
        for i, c in enumerate(codes):
            d.sections[i] = c

    for bad in (dict(k=0), dict(k=65), dict(G=0), dict(G=17), dict(codes=(7, 8, 7)), dict(cat=None), dict(panel=0), dict(panel=100),
                dict(panel=49280), dict(panel_buf=None), dict(panel_buf=p.value + 4), dict(state=None), dict(state_bytes=rows - 4),
                dict(topk=None), dict(X=-1), dict(excl=p.value, X=0)):
        install(**bad)
        assert step() == -1 and twin() == -1, bad
        bt.B = 0                                                   # an argument error is one at B == 0 too (no row: no byte is too few)
        assert (step(), twin()) == ((0, 0) if "state_bytes" in bad else (-1, -1)), bad
        bt.B = 2
    w = _lib.Window()                              # a window descriptor without its arrays
    install(window=C.addressof(w))
    assert step() == -1 and twin() == -1
    o.k, o.state, o.state_bytes, o.topk = 20, p.value, 2 * 44 * 4, p.value
    for f, v in (("k", 0), ("k", 65), ("state", None), ("topk", None), ("state_bytes", 2 * 44 * 4 - 4)):
        keep = getattr(o, f)
        setattr(o, f, v)
        install(overall=C.addressof(o))
        assert step() == -1 and twin() == -1, f
        setattr(o, f, keep)
    install(overall=C.addressof(o))
    assert step() == -1 and twin() == -1           # an empty context (no parameters): still before any launch
    install()
    assert step() == -1 and twin() == -1
    assert lib.tcar_sections_step(None, C.byref(bt), 0, C.byref(d), None) == -1
    assert lib.tcar_sections_step(C.byref(ctx), C.byref(bt), 0, None, None) == -1
    assert lib.tcar_sections_step_ragged(C.byref(ctx), C.byref(bt), None, 0, C.byref(d), None) == -1          # the twin needs its descriptor
    bt.B = 0
    assert step() == 0 and twin() == 0
    install(overall=C.addressof(o))
    assert step() == 0 and twin() == 0


def test_the_engine_validates_a_request_before_any_device_call():
    """TcarEngine._sections_request runs before the upload and the step: on an engine that was never built (no device, no workspace,
    no library handle) a refused request raises ValueError and nothing else is reached"""
    from tcar_amd.engine import SectionLists, TcarEngine
    from tcar_amd.sharded import ShardedEngine
    eng = TcarEngine.__new__(TcarEngine)
    eng.shard, eng.geo = (0, 700), types.SimpleNamespace(N=700, Npad=768)
    feed = {}
    with pytest.raises(ValueError, match=r"call set_categories\(cat_of_item\) first"):
        eng.recommend_sections(feed, [1, 2])
    eng._cat = object()
    codes = "sections: 1 to 16 category codes, not %d"
    refused = [(lambda: eng.recommend_sections(feed, []), codes % 0),
               (lambda: eng.recommend_sections(feed, list(range(17))), codes % 17),
               (lambda: eng.recommend_sections(feed, 5), "sections: 1 to 16 distinct integer category codes"),
               (lambda: eng.recommend_sections(feed, [1, 2, 1]), "section codes must be pairwise distinct"),
               (lambda: eng.recommend_sections(feed, [1, 2.0]), "section codes must be integers"),
               (lambda: eng.recommend_sections(feed, [1, True]), "section codes must be integers"),
               (lambda: eng.recommend_sections(feed, [1, "a"]), "section codes must be integers"),
               (lambda: eng.recommend_sections(feed, [1, 2 ** 31]), "section codes must fit int32"),
               (lambda: eng.recommend_sections(feed, [-2 ** 31 - 1]), "section codes must fit int32"),
               (lambda: eng.recommend_sections(feed, [1], k=0), "k must be an int in [1, 64]"),
               (lambda: eng.recommend_sections(feed, [1], k=65), "k must be an int in [1, 64]"),
               (lambda: eng.recommend_sections(feed, [1], k=2.0), "k must be an int in [1, 64]"),
               (lambda: eng.recommend_sections(feed, [1], k=None), "k must be an int in [1, 64]"),
               (lambda: eng.recommend_sections(feed, [1], overall=0), "overall must be an int in [1, 64]"),
               (lambda: eng.recommend_sections(feed, [1], overall=65), "overall must be an int in [1, 64]"),
               (lambda: eng.recommend_sections(feed, [1], window=(0, 5)), "a window compares item keys: call set_item_keys(keys) first"),
               (lambda: eng.recommend_sections(feed, [1], panel=100), "panel must be a positive multiple of 128, at most 49152"),
               (lambda: eng.recommend_sections(feed, [1], panel=49280), "panel must be a positive multiple of 128, at most 49152")]
    for call, text in refused:
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text
    got, panel = eng._sections_request(np.array([I32_MIN, -1, 0, I32_MAX]), 64, 1, None, None, 768)
    assert got.dtype == np.int32 and got.tolist() == [I32_MIN, -1, 0, I32_MAX] and panel == 768
    assert eng._sections_request(range(16), np.int64(1), None, 128, None, 768)[1] == 128
    eng.shard = (0, 350)
    with pytest.raises(_lib.TcarError, match="whole catalog on this engine"):
        eng.recommend_sections(feed, [1, 2])
    sh = ShardedEngine.__new__(ShardedEngine)
    with pytest.raises(_lib.TcarError, match=r"recommend_sections\(\) needs the whole catalog on one engine.*sections over shards are not built yet"):
        sh.recommend_sections(feed, [1, 2])
    assert SectionLists._fields == ("topk", "scores", "overall_topk", "overall_scores")


def test_eval_sections_is_range_checked_and_refused_where_it_cannot_work():
    from tcar_amd.host import cli
    from tcar_amd.host.model import Seq2SeqAttNN
    from tcar_amd.host.synth import SynthFold
    check = lambda gpus=1, **values: cli.check_eval_options(values, gpus=gpus)
    with pytest.raises(ValueError, match=r"--eval_sections must be in \[1, 16\]"):
        check(eval_sections=17, eval_panel=128, dp_mode="replica")
    with pytest.raises(ValueError, match="eval_sections must be positive"):
        check(eval_sections=-1, eval_panel=128, dp_mode="replica")
    with pytest.raises(ValueError, match="eval_sections needs --eval_panel"):
        check(eval_sections=4, eval_panel=0, dp_mode="replica")
    with pytest.raises(ValueError, match="eval_sections.*sharded"):
        check(eval_sections=4, dp_mode="sharded")          # (with --eval_panel the refusal of --eval_panel comes first)
    for ok in ((0, 0, "sharded"), (0, 0, "replica"), (1, 128, "replica"), (16, 49152, "replica")):
        check(eval_sections=ok[0], eval_panel=ok[1], dp_mode=ok[2])
    ap = cli.build_parser()
    assert ap.parse_args([]).eval_sections == 0
    a = ap.parse_args(["--eval_sections", "4", "--eval_panel", "128", "--fresh_hours", "48", "--eval_mixed", "1"])
    assert (a.eval_sections, a.fresh_hours, a.eval_mixed) == (4, 48, 1)
    cli.check_eval_options(vars(a), gpus=a.gpus)                                            # the combinations the flag allows
    fold = SynthFold(n_items=60, dim=8, n_train=40, n_test=10, seed=1)
    small = dict(batch_size=8, epoch=1, neg_num=2, hidden_size=8, time_hidden_size=4, lr=0.003, emb_stddev=0.3, stddev=0.1)
    for kw, text in ((dict(eval_sections=4), "eval_panel"), (dict(eval_sections=17, eval_panel=128), r"\[1, 16\]"),
                     (dict(eval_sections=4, eval_panel=128, dp_mode="sharded"), "sharded")):
        with pytest.raises(ValueError, match=text):
            Seq2SeqAttNN(fold.model_args(**kw, **small))


def test_the_model_agrees_with_the_windowed_model_whose_keys_are_the_categories():
    """list g of a sectioned call = the windowed list with key = cat, lo = code, hi = code + 1 (a code below INT32_MAX)"""
    rng = np.random.RandomState(11)
    N, k = 400, 7
    x = rng.standard_normal(N).astype(np.float32)
    x[5:40] = x[5]                                                   # ties
    x[[3, 77]] = np.nan
    x[100], x[101] = -0.0, 0.0
    cat = rng.randint(-3, 9, N).astype(np.int32)
    cat[::50] = I32_MIN
    cat[1::50] = I32_MAX - 1
    sections = [I32_MIN, -3, 0, 8, I32_MAX - 1, 1234]
    excl = [int(np.nanargmax(np.where(cat == c, x, -np.inf))) for c in sections[:-1]]
    got = section_lists(x, cat, sections, k, excl=excl)
    ids = np.arange(N)
    ok = ~np.isnan(x)
    for g, code in enumerate(sections):
        pool = (np.int64(code) <= cat.astype(np.int64)) & (cat.astype(np.int64) < np.int64(code) + 1)
        want = fold_state(ids[ok], x[ok], k, pool=pool[ok], excl=excl)
        assert got[g][0] == want["ids"] and got[g][1].tobytes() == want["scores"].tobytes(), code
        assert not set(got[g][0]) & set(excl) and all(cat[i] == code for i in got[g][0])
    assert got[-1][0] == [] and len(got[1][0]) == k
    # a publish window on top of the sections: the pool is the intersection
    key = rng.permutation(N).astype(np.int32)
    both = section_lists(x, cat, sections, k, window=(100, 300), key=key)
    for g, code in enumerate(sections):
        want = fold_state(ids[ok], x[ok], k, pool=((cat == code) & (key >= 100) & (key < 300))[ok])
        assert both[g][0] == want["ids"]


def test_the_sections_of_test_are_the_largest_categories_and_its_line_counts_labels_in_their_own_list():
    from tcar_amd.host import metrics as M
    cat = np.array([5, 5, 5, -2, -2, -2, 9, 9, 7, 7, 1], np.int32)              # sizes: 5 -> 3, -2 -> 3, 9 -> 2, 7 -> 2, 1 -> 1
    assert M.largest_categories(cat, 1).tolist() == [-2]                         # a tie goes to the smaller code
    assert M.largest_categories(cat, 2).tolist() == [-2, 5]
    assert M.largest_categories(cat, 3).tolist() == [-2, 5, 7]
    assert M.largest_categories(cat, 4).tolist() == [-2, 5, 7, 9]
    assert M.largest_categories(cat, 16).tolist() == [-2, 5, 7, 9, 1]            # fewer codes than sections: all of them
    sections = [-2, 5, 7]
    topk = np.full((5, 3, 2), -1, np.int64)
    topk[0, 0] = [3, 4]          # label 4 (category -2) is in the list of section -2: a hit
    topk[1, 1] = [0, 1]          # label 2 (category 5) is not in its section's list: covered, no hit
    topk[2, 0] = [8, 9]          # label 8 (category 7) sits in ANOTHER section's list only: covered, no hit
    topk[3, 2] = [9, -1]         # label 9 (category 7) in the short list of its own section: a hit
    topk[4, 0] = [6, 10]         # label 6 (category 9): no listed section
    hit, covered = M.section_hits(topk, np.array([4, 2, 8, 9, 6]), cat, sections)
    assert hit.tolist() == [True, False, False, True, False] and covered.tolist() == [True, True, True, True, False]
    assert hit.sum() / covered.sum() == 0.5 and covered.sum() / 5 == 0.8
