"""Sectioned streamed selection at the op level (include/tcar_sections.h: tcar_section_panel) against the numpy model, exactly.

Built like test_gpu_quota_select.py, with its sizes: one fp32 matrix x [B, ldn] per catalog size, the panels pointer views into it,
padding columns at 1e9.  List g of a row is select_ref.fold_state over the pool "category == sections[g], inside the window, not
excluded, not NaN" (section_case.section_lists); topk and the scores where topk >= 0 must be the model's bits for every partition,
for the panels folded in reverse order and (N = 1003) for one-column panels, which give n = 1 and every n0 mod 4.

Two category tables per G:
  "rand"  about N/3 random codes, among them I32_MIN, -1, 0 and I32_MAX, so most listed sections hold fewer than k items; the sections
          of G >= 5 start with those four codes and a code no item carries
  "mod"   cat[i] = sections[i % G]: the G sections cover the catalog, N/G items each — more than a buffer holds.  G = 1 is "one code
          for the whole catalog": there output AND the list words of the raw state must equal those of tcar_select_panel on the same
          panels (the four tail words cannot: tcar_select_panel keeps its softmax pair in them, the sectioned fold never writes them)
and two configurations: A (no window, no exclusions) and B (windows on rows 2 and 6, exclusion lists on rows 0 and 6).

One row per case:
  0  random scores (B: its two best items excluded)
  1  random scores ("mod", G = 1: the comparison with tcar_select_panel covers every row)
  2  half the row tied at one value (B: a window of half the catalog)
  3  the whole row tied: more ties than any buffer holds — the overflow-and-retry path; the lists are the highest ids
  4  scores ascending with the item id, so ascending inside every section: every element is admitted
  5  items 0 .. 127 lead every section from the first panel on, and the LAST item of the catalog beats them
  6  B: a window, and the best item of every listed section excluded
  7  NaN at the would-be best items, and a run of -0.0 / +0.0 scores above everything else"""
import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401

from gpu_util import lib, ptr  # noqa: F401  (lib: the fixture)
from section_case import I32_MAX, I32_MIN, check_sections, section_lists

pytestmark = pytest.mark.gpu

PANELS = {7: (128,), 1003: (1024, 128), 20001: (20096, 4096), 49200: (49152, 8192)}
KS = (1, 20, 64)
GS = (1, 5, 16)
B = 8
ABSENT = 777_777_777                                     # a code no item carries
SPECIAL = (I32_MIN, -1, 0, I32_MAX)
GUARD = 0x5A5A5A5A

_BASE, _MODEL = {}, {}


def base(N):
    """scores and keys of one catalog size: computed once, shared by every k and G, never written"""
    if N not in _BASE:
        rng = np.random.RandomState(N)
        ldn = (N + 127) // 128 * 128
        x = (rng.standard_normal((B, ldn)) * 2).astype(np.float32)
        x[2, : N // 2] = x[2, 0]
        x[3, :N] = -0.75
        x[4, :N] = np.arange(N, dtype=np.float32) * 0.125 - 100.0
        F = min(128, N - 1)
        x[5, :F] = 200 + np.arange(F)
        x[5, N - 1] = 1000
        x[7, :N] = -1.0 - np.abs(x[7, :N])
        z = np.arange(1, min(13, N - 1))                   # a run of zeros of both signs above every other score of row 7
        x[7, z] = np.where(z % 2 == 0, np.float32(-0.0), np.float32(0.0))
        x[7, [0, N // 2]] = np.nan                         # (anything beats nothing: a NaN must never be listed)
        x[:, N:] = 1e9                                     # padding columns must never be picked
        key = (rng.permutation(N) - N // 2).astype(np.int32)
        codes = np.unique(rng.randint(I32_MIN, I32_MAX, max(N // 3, 2), dtype=np.int64))
        codes = codes[~np.isin(codes, SPECIAL) & ((codes < ABSENT) | (codes > ABSENT + 32))]     # (ABSENT + i: codes no item carries)
        rand = codes[rng.randint(0, len(codes), N)]
        pos = rng.permutation(N)[:min(N, 12)]              # up to three items for each of the four special codes
        rand[pos] = np.resize(np.asarray(SPECIAL, np.int64), len(pos))
        rand = rand.astype(np.int32)
        assert all((rand == s).any() for s in SPECIAL) and not (rand == ABSENT).any()
        for a in (x, key, rand):
            a.setflags(write=False)
        _BASE[N] = dict(x=x, key=key, ldn=ldn, rand=rand)
    return _BASE[N]


def tables(N, G):
    """{"rand" | "mod": (cat int32 [N], sections [G])}"""
    r = base(N)
    vals, counts = np.unique(r["rand"], return_counts=True)
    common = [int(v) for v in vals[np.argsort(-counts, kind="stable")] if v not in SPECIAL]
    lead = list(SPECIAL) + [ABSENT] if G >= 5 else []
    rand_sections = (lead + common + [ABSENT + 1 + i for i in range(G)])[:G]         # (a tiny catalog has fewer than G codes)
    assert len(set(rand_sections)) == G
    mod_sections = (list(SPECIAL) + [12345 + 7 * i for i in range(G)])[:G] if G >= 4 else [-5, 9, 11][:G]
    mod = np.asarray(mod_sections, np.int64)[np.arange(N) % G].astype(np.int32)
    return {"rand": (r["rand"], rand_sections), "mod": (mod, mod_sections)}


def config_b(N, cat, sections):
    """configuration B: the windows (rows 2 and 6: half the catalog) and the exclusion lists (row 6: the best item of every listed
    section inside its window; row 0: its two best items)"""
    r = base(N)
    x, key = r["x"], r["key"]
    lo, hi = np.full(B, I32_MIN, np.int64), np.full(B, I32_MAX, np.int64)
    lo[2], hi[2] = lo[6], hi[6] = -(N // 2), 0
    six = [w[0][0] for w in section_lists(x[6, :N], cat, sections, 1, (lo[6], hi[6]), key) if w[0]]
    excl = np.full((B, max(len(six), 2)), -1, np.int32)
    excl[6, :len(six)] = six
    excl[0, :2] = np.argsort(x[0, :N], kind="stable")[::-1][:2]
    return lo.astype(np.int32), hi.astype(np.int32), excl


def model(N, G, name, window):
    """the model's lists at k = 64 (a shorter list is its prefix): [B][G] (ids, scores); computed once per case"""
    if (N, G, name, window) not in _MODEL:
        r = base(N)
        cat, sections = tables(N, G)[name]
        lo, hi, excl = config_b(N, cat, sections) if window else (None, None, None)
        _MODEL[N, G, name, window] = [
            section_lists(r["x"][b, :N], cat, sections, 64, (lo[b], hi[b]) if window else None, r["key"],
                          excl[b][excl[b] >= 0] if window else ()) for b in range(B)]
    return _MODEL[N, G, name, window]


def model_cases(N, k, G, name, window):
    """what the cases are, in the model itself (no GPU needed)"""
    want = model(N, G, name, window)
    cat, sections = tables(N, G)[name]
    tag = "N=%d k=%d G=%d %s %s" % (N, k, G, name, "B" if window else "A")
    if name == "rand" and not window and N > 128:
        short = sum(len(want[0][g][0][:k]) < k for g in range(G))
        assert k == 1 or short >= (G + 1) // 2, tag                                # row 0: most sections are short
        if G >= 5:
            assert want[0][4][0] == [] and all(want[0][g][0] for g in range(4)), tag   # the absent code; the four special ones
    if name == "mod" and not window and N // G >= 64:
        sec = np.asarray(sections)[np.arange(N) % G]
        for g in range(G):
            mine = np.where(sec == sections[g])[0]
            assert want[3][g][0][:k] == mine[::-1][:k].tolist(), tag               # all tie: the section's highest ids
            assert want[4][g][0][:k] == mine[::-1][:k].tolist(), tag               # ascending: the same items
        g_last = (N - 1) % G
        assert want[5][g_last][0][0] == N - 1, tag                                 # row 5: the last item leads its section
    if not window:
        flat7 = [i for g in range(G) for i in want[7][g][0]]
        assert 0 not in flat7 and N // 2 not in flat7, tag                         # the NaN items are in no list
    if window:
        lo, hi, excl = config_b(N, cat, sections)
        six = set(excl[6][excl[6] >= 0].tolist())
        assert not six & {i for g in range(G) for i in want[6][g][0]}, tag


class Runner:
    """the device copies of one (N, G, table), and one reset / folds / finish per call"""

    def __init__(self, lib, N, G, name):
        r = base(N)
        self.lib, self.N, self.G, self.r = lib, N, G, r
        self.cat, self.sections = tables(N, G)[name]
        self.d = torch.tensor(r["x"]).cuda()
        self.dk = torch.tensor(r["key"]).cuda()
        self.dc = torch.tensor(self.cat).cuda()
        self.codes = (np.ctypeslib.as_ctypes(np.asarray(self.sections, np.int64).astype(np.int32)))
        lo, hi, excl = config_b(N, self.cat, self.sections)
        self.dlo, self.dhi, self.de, self.X = torch.tensor(lo).cuda(), torch.tensor(hi).cuda(), torch.tensor(excl).cuda(), excl.shape[1]

    def __call__(self, k, panels, window=False, state=None, finish=True, columns=False):
        """panels: [(n0, n)] in fold order.  Returns (topk [B, G, k], score [B, G, k], state words [B G, 2k + 4]) as numpy arrays;
        the guard words behind the state and behind both outputs are checked here."""
        lib, G, d = self.lib, self.G, self.d
        rw = 2 * k + 4
        words = int(lib.tcar_select_state_bytes(B * G, k)) // 4
        assert words == B * G * rw
        if state is None:
            state = torch.full((words + 8,), GUARD, dtype=torch.int32, device="cuda")
            assert lib.tcar_select_reset(B * G, k, ptr(state), None) == 0
        topk = torch.full((B * G * k + 8,), -7, dtype=torch.int32, device="cuda")
        score = torch.full((B * G * k + 8,), -7.0, device="cuda")
        win = (ptr(self.dk), ptr(self.dlo), ptr(self.dhi)) if window else (None, None, None)
        ex = (ptr(self.de), self.X) if window else (None, 0)
        assert self.dc.numel() == self.N                                  # the fold reads cat[n0 .. n0 + n): inside the table
        if columns:          # one-column panels: a panel's rows are 16-byte aligned, so every column gets a buffer [B, 4] of its own
            cols = torch.full((self.N, B, 4), 1e9, device="cuda")
            cols[:, :, 0] = d[:, :self.N].t()
        for n0, n in panels:
            assert 0 <= n0 and n0 + n <= self.N and n <= 49152 and (n == 1 or not columns)
            where, ld = (ptr(cols[n0]), 4) if columns else (ptr(d, n0), self.r["ldn"])
            assert lib.tcar_section_panel(B, n0, n, where, ld, k, G, self.codes, ptr(self.dc), *ex, *win, ptr(state), None) == 0
        if finish:
            assert lib.tcar_select_finish(B * G, k, ptr(state), None, ptr(topk), ptr(score), None, None, None) == 0
        torch.cuda.synchronize()
        st = state.cpu().numpy()
        assert (st[words:] == GUARD).all() and (topk[-8:] == -7).all() and (score[-8:] == -7.0).all()
        self.state = state
        return topk[:-8].view(B, G, k).cpu().numpy(), score[:-8].view(B, G, k).cpu().numpy(), st[:words].reshape(B * G, rw)


def partition(N, P, reverse=False):
    parts = [(n0, min(P, N - n0)) for n0 in range(0, N, P)]
    return parts[::-1] if reverse else parts


def check(run, k, want, tk, sc, st, tag):
    x, N, G = run.r["x"], run.N, run.G
    for b in range(B):
        check_sections(x[b], [(ids[:k], s[:k]) for ids, s in want[b]], tk[b], sc[b], k, (tag, b))
    # the raw state: the list of every row, (-inf, -1) behind its end, and the reset's tail (count 0, max -inf, sum 0, pad 0)
    assert (st[:, k:2 * k].reshape(B, G, k) == tk).all(), tag
    assert (st[:, 2 * k:] == np.array([0, 0xff800000 - 2 ** 32, 0, 0], np.int64)).all(), tag
    empty = st[:, k:2 * k] < 0
    assert (st[:, :k][empty] == np.array(-np.inf, np.float32).view(np.int32)).all(), tag


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("N", sorted(PANELS))
def test_section_lists_are_the_model_for_every_partition(lib, N, k, G):
    x = base(N)["x"]
    for name in ("rand", "mod"):
        run = Runner(lib, N, G, name)
        for window in (False, True):
            want = model(N, G, name, window)
            tag = "N=%d k=%d G=%d %s %s" % (N, k, G, name, "B" if window else "A")
            model_cases(N, k, G, name, window)
            outs = []
            for P in PANELS[N]:
                outs.append(run(k, partition(N, P), window))
                check(run, k, want, *outs[-1], "%s P=%d" % (tag, P))
            outs.append(run(k, partition(N, PANELS[N][-1], reverse=True), window))
            check(run, k, want, *outs[-1], tag + " reversed")
            for o in outs[1:]:
                for a, b in zip(outs[0], o):
                    assert a.tobytes() == b.tobytes(), tag
            if name == "mod" and G == 1 and not window:
                # one code for the whole catalog: the unlabelled tcar_select_panel on the same panels, output and list words
                P = PANELS[N][-1]
                state = torch.full((B * (2 * k + 4),), GUARD, dtype=torch.int32, device="cuda")
                topk = torch.full((B, k), -7, dtype=torch.int32, device="cuda")
                score = torch.full((B, k), -7.0, device="cuda")
                assert lib.tcar_select_reset(B, k, ptr(state), None) == 0
                for n0, n in partition(N, P):
                    assert lib.tcar_select_panel(B, n0, n, ptr(run.d, n0), run.r["ldn"], k, None, None, None, 0, ptr(state), None) == 0
                assert lib.tcar_select_finish(B, k, ptr(state), None, ptr(topk), ptr(score), None, None, None) == 0
                torch.cuda.synchronize()
                tk, sc, st = outs[-2]
                assert tk.reshape(B, k).tobytes() == topk.cpu().numpy().tobytes(), tag
                assert sc.reshape(B, k).tobytes() == score.cpu().numpy().tobytes(), tag
                assert st[:, :2 * k].tobytes() == np.ascontiguousarray(state.cpu().numpy().reshape(B, 2 * k + 4)[:, :2 * k]).tobytes(), tag
    assert x.flags.writeable is False


@pytest.mark.parametrize("name", ("rand", "mod"))
def test_one_column_panels_reach_every_alignment_of_the_slices(lib, name):
    N, k, G = 1003, 20, 5
    run = Runner(lib, N, G, name)
    want = model(N, G, name, True)
    tk, sc, st = run(k, partition(N, 1), window=True, columns=True)
    check(run, k, want, tk, sc, st, "one-column panels " + name)
    assert run(k, partition(N, 1024), window=True)[0].tobytes() == tk.tobytes()


def test_a_session_whose_sections_admit_nothing_keeps_its_rows(lib):
    """the first panel fills the rows; in the second panel nothing is eligible for the sessions 2 and 6 (their windows end below
    every key of it): their G rows keep every bit, while the other sessions fold the panel"""
    N, k, G = 1003, 20, 5
    run = Runner(lib, N, G, "mod")
    first, second = [(0, 512)], [(512, N - 512)]
    _, _, st1 = run(k, first, window=True, finish=False)
    state = run.state
    key = base(N)["key"]
    lo = run.dlo.clone()
    run.dhi[2] = run.dhi[6] = int(key[512:].min())          # (lo <= key < hi holds for no item of the second panel)
    try:
        _, _, st2 = run(k, second, window=True, state=state)
    finally:
        run.dhi[2] = run.dhi[6] = 0
    assert torch.equal(lo, run.dlo)
    rows = st1.reshape(B, G, -1)
    after = st2.reshape(B, G, -1)
    for b in (2, 6):
        assert rows[b].tobytes() == after[b].tobytes(), b
    assert any(rows[b].tobytes() != after[b].tobytes() for b in (0, 1, 3, 4))       # (the other sessions did fold the panel)


def test_argument_errors_leave_the_state_untouched(lib):
    N, k, G = 1003, 20, 5
    run = Runner(lib, N, G, "rand")
    _, _, before = run(k, partition(N, 1024))
    state = run.state
    codes = np.asarray(run.sections, np.int64).astype(np.int32)
    dup = codes.copy()
    dup[3] = dup[1]
    args = lambda G_, c, cat: (B, 0, N, ptr(run.d), run.r["ldn"], k, G_, np.ctypeslib.as_ctypes(c) if c is not None else None, cat, None,
                               0, None, None, None, ptr(state), None)
    assert lib.tcar_section_panel(*args(G, dup, ptr(run.dc))) == -1
    assert lib.tcar_section_panel(*args(0, codes, ptr(run.dc))) == -1
    assert lib.tcar_section_panel(*args(17, np.arange(17, dtype=np.int32), ptr(run.dc))) == -1
    assert lib.tcar_section_panel(*args(G, None, ptr(run.dc))) == -1
    assert lib.tcar_section_panel(*args(G, codes, None)) == -1
    torch.cuda.synchronize()
    assert state.cpu().numpy()[:before.size].tobytes() == before.tobytes()
