"""Capped streamed selection at the op level (include/tcar_quota.h: tcar_select_panel_quota) against the numpy walk, exactly.

Built like test_gpu_window_select.py, with its sizes: one fp32 matrix x [B, ldn] per catalog size, the panels pointer views into it.
The list of a row is select_ref.capped_walk over its eligible items (in its pool, not excluded); topk, the scores where topk >= 0 and
the rank must be the model's bits for every partition and for the panels folded in reverse order; ce must be the bits of the uncapped
call of the same partition.  Three category tables — one code for all, about N/3 random codes, id % 5 — and two configurations:
A (no window, no exclusions) and B (windows and exclusion lists).

One row per case:
  0  plain random scores (with m >= k: output and raw state are those of tcar_select_panel_window)
  1  plain random scores; under the one-code table every list is m items, then -1
  2  half the row tied at one value; B: a window of half the catalog
  3  dominant category: the 2k best scores, all in the first panel, share one code (a list that is not full below the threshold)
  4  all-tie row: more than 1,024 candidates tie (the register path); under id % 5 the highest ids that respect the cap
  5  displacement: m items of one category lead the first panel, the last panel holds a better one of it
  6  B: the best item of every category is excluded and consumes no quota
  7  B: a window and a label outside it; the label is in the pool and counts against its category"""
import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401

from select_ref import capped_walk
from gpu_util import lib, ptr  # noqa: F401  (lib: the fixture)

pytestmark = pytest.mark.gpu

PANELS = {7: (128,), 1003: (1024, 128), 20001: (20096, 4096), 49200: (49152, 8192)}
KS = (1, 20, 64)
B = 8
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
DOM = I32_MAX                                          # the code of the dominant category of rows 3 and 5


_BASE = {}


def base(N):
    """scores, keys and labels of one catalog size: computed once, shared by every k and m, never written"""
    if N not in _BASE:
        rng = np.random.RandomState(N)
        ldn = (N + 127) // 128 * 128
        x = (rng.standard_normal((B, ldn)) * 2).astype(np.float32)
        x[4, :N] = -0.75                                   # all-tie row
        x[2, : N // 2] = x[2, 0]                           # half the row tied at one value
        x[:, N:] = 1e9                                     # padding columns must never be picked
        key = (rng.permutation(N) - N // 2).astype(np.int32)          # distinct, about half of them negative
        out_half = int(np.where(key >= 0)[0][0])           # an item outside the window [-N/2, 0) of rows 2 and 7
        lab = np.array([0, N // 3, N // 2, N - 4, N - 2, 1, 0, out_half], np.int32)
        codes = np.unique(np.r_[rng.randint(I32_MIN, I32_MAX, max(N // 3, 2), dtype=np.int64), -1, I32_MIN, 0])
        codes = codes[codes != DOM]
        assert (codes < 0).any() and (codes > 0).any()
        rand = codes[rng.randint(0, len(codes), N)].astype(np.int32)
        for a in (x, key, lab, rand):
            a.setflags(write=False)
        _BASE[N] = dict(x=x, key=key, lab=lab, ldn=ldn, rand=rand)
    return _BASE[N]


def case(N, k, m):
    """the rows that depend on k and m (3 and 5), the three category tables, and configuration B's windows and exclusion lists"""
    r = base(N)
    x = r["x"].copy()
    D = max(1, min(2 * k, 128, N // 2))                    # the dominant items 0 .. D - 1: in the first panel of every partition
    x[3, :D] = 50 + 0.25 * np.random.RandomState(k).permutation(D)
    F = min(m, D)                                          # row 5: items 0 .. F - 1 lead, the LAST item of the catalog beats them
    x[5, :F] = 200 + np.arange(F)
    x[5, N - 1] = 300
    rand = r["rand"].copy()
    rand[:D] = DOM
    rand[N - 1] = DOM
    tables = {"one": np.full(N, -5, np.int32), "rand": rand, "mod5": (np.arange(N) % 5).astype(np.int32)}
    lo, hi = np.full(B, I32_MIN, np.int64), np.full(B, I32_MAX, np.int64)
    lo[2], hi[2] = lo[7], hi[7] = -(N // 2), 0
    assert not lo[7] <= r["key"][r["lab"][7]] < hi[7]      # row 7: the label's key lies outside its window
    pool = (lo[:, None] <= r["key"][None, :]) & (r["key"][None, :] < hi[:, None])
    pool |= np.arange(N)[None, :] == r["lab"][:, None]     # a labelled call: the label is always in the pool
    x.setflags(write=False)
    return dict(r, x=x, tables=tables, lo=lo.astype(np.int32), hi=hi.astype(np.int32), pool=pool, D=D, F=F)


def best_of_every_category(x_row, cat, N):
    order = np.argsort(x_row[:N], kind="stable")[::-1]
    _, first = np.unique(cat[order], return_index=True)
    return np.sort(order[first]).astype(np.int32)


def exclusions(c, cat, N):
    """row 6: the best item of every category; rows 0 and 7: the two best items; the other rows: nothing"""
    six = best_of_every_category(c["x"][6], cat, N)
    excl = np.full((B, len(six) + 2), -1, np.int32)
    excl[6, :len(six)] = six
    for b in (0, 7):
        excl[b, :2] = np.argsort(c["x"][b, :N], kind="stable")[::-1][:2]
    return excl


def model(c, cat, N, k, m, pool=None, excl=None):
    x, lab = c["x"], c["lab"]
    lists, rank = [], np.zeros(B, np.int32)
    for b in range(B):
        inpool = np.ones(N, bool) if pool is None else pool[b]
        elig = inpool.copy()
        if excl is not None:
            elig[excl[b][excl[b] >= 0]] = False
        lists.append(capped_walk(x[b, :N], cat, k, m, elig))
        ids = np.where(inpool)[0]
        rank[b] = 1 + int(((x[b, ids] > x[b, lab[b]]) & (ids != lab[b])).sum())
    return lists, rank


class Runner:
    """the device copies of one case, and one reset / folds / finish per call"""

    def __init__(self, lib, c, N, k):
        self.lib, self.c, self.N, self.k = lib, c, N, k
        self.d = torch.tensor(c["x"]).cuda()
        self.dl = torch.tensor(c["lab"]).cuda()
        self.ls = self.d[torch.arange(B), self.dl.long()].contiguous()
        self.dk, self.dlo, self.dhi = (torch.tensor(c[n]).cuda() for n in ("key", "lo", "hi"))
        self.cats = {n: torch.tensor(t).cuda() for n, t in c["tables"].items()}

    def __call__(self, P, table=None, cap=0, window=False, excl=None, reverse=False):
        lib, N, k, d = self.lib, self.N, self.k, self.d
        state = torch.empty(int(lib.tcar_select_state_bytes(B, k)) // 4, dtype=torch.int32, device="cuda")
        topk = torch.full((B, k), -7, dtype=torch.int32, device="cuda")
        score = torch.full((B, k), -7.0, device="cuda")
        rank = torch.full((B,), -7, dtype=torch.int32, device="cuda")
        ce = torch.full((B,), -7.0, device="cuda")
        de, X = (torch.tensor(excl).cuda(), excl.shape[1]) if excl is not None else (None, 0)
        win = (ptr(self.dk), ptr(self.dlo), ptr(self.dhi)) if window else (None, None, None)
        assert lib.tcar_select_reset(B, k, ptr(state), None) == 0
        starts = list(range(0, N, P))
        for n0 in (starts[::-1] if reverse else starts):
            args = (B, n0, min(P, N - n0), ptr(d, n0), self.c["ldn"], k, ptr(self.dl), ptr(self.ls), ptr(de) if X else None, X,
                    ptr(state), None) + win
            if table is None:
                assert lib.tcar_select_panel_window(*args) == 0
            else:
                assert self.cats[table].numel() == N                  # the fold reads cat[n0 .. n0 + n) and cat[index]: inside the table
                assert lib.tcar_select_panel_quota(*args, ptr(self.cats[table]), cap) == 0
        assert lib.tcar_select_finish(B, k, ptr(state), ptr(self.ls), ptr(topk), ptr(score), ptr(rank), ptr(ce), None) == 0
        torch.cuda.synchronize()
        return topk.cpu().numpy(), score.cpu().numpy(), rank.cpu().numpy(), ce.cpu().numpy(), state.cpu().numpy()


def check_lists(x, k, tk, sc, want_lists, name):
    for b in range(B):
        want = want_lists[b]
        assert tk[b].tolist() == want + [-1] * (k - len(want)), (name, b, tk[b].tolist(), want)
        n = len(want)
        assert (sc[b, :n].view(np.int32) == x[b, want].view(np.int32)).all(), (name, b)        # bit for bit
        assert (sc[b, n:] == -7.0).all(), (name, b)                                            # untouched where the list ends


@pytest.mark.parametrize("mi", (0, 1, 2))
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("N", sorted(PANELS))
def test_capped_selection_is_the_walk_for_every_partition(lib, N, k, mi):
    m = (1, 2, k)[mi]
    c = case(N, k, m)
    x = c["x"]
    run = Runner(lib, c, N, k)
    parts = [(P, False) for P in PANELS[N]] + [(PANELS[N][-1], True)]       # every partition, and the smallest panels in reverse order
    for window in (False, True):                                            # configuration A, configuration B
        plain = {part: run(part[0], window=window, reverse=part[1]) for part in parts}
        for name, cat in c["tables"].items():
            excl = exclusions(c, cat, N) if window else None
            pool = c["pool"] if window else None
            lists, rank_w = model(c, cat, N, k, m, pool, excl)
            tag = "N=%d k=%d m=%d %s %s" % (N, k, m, name, "B" if window else "A")
            # what the cases are, in the model itself
            cats_of = [cat[l] for l in lists]
            assert all(np.unique(co, return_counts=True)[1].max() <= m for co in cats_of if len(co)), tag
            if name == "one" and not window:
                assert all(len(l) == min(m, k, N) for l in lists), tag                            # m items, then -1
            if name == "mod5" and not window:
                want4 = [i for i in range(N - 1, -1, -1)][:min(5 * m, N)]         # all tie: ids descending, m rounds over the 5 codes
                assert lists[4] == capped_walk(x[4, :N], cat, k, m) and (m >= k or lists[4] == want4[:k]), tag
            if name == "rand" and not window and m < k and N > 128:
                P0 = PANELS[N][-1]
                uncapped = np.argsort(x[3, :N], kind="stable")[::-1][:min(2 * k, 128)]
                assert (cat[uncapped] == DOM).all() and uncapped.max() < P0, tag                  # row 3: the 2k best share one code
                assert (cat[lists[3]] == DOM).sum() == m and len(lists[3]) == k, tag
                first = capped_walk(x[5, :P0], cat[:P0], k, m)                                    # row 5 after the first panel ...
                assert (cat[first] == DOM).sum() == m == c["F"] and first[:m] == list(range(m - 1, -1, -1)), tag
                assert lists[5][0] == N - 1 and 0 not in lists[5] and (cat[lists[5]] == DOM).sum() == m, tag   # ... and at the end
            if window:
                six = excl[6][excl[6] >= 0]
                assert not set(lists[6]) & set(six.tolist()) and len(six) == len(np.unique(cat)), tag
                lab7 = int(c["lab"][7])
                assert not c["lo"][7] <= c["key"][lab7] < c["hi"][7] and c["pool"][7, lab7], tag
            outs = []
            for part in parts:
                P, rev = part
                tk, sc, rank, ce, state = run(P, name, m, window=window, excl=excl, reverse=rev)
                t = "%s P=%d%s" % (tag, P, " reversed" if rev else "")
                check_lists(x, k, tk, sc, lists, t)
                assert (rank == rank_w).all(), (t, rank, rank_w)
                ptk, psc, prank, pce, pstate = plain[part] if excl is None else run(P, window=window, excl=excl, reverse=rev)
                assert (rank == prank).all() and ce.tobytes() == pce.tobytes(), t              # the cap does not touch rank and ce
                if m >= k:                                                                     # the uncapped call: output and raw state
                    assert tk.tobytes() == ptk.tobytes() and sc.tobytes() == psc.tobytes() and state.tobytes() == pstate.tobytes(), t
                outs.append((tk, sc, rank))
            for o in outs[1:]:
                for a, b in zip(outs[0], o):
                    assert a.tobytes() == b.tobytes(), tag


def test_a_fold_whose_category_slice_is_not_16_byte_aligned(lib):
    """one direct call with n0 = 3 on a panel buffer of its own: column j is item 3 + j, so the fold reads cat[3 + j]; the all-tie row
    takes the register path and its kill passes"""
    N, k, m, n0 = 1500, 20, 1, 3
    rng = np.random.RandomState(5)
    n = N - n0
    ld = (n + 127) // 128 * 128
    x = (rng.standard_normal((B, N)) * 2).astype(np.float32)
    x[4] = 0.5
    x[3, n0:n0 + 40] = 60 + np.arange(40)
    cat = (np.arange(N) % 11 - 3).astype(np.int32)
    cat[n0:n0 + 40] = DOM
    panel = np.full((B, ld), 1e9, np.float32)
    panel[:, :n] = x[:, n0:]
    elig = np.arange(N) >= n0
    want = [capped_walk(x[b], cat, k, m, elig) for b in range(B)]
    assert want[4] == list(range(N - 1, N - 12, -1)) + [n0 + 39] and (cat[want[3]] == DOM).sum() == m and len(want[3]) == 12
    d, dc = torch.tensor(panel).cuda(), torch.tensor(cat).cuda()
    assert (dc.data_ptr() + 4 * n0) % 16 != 0
    state = torch.empty(int(lib.tcar_select_state_bytes(B, k)) // 4, dtype=torch.int32, device="cuda")
    topk = torch.full((B, k), -7, dtype=torch.int32, device="cuda")
    score = torch.full((B, k), -7.0, device="cuda")
    assert lib.tcar_select_reset(B, k, ptr(state), None) == 0
    assert lib.tcar_select_panel_quota(B, n0, n, ptr(d), ld, k, None, None, None, 0, ptr(state), None, None, None, None, ptr(dc), m) == 0
    assert lib.tcar_select_finish(B, k, ptr(state), None, ptr(topk), ptr(score), None, None, None) == 0
    torch.cuda.synchronize()
    check_lists(x, k, topk.cpu().numpy(), score.cpu().numpy(), want, "n0 = 3")


def test_cap_argument_errors_leave_the_state_untouched(lib):
    N, k = 1003, 20
    c = case(N, k, 2)
    run = Runner(lib, c, N, k)
    state = torch.empty(int(lib.tcar_select_state_bytes(B, k)) // 4, dtype=torch.int32, device="cuda")
    assert lib.tcar_select_reset(B, k, ptr(state), None) == 0
    args = (B, 0, 1003, ptr(run.d), c["ldn"], k, ptr(run.dl), ptr(run.ls), None, 0, ptr(state), None, None, None, None)
    assert lib.tcar_select_panel_quota(*args, ptr(run.cats["rand"]), 2) == 0
    torch.cuda.synchronize()
    before = state.cpu().numpy().copy()
    assert lib.tcar_select_panel_quota(*args, ptr(run.cats["rand"]), 0) == -1            # a table with cap = 0
    assert lib.tcar_select_panel_quota(*args, ptr(run.cats["rand"]), -2) == -1
    assert lib.tcar_select_panel_quota(*args, None, 2) == -1                             # a cap without a table
    torch.cuda.synchronize()
    assert state.cpu().numpy().tobytes() == before.tobytes()
