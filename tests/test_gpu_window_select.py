"""Windowed streamed selection at the op level (include/tcar_window.h: tcar_select_panel_window) against numpy, exactly.

Built like test_gpu_select.py: one fp32 matrix x [B, ldn] per catalog size, the panels pointer views into it; one int32 key per item
and one half-open window [lo, hi) per row.  Item n is in the pool of row b iff lo[b] <= key[n] < hi[b], or (labelled call) n is the
row's label.  The list, its scores and the rank follow a total order inside the pool, so they must be the same bits for every
partition and on every run; ce is an online sum (that file's `close`).

One row per case:
  0  window = all of int32: the bits of tcar_select_panel         4  pool and label only in the LAST panel (empty slices, empty state)
  1  lo == hi: the label alone / nothing                          5  pool only in the first panel
  2  about half the catalog                                       6  exactly min(k, N) items in the pool
  3  all-tie row, fewer than k items in the pool                  7  the label outside its own window"""
import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401

from gpu_util import close, lib, ptr  # noqa: F401  (lib: the fixture)

pytestmark = pytest.mark.gpu

# N -> panel sizes: the largest allowed (ceil128(N), at most 49,152) and a smaller one.  Together they reach R = 2, 8 and 24.
PANELS = {7: (128,), 1003: (1024, 128), 20001: (20096, 4096), 49200: (49152, 8192)}
KS = (1, 20, 64)
B = 8
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
LATE, EARLY = 1_000_000, -1_000_000                  # reserved key values of a few items at the end / the start of the catalog


_CASES = {}


def case(N):
    """scores, keys and labels of one catalog size: computed once, shared by every k and partition, never written"""
    if N in _CASES:
        return _CASES[N]
    rng = np.random.RandomState(N)
    ldn = (N + 127) // 128 * 128
    x = (rng.standard_normal((B, ldn)) * 2).astype(np.float32)
    x[3, :N] = -0.75                                      # all-tie row: the list is the highest ids of the pool
    x[2, : N // 2] = x[2, 0]                              # half the row tied at one value
    x[4, 0] = 50.0                                        # row 4: the catalog's winner is OUT of the pool (first panel, pool in the last)
    x[:, N:] = 1e9                                        # padding columns must never be picked
    # a permutation of [-N/2, N - N/2): distinct, about half of them negative; the last / first items carry reserved values, so an
    # interval of keys can name "only items of the last panel" / "only items of the first panel" for every partition
    key = (rng.permutation(N) - N // 2).astype(np.int32)
    late = [N - 4, N - 2, N - 1]                          # all in the last panel of every partition (its last 4 columns)
    early = [0, 1]
    key[late] = [LATE, LATE + 1, LATE + 2]
    key[early] = [EARLY, EARLY - 1]
    out_half = int(np.where((key >= 0) & (key < LATE))[0][0])       # an item outside the window [-N/2, 0) of rows 2 and 7
    lab = np.array([0, N // 3, N // 2, N - 4, N - 2, 1, 0, out_half], np.int32)
    ref = {"x": x, "key": key, "lab": lab, "ldn": ldn, "late": late, "early": early}
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CASES[N] = ref
    return ref


def windows(ref, N, k):
    """[lo, hi) of the eight rows.  Row 6 depends on k: the min(k, N) smallest keys from the label's on."""
    key, lab = ref["key"], ref["lab"]
    lo, hi = np.zeros(B, np.int64), np.zeros(B, np.int64)
    lo[0], hi[0] = I32_MIN, I32_MAX
    lo[1], hi[1] = 5, 5
    lo[2], hi[2] = -(N // 2), 0
    lo[3], hi[3] = LATE + 1, LATE + 3                     # items N - 2 and N - 1, + the label N - 4: three items
    lo[4], hi[4] = LATE, LATE + 3
    lo[5], hi[5] = EARLY - 1, EARLY + 1
    kk = min(k, N)
    srt = np.sort(key.astype(np.int64))
    j = min(int(np.searchsorted(srt, key[lab[6]])), N - kk)
    lo[6], hi[6] = srt[j], srt[j + kk - 1] + 1
    assert ((srt >= lo[6]) & (srt < hi[6])).sum() == kk
    lo[7], hi[7] = -(N // 2), 0
    assert not lo[7] <= key[lab[7]] < hi[7]               # row 7: the label's key lies outside its window
    return lo.astype(np.int32), hi.astype(np.int32)


def model(x, key, lab, lo, hi, k, items, labelled, excl=None):
    """the numpy model over the item ids `items` (ascending): lists, ranks, fp64 cross entropy"""
    from oracle.metrics_oracle import topk_list
    lists, rank, ce = [], np.zeros(B, np.int32), np.zeros(B)
    items = np.asarray(items)
    for b in range(B):
        pool = (lo[b] <= key[items]) & (key[items] < hi[b])
        if labelled:
            pool |= items == lab[b]
        ids = items[pool]
        keep = ids if excl is None else np.setdiff1d(ids, excl[b][excl[b] >= 0])
        lists.append([int(keep[j]) for j in topk_list(x[b, keep], k)])
        if labelled:
            xp, xl = x[b, ids].astype(np.float64), np.float64(x[b, lab[b]])
            rank[b] = 1 + int(((xp > xl) & (ids != lab[b])).sum())
            ce[b] = np.log(np.exp(xp - xp.max()).sum()) + xp.max() - xl
    return lists, rank, ce


def run(lib, ref, N, k, P, lo=None, hi=None, labelled=True, excl=None, plain=False):
    """reset, one fold per panel of P columns (the last one partial), finish -> numpy outputs.  plain: tcar_select_panel"""
    ldn = ref["ldn"]
    d = torch.tensor(ref["x"]).cuda()
    dl = torch.tensor(ref["lab"]).cuda()
    ls = d[torch.arange(B), dl.long()].contiguous()       # gathered from x: exact
    state = torch.empty(int(lib.tcar_select_state_bytes(B, k)) // 4, dtype=torch.int32, device="cuda")
    topk = torch.full((B, k), -7, dtype=torch.int32, device="cuda")
    score = torch.full((B, k), -7.0, device="cuda")
    rank = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    ce = torch.full((B,), -7.0, device="cuda")
    de, X = (torch.tensor(excl).cuda(), excl.shape[1]) if excl is not None else (None, 0)
    lsp = ptr(ls) if labelled else None
    if not plain:
        dk, dlo, dhi = torch.tensor(ref["key"]).cuda(), torch.tensor(lo).cuda(), torch.tensor(hi).cuda()
    assert lib.tcar_select_reset(B, k, ptr(state), None) == 0
    for n0 in range(0, N, P):
        args = (B, n0, min(P, N - n0), ptr(d, n0), ldn, k, ptr(dl), lsp, ptr(de) if X else None, X, ptr(state), None)
        if plain:
            assert lib.tcar_select_panel(*args) == 0
        else:
            assert lib.tcar_select_panel_window(*args, ptr(dk), ptr(dlo), ptr(dhi)) == 0
    assert lib.tcar_select_finish(B, k, ptr(state), lsp, ptr(topk), ptr(score), ptr(rank) if labelled else None,
                                  ptr(ce) if labelled else None, None) == 0
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == ref["x"]).all()            # the scores are left untouched
    return topk.cpu().numpy(), score.cpu().numpy(), rank.cpu().numpy(), ce.cpu().numpy()


def check_lists(x, k, tk, sc, want_lists):
    for b in range(B):
        want = want_lists[b][:k]
        assert tk[b].tolist() == want + [-1] * (k - len(want)), (b, tk[b].tolist(), want)
        n = len(want)
        assert (sc[b, :n].view(np.int32) == x[b, want].view(np.int32)).all(), b           # bit for bit
        assert (sc[b, n:] == -7.0).all(), b                                               # untouched where the list ends


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("N", sorted(PANELS))
def test_windowed_selection_is_exact_for_every_partition(lib, N, k):
    ref = case(N)
    x, key, lab = ref["x"], ref["key"], ref["lab"]
    lo, hi = windows(ref, N, k)
    lists, rank_w, ce_w = model(x, key, lab, lo, hi, k, np.arange(N), True)
    # what the cases are, in the model itself
    assert lists[1] == [int(lab[1])] and rank_w[1] == 1 and ce_w[1] == 0.0
    assert lists[3] == [N - 1, N - 2, N - 4][:k] and len(lists[3]) == min(k, 3)
    assert set(lists[4]) <= set(ref["late"]) and set(lists[5]) <= set(ref["early"])
    assert len(lists[6]) == min(k, N) and int(lab[7]) not in np.where((lo[7] <= key) & (key < hi[7]))[0]
    outs = []
    for P in PANELS[N] + (PANELS[N][0],):                 # every partition, the first one twice (two runs)
        tk, sc, rank, ce = run(lib, ref, N, k, P, lo, hi)
        check_lists(x, k, tk, sc, lists)
        assert (rank == rank_w).all(), (P, rank, rank_w)
        assert np.isfinite(ce).all(), (P, ce)
        close(ce, ce_w, name="ce P=%d" % P)
        assert ce[1] == 0.0                               # lo == hi: the label alone, exactly
        # row 0, the window that holds every key: the bits of the unwindowed fold of the same partition
        ptk, psc, prank, pce = run(lib, ref, N, k, P, plain=True)
        assert tk[0].tobytes() == ptk[0].tobytes() and sc[0].tobytes() == psc[0].tobytes()
        assert rank[0] == prank[0] and ce[0:1].tobytes() == pce[0:1].tobytes()
        outs.append((tk, sc, rank))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("N", sorted(PANELS))
def test_windowed_recommendation_without_a_label(lib, N, k):
    """no label rule: lo == hi is an empty pool (all -1, the scores untouched), the pools of rows 3 and 7 lose their label"""
    ref = case(N)
    lo, hi = windows(ref, N, k)
    lists, _, _ = model(ref["x"], ref["key"], ref["lab"], lo, hi, k, np.arange(N), False)
    assert lists[1] == [] and lists[3] == [N - 1, N - 2][:k] and int(ref["lab"][7]) not in lists[7]
    outs = []
    for P in PANELS[N]:
        tk, sc, rank, ce = run(lib, ref, N, k, P, lo, hi, labelled=False)
        check_lists(ref["x"], k, tk, sc, lists)
        assert (tk[1] == -1).all() and (rank == -7).all() and (ce == -7.0).all()
        outs.append((tk, sc))
    for o in outs[1:]:
        assert o[0].tobytes() == outs[0][0].tobytes() and o[1].tobytes() == outs[0][1].tobytes()


def test_exclusions_apply_on_top_of_a_window(lib):
    N, k, P, X = 1003, 20, 128, 6
    ref = case(N)
    x, key, lab = ref["x"], ref["key"], ref["lab"]
    lo, hi = windows(ref, N, k)
    pooled, _, _ = model(x, key, lab, lo, hi, k, np.arange(N), True)
    excl = np.full((B, X), -1, np.int32)
    for b in range(B):
        excl[b, 0] = excl[b, 3] = pooled[b][0]                          # the pool's winner, twice
        excl[b, 2] = pooled[b][min(2, len(pooled[b]) - 1)]              # one more of the list
        excl[b, 4] = int(np.where(~((lo[b] <= key) & (key < hi[b])))[0][-1]) if b != 0 else -1        # one that is out of the pool anyway
    want, _, _ = model(x, key, lab, lo, hi, k, np.arange(N), True, excl)
    assert want[1] == [] and want != pooled
    plain = run(lib, ref, N, k, P, lo, hi)
    tk, sc, rank, ce = run(lib, ref, N, k, P, lo, hi, excl=excl)
    check_lists(x, k, tk, sc, want)
    assert (rank == plain[2]).all() and ce.tobytes() == plain[3].tobytes()          # exclusion: the list only


def test_a_fold_whose_key_slice_is_not_16_byte_aligned(lib):
    """one direct call with n0 = 3 on a panel buffer of its own: column j is item 3 + j, so the fold reads key[3 + j]"""
    N, k, n0 = 1003, 20, 3
    ref = case(N)
    x, key, lab = ref["x"], ref["key"], ref["lab"]
    lo, hi = windows(ref, N, k)
    lab = np.where(lab < n0, n0 + 5, lab).astype(np.int32)              # every label among the folded items
    n = N - n0
    ld = (n + 127) // 128 * 128
    panel = np.full((B, ld), 1e9, np.float32)
    panel[:, :n] = x[:, n0:N]
    want, rank_w, ce_w = model(x, key, lab, lo, hi, k, np.arange(n0, N), True)
    d, dl = torch.tensor(panel).cuda(), torch.tensor(lab).cuda()
    ls = torch.tensor(x[np.arange(B), lab]).cuda()
    dk, dlo, dhi = torch.tensor(key).cuda(), torch.tensor(lo).cuda(), torch.tensor(hi).cuda()
    assert (dk.data_ptr() + 4 * n0) % 16 != 0
    state = torch.empty(int(lib.tcar_select_state_bytes(B, k)) // 4, dtype=torch.int32, device="cuda")
    topk = torch.full((B, k), -7, dtype=torch.int32, device="cuda")
    score = torch.full((B, k), -7.0, device="cuda")
    rank = torch.empty(B, dtype=torch.int32, device="cuda")
    ce = torch.empty(B, device="cuda")
    assert lib.tcar_select_reset(B, k, ptr(state), None) == 0
    assert lib.tcar_select_panel_window(B, n0, n, ptr(d), ld, k, ptr(dl), ptr(ls), None, 0, ptr(state), None, ptr(dk), ptr(dlo),
                                        ptr(dhi)) == 0
    assert lib.tcar_select_finish(B, k, ptr(state), ptr(ls), ptr(topk), ptr(score), ptr(rank), ptr(ce), None) == 0
    torch.cuda.synchronize()
    check_lists(x, k, topk.cpu().numpy(), score.cpu().numpy(), want)
    assert (rank.cpu().numpy() == rank_w).all()
    close(ce.cpu().numpy(), ce_w, name="ce, n0 = 3")
