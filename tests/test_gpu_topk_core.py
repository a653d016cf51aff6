"""The two front ends of the row-resident top-k core (csrc/topk_rows.h) against numpy and against each other: tcar_eval_rows
(rank_topk_rows_kernel) and one whole-row fold of the streamed selection (tcar_select_reset / _panel / _finish), on the same matrix.

What each size reaches (`candidates_at_or_above_threshold` below restates phases A and B on the CPU, and a test without a kernel
asserts these counts before anything runs on the GPU):

  N = 7      k > N: the -1 tail; -inf entries enter the list by index; fewer than k threads hold anything (threshold = nothing).
  N = 1003   phase C; R = 8 in eval_rows, R = 2 in the fold.
  N = 5000   phase C; R = 8 in both front ends.
  N = 16000  R = 8 in both, slices nearly full.  k = 64: the block row overflows the LDS (1,305 candidates > CAP = 1,024): the FALLBACK.
  N = 16500  R = 24 in both.  k = 64: the block row overflows the LDS (1,420 candidates): the fallback.

Phase A's threshold is exact in the index, so tie rows do NOT overflow (an all-tie row passes the highest indices of about k threads,
under 100 candidates here): every row but the block row takes phase C at every size and k (506 candidates at most).  The block row gives the largest values
of the row to the columns of 40 threads; with k = 64 > 40 the threshold falls among the other threads' bests and every block column
is at or above it.  k = 0 extracts and writes nothing."""
import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401

from gpu_util import close, lib, ptr  # noqa: F401  (lib: the fixture)

pytestmark = pytest.mark.gpu

SIZES = {7: 128, 1003: 1024, 5000: 5120, 16000: 16000, 16500: 16512}          # N -> ld
KS = (0, 1, 20, 64)
SAME_R = (5000, 16000, 16500)       # both front ends keep the row in R = 8 / 8 / 24 float4 per thread and sum in the same order
B = 8
GUARD = 4
NT, CAP = 512, 1024                 # threads of a workgroup, LDS candidates (csrc/topk_rows.h)
BLOCK_THREADS = 40                  # threads that own the block row's largest values: more than 20, fewer than 64
FALLBACK = ((16000, 64), (16500, 64))         # (N, k) at which the block row overflows the LDS

_CASES = {}


def case(N):
    """inputs and the numpy reference of one catalog size (rows as in select_case.case, plus a row of -inf): computed once,
    shared by every k, never written"""
    if N in _CASES:
        return _CASES[N]
    from oracle.metrics_oracle import topk_list
    rng = np.random.RandomState(N)
    ld = SIZES[N]
    x = (rng.standard_normal((B, ld)) * 2).astype(np.float32)       # rows 0, 4 and 5: random
    x[1, :N] = -0.75                                      # all-tie row: top-k is the highest indices
    x[2, : N // 2] = x[2, 0]                              # half the row tied at one value
    x[3, N - 1] = 50.0                                    # the winner sits in the last column
    fin = (N // 4, N - 2)                                 # row 6: -inf everywhere but two columns; the label is one of them
    x[6, :N] = -np.inf
    x[6, fin[0]], x[6, fin[1]] = 1.5, -2.0
    cols = np.arange(N)                                   # row 7, the block row: the columns of 40 threads hold the largest values
    block = cols[(cols // 4) % NT < BLOCK_THREADS]        # (thread t keeps the columns c with (c // 4) % 512 == t)
    x[7, block] = 10.0 + rng.permutation(len(block)).astype(np.float32) / 8
    x[:, N:] = 1e9                                        # padding columns must never be picked
    lab = np.array([0, N - 1, N // 3, N - 1, min(5, N - 1), N // 2, fin[0], min(12, N - 1)], np.int32)
    xv = x[:, :N].astype(np.float64)
    ref = {"x": x, "lab": lab, "ld": ld,
           "top": [topk_list(x[b, :N], max(KS)) for b in range(B)],
           "rank": ((xv > xv[np.arange(B), lab][:, None]).sum(1) + 1).astype(np.int32),
           "ce": np.log(np.exp(xv - xv.max(1, keepdims=True)).sum(1)) + xv.max(1) - xv[np.arange(B), lab]}
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CASES[N] = ref
    return ref


def candidates_at_or_above_threshold(row, k):
    """phases A and B of the core for one row of live columns and an empty running list: the number of candidates at or above L,
    the k-th largest of the per-thread bests in list order (fewer than k threads with a column: every candidate qualifies)"""
    N = len(row)
    pos = np.empty(N, np.int64)
    pos[np.lexsort((np.arange(N), row))] = np.arange(N)            # place in ascending list order: score, then index
    best = np.full(NT, -1, np.int64)
    np.maximum.at(best, (np.arange(N) // 4) % NT, pos)
    best = np.sort(best[best >= 0])[::-1]
    return N if len(best) < k else int((pos >= best[k - 1]).sum())


def test_the_sizes_reach_the_paths_the_docstring_names():
    """(no kernel) phase C everywhere but the block row at FALLBACK, which overflows the LDS"""
    for N in SIZES:
        x = case(N)["x"]
        for k in KS[1:]:
            for b in range(B):
                nc = candidates_at_or_above_threshold(x[b, :N], k)
                if b == 7 and (N, k) in FALLBACK:
                    assert nc > CAP, (N, k, nc)
                else:
                    assert nc <= CAP, (N, k, b, nc)
    assert candidates_at_or_above_threshold(case(16000)["x"][7, :16000], 64) == 1305         # 1,280 block columns + 24 better bests of other threads + L itself
    assert candidates_at_or_above_threshold(case(16500)["x"][7, :16500], 64) == 1420
    assert candidates_at_or_above_threshold(case(7)["x"][1, :7], 20) == 7          # two threads hold the seven columns


def test_the_reference_handles_the_row_of_minus_infinity():
    """(no kernel: the oracle's list and the numpy rank / CE of row 6, by hand, before anything is compared with them)"""
    for N in SIZES:
        ref = case(N)
        a, b = N // 4, N - 2                              # 1.5 and -2.0; every other column is -inf, the higher index first
        rest = [i for i in range(N - 1, -1, -1) if i not in (a, b)]
        assert ref["top"][6] == ([a, b] + rest)[:max(KS)]
        assert ref["rank"][6] == 1
        assert abs(ref["ce"][6] - np.log1p(np.exp(-3.5))) < 1e-12


def eval_rows(lib, ref, N, k):
    """tcar_eval_rows -> topk (None for k = 0), rank, ce; rank and ce sit inside guard words, which must stay as they were"""
    d, dl = torch.tensor(ref["x"]).cuda(), torch.tensor(ref["lab"]).cuda()
    rank = torch.full((B + 2 * GUARD,), -7, dtype=torch.int32, device="cuda")
    ce = torch.full((B + 2 * GUARD,), -7.0, device="cuda")
    topk = torch.full((B, k), -7, dtype=torch.int32, device="cuda") if k else None
    assert lib.tcar_eval_rows(B, N, ptr(d), ref["ld"], ptr(dl), k, ptr(rank, GUARD), ptr(topk) if k else None, ptr(ce, GUARD),
                              None) == 0
    torch.cuda.synchronize()
    assert (d.cpu().numpy().view(np.int32) == ref["x"].view(np.int32)).all()          # the scores are left untouched
    rank, ce = rank.cpu().numpy(), ce.cpu().numpy()
    for g in (rank, ce):
        assert (g[:GUARD] == -7).all() and (g[GUARD + B:] == -7).all()
    return topk.cpu().numpy() if k else None, rank[GUARD:GUARD + B], ce[GUARD:GUARD + B]


def fold_row(lib, ref, N, k):
    """reset, ONE tcar_select_panel over the whole row, finish -> topk, score, rank, ce"""
    d, dl = torch.tensor(ref["x"]).cuda(), torch.tensor(ref["lab"]).cuda()
    ls = d[torch.arange(B), dl.long()].contiguous()       # gathered from x: exact
    state = torch.empty(int(lib.tcar_select_state_bytes(B, k)) // 4, dtype=torch.int32, device="cuda")
    topk = torch.full((B, k), -7, dtype=torch.int32, device="cuda")
    score = torch.full((B, k), -7.0, device="cuda")
    rank = torch.empty(B, dtype=torch.int32, device="cuda")
    ce = torch.empty(B, device="cuda")
    assert lib.tcar_select_reset(B, k, ptr(state), None) == 0
    assert lib.tcar_select_panel(B, 0, N, ptr(d), ref["ld"], k, ptr(dl), ptr(ls), None, 0, ptr(state), None) == 0
    assert lib.tcar_select_finish(B, k, ptr(state), ptr(ls), ptr(topk), ptr(score), ptr(rank), ptr(ce), None) == 0
    torch.cuda.synchronize()
    assert (d.cpu().numpy().view(np.int32) == ref["x"].view(np.int32)).all()
    return topk.cpu().numpy(), score.cpu().numpy(), rank.cpu().numpy(), ce.cpu().numpy()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("N", sorted(SIZES))
def test_eval_rows_and_one_fold_give_the_same_list_rank_and_ce(lib, N, k):
    ref = case(N)
    x = ref["x"]
    tk_e, rank_e, ce_e = eval_rows(lib, ref, N, k)
    assert (rank_e == ref["rank"]).all(), (rank_e, ref["rank"])
    close(ce_e, ref["ce"], name="ce eval_rows")
    if k == 0:
        return                                            # (the fold takes k >= 1)
    tk_f, sc_f, rank_f, ce_f = fold_row(lib, ref, N, k)
    assert (rank_f == ref["rank"]).all(), (rank_f, ref["rank"])
    close(ce_f, ref["ce"], name="ce fold")
    for b in range(B):
        want = ref["top"][b][:k]
        n = len(want)
        want = want + [-1] * (k - n)
        assert tk_e[b].tolist() == want, ("eval_rows", b, tk_e[b].tolist(), want)
        assert tk_f[b].tolist() == want, ("fold", b, tk_f[b].tolist(), want)
        assert (sc_f[b, :n].view(np.int32) == x[b, want[:n]].view(np.int32)).all(), b        # the matrix entries, bit for bit
        assert (sc_f[b, n:] == -7.0).all(), b                                                  # untouched where the list ends
    assert tk_e.tobytes() == tk_f.tobytes()
    if N in SAME_R:                                       # same R, same order of every sum, the same expression: the same bits
        assert ce_e.tobytes() == ce_f.tobytes(), (ce_e, ce_f)
