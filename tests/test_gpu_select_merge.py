"""tcar_select_merge at the op level (include/tcar_serve_shard.h), exactly: the columns of the matrices of select_case are cut into S
pieces, every piece is folded into its OWN state with the existing fold calls, and the S states are merged and finished.  The list, its
scores and the rank must be the bits of the single-state run and of numpy; ce follows the repartitioned sum (gpu_util.close) and
is the same bits on every run."""
import ctypes as C

import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401

from gpu_util import close, lib, ptr  # noqa: F401  (lib: the fixture)
from select_case import KS, PANELS, case, check_lists, run
from select_ref import capped_walk

pytestmark = pytest.mark.gpu

NS = (7, 1003, 20001)
NAN_BITS = 0x7FC00000


def cuts_of(N, S):
    """S - 1 cuts of [0, N): multiples of 4 (panel rows stay 16-byte aligned), no multiple of 128 (so of no panel size); at N = 7 the
    only such cut is 4, and the other pieces are empty"""
    if S == 1:
        return []
    if N < 16:
        return [4] + [N] * (S - 2)
    out = []
    for i in range(1, S):
        c = int(round(N * i / S / 4.0)) * 4
        out.append(c + 4 if c % 128 == 0 else c)
    assert all(0 < c < N and c % 4 == 0 and c % 128 for c in out) and out == sorted(out)
    return out


def merged(lib, x, lab, N, k, cuts, P, S=None, gap=0, key=None, lo=None, hi=None, cat=None, cap=0, labelled=True):
    """x [B, ldn] fp32 on the host: piece s = columns [cuts[s-1], cuts[s]) folded into state s in panels of P columns; states past the
    pieces stay reset states; then tcar_select_merge over S states + tcar_select_finish -> numpy (topk, score, rank, ce, merged state)"""
    B, ldn = x.shape
    rw = 2 * k + 4
    edges = [0] + list(cuts) + [N]
    S = S or len(edges) - 1
    stride = B * rw + gap
    d, dl = torch.tensor(x).cuda(), torch.tensor(lab).cuda()
    ls = d[torch.arange(B), dl.long()].contiguous()
    states = torch.full((S * stride,), NAN_BITS, dtype=torch.int32, device="cuda")        # what lies between two shards' rows: NaN bits
    dev = lambda a: torch.tensor(a).cuda() if a is not None else None
    dkey, dlo, dhi, dcat = dev(key), dev(lo), dev(hi), dev(cat)
    p = lambda t: ptr(t) if t is not None else None
    for s in range(S):
        assert lib.tcar_select_reset(B, k, ptr(states, s * stride), None) == 0
    for s in range(len(edges) - 1):
        for n0 in range(edges[s], edges[s + 1], P):
            n = min(P, edges[s + 1] - n0)
            assert lib.tcar_select_panel_quota(B, n0, n, ptr(d, n0), ldn, k, ptr(dl) if labelled else None, ptr(ls) if labelled else None,
                                               None, 0, ptr(states, s * stride), None, p(dkey), p(dlo), p(dhi), p(dcat), cap) == 0
    out = torch.full((B * rw,), NAN_BITS, dtype=torch.int32, device="cuda")
    topk = torch.full((B, k), -7, dtype=torch.int32, device="cuda")
    score = torch.full((B, k), -7.0, device="cuda")
    rank = torch.empty(B, dtype=torch.int32, device="cuda")
    ce = torch.empty(B, device="cuda")
    assert lib.tcar_select_merge(B, k, S, ptr(states), stride, ptr(out), p(dcat), cap, None) == 0
    assert lib.tcar_select_finish(B, k, ptr(out), ptr(ls) if labelled else None, ptr(topk), ptr(score), ptr(rank) if labelled else None,
                                  ptr(ce) if labelled else None, None) == 0
    torch.cuda.synchronize()
    if gap:                                                # the gap was neither written nor (it would show in the results) read
        g = states.view(S, stride)[:, B * rw:].cpu().numpy()
        assert (g == NAN_BITS).all()
    return topk.cpu().numpy(), score.cpu().numpy(), rank.cpu().numpy(), ce.cpu().numpy(), out.cpu().numpy().reshape(B, rw)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("N", NS)
def test_merged_shard_states_give_the_bits_of_one_state(lib, N, k):
    ref = case(N)
    P = min(PANELS[N])
    one = run(lib, ref, N, k, P)
    for S in (1, 2, 3, 8) + ((64,) if N == 7 else ()):
        cuts = cuts_of(N, min(S, 8))
        got = [merged(lib, ref["x"], ref["lab"], N, k, cuts, P, S=S) for _ in range(2)]
        tk, sc, rank, ce, st = got[0]
        check_lists(ref, N, k, tk, sc, ref["top"])                        # numpy: lists, scores bit for bit, -1 tails
        assert (rank == ref["rank"]).all(), (S, rank, ref["rank"])
        close(ce, ref["ce"], name="ce S=%d" % S)
        for a, b in zip((tk, sc, rank), one[:3]):                         # the single-state run
            assert a.tobytes() == b.tobytes(), S
        for a, b in zip(got[0], got[1]):                                  # two runs: every output, ce and the state included
            assert a.tobytes() == b.tobytes(), S
        # slots past the end of a list hold -inf / -1, the pad word 0
        n_live = (st[:, k:2 * k] >= 0).sum(1)
        for b in range(ref["B"]):
            assert (st[b, n_live[b]:k].view(np.float32) == -np.inf).all() and (st[b, k + n_live[b]:2 * k] == -1).all()
        assert (st[:, 2 * k + 3] == 0).all()


def test_shards_shorter_than_k_leave_minus_one_tails(lib):
    N, k = 7, 20
    ref = case(N)
    tk, sc, rank, ce, st = merged(lib, ref["x"], ref["lab"], N, k, [4], 128)
    assert (tk[:, :7] >= 0).all() and (tk[:, 7:] == -1).all() and (sc[:, 7:] == -7.0).all()
    check_lists(ref, N, k, tk, sc, ref["top"])


def test_windowed_shards_and_an_unread_gap_between_the_states(lib):
    """keys = item ids, so a window is an id range: session 0's pool lies inside shard 0 (shards 1 and 2 fold nothing for it: their
    (max, sum) stay (-inf, 0)), session 1's pool is its label alone, session 2's is empty but for the label too (lo > hi), the others see
    parts of several shards.  stride_words > B (2k + 4): what lies between is NaN bits."""
    from oracle.metrics_oracle import topk_list
    N, k, S = 1003, 20, 3
    ref = case(N)
    x, lab, B = ref["x"], ref["lab"], ref["B"]
    cuts = cuts_of(N, S)
    key = np.arange(N, dtype=np.int32)
    lo = np.array([10, 5, 900, cuts[0] - 7, 0, cuts[1]], np.int32)
    hi = np.array([cuts[0] - 3, 5, 100, cuts[1] + 9, N, N], np.int32)
    tk, sc, rank, ce, st = merged(lib, x, lab, N, k, cuts, 128, gap=13, key=key, lo=lo, hi=hi)
    again = merged(lib, x, lab, N, k, cuts, 128, gap=13, key=key, lo=lo, hi=hi)
    single = merged(lib, x, lab, N, k, [], 1024, key=key, lo=lo, hi=hi)              # one state over the whole range
    want = []
    for b in range(B):
        pool = (key >= lo[b]) & (key < hi[b])
        pool[lab[b]] = True
        ids = np.where(pool)[0]
        want.append([int(ids[j]) for j in topk_list(x[b, ids], k)])
        xv = x[b, ids].astype(np.float64)
        assert rank[b] == 1 + int(((x[b, ids] > x[b, lab[b]]) & (ids != lab[b])).sum()), b
        close(ce[b:b + 1], [np.log(np.exp(xv - xv.max()).sum()) + xv.max() - float(x[b, lab[b]])], name="ce %d" % b)
    check_lists(ref, N, k, tk, sc, want)
    assert want[1] == [int(lab[1])] and want[2] == [int(lab[2])] and rank[1] == 1 and ce[1] == 0.0        # the label alone
    assert np.isfinite(ce).all() and not np.isnan(st.view(np.float32)[:, 2 * k + 1:2 * k + 3]).any()
    for a, b in zip((tk, sc, rank), single[:3]):
        assert a.tobytes() == b.tobytes()
    for a, b in zip((tk, sc, rank, ce, st), again):
        assert a.tobytes() == b.tobytes()


def test_all_shards_empty_give_minus_inf_and_zero(lib):
    """recommendation (no label) with a window that holds nothing: every shard state stays a reset state"""
    N, k = 1003, 20
    ref = case(N)
    B = ref["B"]
    key = np.arange(N, dtype=np.int32)
    lo, hi = np.full(B, 5, np.int32), np.full(B, 5, np.int32)
    tk, sc, _, _, st = merged(lib, ref["x"], ref["lab"], N, k, cuts_of(N, 3), 128, key=key, lo=lo, hi=hi, labelled=False)
    assert (tk == -1).all() and (sc == -7.0).all()
    f = st.view(np.float32)
    assert (st[:, 2 * k] == 0).all() and (f[:, 2 * k + 1] == -np.inf).all() and (f[:, 2 * k + 2] == 0.0).all()


def _capped_case(N, k, cuts):
    """the matrix of case(N) with 3k columns of EVERY piece lifted above everything else, all of one category: every shard's capped list
    has to reach far below its k best scores"""
    ref = case(N)
    x = ref["x"].copy()
    rng = np.random.RandomState(5)
    cat = (1 + np.arange(N) % 11).astype(np.int32)
    edges = [0] + list(cuts) + [N]
    for s in range(len(edges) - 1):
        cols = edges[s] + rng.choice(edges[s + 1] - edges[s], 3 * k, replace=False)
        x[:, cols] += np.float32(100.0)
        cat[cols] = 0
    return ref, x, cat


@pytest.mark.parametrize("m", (1, 3))
def test_capped_merge_is_the_capped_walk_over_the_whole_row(lib, m):
    N, k, S = 1003, 20, 3
    cuts = cuts_of(N, S)
    ref, x, cat = _capped_case(N, k, cuts)
    lab, B = ref["lab"], ref["B"]
    tk, sc, rank, ce, _ = merged(lib, x, lab, N, k, cuts, 128, cat=cat, cap=m)
    single = merged(lib, x, lab, N, k, [], 1024, cat=cat, cap=m)
    plain = merged(lib, x, lab, N, k, cuts, 128)
    ended_early = 0
    for b in range(B):
        want = capped_walk(x[b, :N], cat, k, m)
        assert tk[b].tolist() == want + [-1] * (k - len(want)), (b, tk[b].tolist(), want)
        assert (sc[b, :len(want)].view(np.int32) == x[b, want].view(np.int32)).all() and (sc[b, len(want):] == -7.0).all()
        ended_early += len(want) < k
    assert ended_early == B if m == 1 else ended_early == 0              # 12 categories: m = 1 ends every walk at 12 entries
    for a, b in zip((tk, sc, rank), single[:3]):
        assert a.tobytes() == b.tobytes()
    assert rank.tobytes() == plain[2].tobytes() and ce.tobytes() == plain[3].tobytes()        # the cap leaves rank and ce alone


def test_a_cap_of_k_or_more_is_the_uncapped_merge(lib):
    N, k, S = 1003, 20, 3
    cuts = cuts_of(N, S)
    ref, x, cat = _capped_case(N, k, cuts)
    plain = merged(lib, x, ref["lab"], N, k, cuts, 128)
    for m in (k, 99):
        got = merged(lib, x, ref["lab"], N, k, cuts, 128, cat=cat, cap=m)
        for a, b in zip(got, plain):
            assert a.tobytes() == b.tobytes(), m
