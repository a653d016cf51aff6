"""tcar_retrieve_merge and tcar_retrieve_panel_live at the op level (include/tcar_retrieve_shard.h), exactly: the columns of one matrix
are cut into S shards at multiples of 128, every shard is folded into its OWN state by tcar_retrieve_panel with its global n0, and
the S states are merged.  The list order is total and the merge copies entries, so the merged list, its score bits and the state
words (entries, `held`, threshold) must be those of ONE fold of the whole matrix and of the numpy model, for every shard order.

x [B = 5, N = 1,000] fp32 (ld 1,024; the padding holds 1e9 and must never be picked), quantised to 16 levels so that ties cross shard
borders.  Row 1 holds NaN, -0.0, +0.0 and -inf entries; row 2 is all-equal.  Filtered runs carry exclusion lists and a window whose
keys are the item ids: row 3 sees [600, 1000) and row 4 [130, 250) alone, so whole shards hold nothing eligible for them."""
import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401

from retrieve_merge_ref import merge_shortlists
from retrieve_ref import shortlist
from gpu_util import lib, ptr  # noqa: F401  (lib: the fixture)

pytestmark = pytest.mark.gpu

B, N, LD, X = 5, 1000, 1024, 6
CS = (1, 7, 64, 200, 1024)
CUTS = {1: [], 2: [512], 3: [256, 640], 7: [128, 256, 384, 512, 640, 768]}
POISON = 0x7f7f7f7f
GAP = 13
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1

_REF = {}


def reference():
    """inputs and the model's shortlists at C = 1,024 (a shortlist of C is their first C columns): computed once, never written"""
    if _REF:
        return _REF
    rng = np.random.RandomState(23)
    x = np.full((B, LD), 1e9, np.float32)
    x[:, :N] = rng.randint(0, 16, (B, N)).astype(np.float32) / 4 - 2
    sp = rng.permutation(N)
    x[1, sp[:9]] = np.nan
    x[1, sp[9:200]] = -0.0
    x[1, sp[200:400]] = 0.0
    x[1, sp[400:406]] = -np.inf
    x[1, sp[406:]] = -np.abs(x[1, sp[406:]]) - 0.25          # the zeros of both signs lead the row: their ties reach every C
    x[2, :N] = 0.5
    key = np.arange(N, dtype=np.int32)
    lo, hi = np.full(B, I32_MIN, np.int64), np.full(B, I32_MAX, np.int64)
    lo[3], hi[3] = 600, 1000
    lo[4], hi[4] = 130, 250
    lo, hi = lo.astype(np.int32), hi.astype(np.int32)
    excl = np.full((B, X), -1, np.int32)
    excl[0, :3] = (N - 1, 511, 512)                          # both sides of a shard border
    excl[2, :4] = (N - 1, N - 2, N - 2, N + 5)               # the winners of the tie row, a repeat, an id past the catalog
    excl[4, :2] = (130, 249)
    plain = shortlist(x[:, :N], 1024)
    full = shortlist(x[:, :N], 1024, excl=excl, key=key, lo=lo, hi=hi)
    assert (full[0][4] >= 0).sum() == 118 and (full[0][3] >= 0).sum() == 400
    _REF.update(x=x, key=key, lo=lo, hi=hi, excl=excl, plain=plain, full=full)
    for v in (x, key, lo, hi, excl) + plain + full:
        v.setflags(write=False)
    return _REF


@pytest.fixture(scope="module")
def dev(lib):
    r = reference()
    return {n: torch.tensor(np.array(r[n])).cuda() for n in ("x", "key", "lo", "hi", "excl")}


def words(Bn, C_):
    return Bn * (2 * C_ + 4)


def fold(lib, dev, C_, state, off, cols, P, filtered, live=None):
    """the columns [cols[0], cols[1]) of x in panels of P into the state at word `off` of `state`"""
    for n0 in range(cols[0], cols[1], P):
        n = min(P, cols[1] - n0)
        f = [ptr(dev["excl"]), X, ptr(dev["key"]), ptr(dev["lo"]), ptr(dev["hi"])] if filtered else [None, 0, None, None, None]
        if live is None:
            rc = lib.tcar_retrieve_panel(B, n0, n, ptr(dev["x"], n0), LD, C_, *f, ptr(state, off), None)
        else:
            rc = lib.tcar_retrieve_panel_live(B, n0, n, ptr(dev["x"], n0), LD, C_, *f, ptr(state, off), ptr(live), None)
        assert rc == 0, (n0, n, rc)


def finish(lib, Bn, C_, state, off=0):
    ids = torch.full((Bn, C_), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((Bn, C_), -7.0, device="cuda")
    assert lib.tcar_retrieve_finish(Bn, C_, ptr(state, off), ptr(ids), ptr(sc), None) == 0
    torch.cuda.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy()


def shard_states(lib, dev, C_, edges, P, filtered, order=None):
    """one state per shard, laid out in `order` with GAP poison words between two shards' rows -> (states, stride)"""
    S = len(edges) - 1
    stride = words(B, C_) + GAP
    states = torch.full((S * stride,), POISON, dtype=torch.int32, device="cuda")
    for slot, s in enumerate(order or range(S)):
        assert lib.tcar_retrieve_reset(B, C_, ptr(states, slot * stride), None) == 0
        fold(lib, dev, C_, states, slot * stride, (edges[s], edges[s + 1]), P, filtered)
    return states, stride


def merge(lib, C_, S, states, stride, Bn=B):
    """-> the merged state [Bn, 2C + 4] as a device tensor with GAP poison words behind it"""
    out = torch.full((words(Bn, C_) + GAP,), POISON, dtype=torch.int32, device="cuda")
    assert lib.tcar_retrieve_merge(Bn, C_, S, ptr(states), stride, ptr(out), None) == 0
    torch.cuda.synchronize()
    assert bool((out[words(Bn, C_):] == POISON).all())
    if S > 1:
        assert bool((states.view(-1, stride)[:, words(Bn, C_):] == POISON).all())
    return out


@pytest.mark.parametrize("C_", CS)
def test_merged_shard_states_are_the_one_fold_of_the_whole_matrix(lib, dev, C_):
    r = reference()
    rw = 2 * C_ + 4
    for filtered in (False, True):
        want_ids, want_sc = (a[:, :C_] for a in r["full" if filtered else "plain"])
        one = torch.full((words(B, C_),), POISON, dtype=torch.int32, device="cuda")
        assert lib.tcar_retrieve_reset(B, C_, ptr(one), None) == 0
        fold(lib, dev, C_, one, 0, (0, N), 1024, filtered)
        torch.cuda.synchronize()
        one = one.cpu().numpy().reshape(B, rw)
        for S, cuts in CUTS.items():
            edges = [0] + cuts + [N]
            for P in (128, 256):
                what = (C_, S, P, filtered)
                states, stride = shard_states(lib, dev, C_, edges, P, filtered)
                out = merge(lib, C_, S, states, stride)
                ids, sc = finish(lib, B, C_, out)
                assert (ids == want_ids).all(), what
                assert sc.tobytes() == want_sc.tobytes(), what
                st = out[:words(B, C_)].cpu().numpy().reshape(B, rw)
                assert st[:, :2 * C_ + 3].tobytes() == one[:, :2 * C_ + 3].tobytes(), what          # entries, held, threshold
                # the numpy merge of the shards' own finished lists
                per = [finish(lib, B, C_, states, s * stride) for s in range(S)]
                mi, ms = merge_shortlists(per, C_)
                assert (mi == want_ids).all() and ms.tobytes() == want_sc.tobytes(), what
            if S == 1:
                continue
            # the shards in another order: the same bits
            perm = list(range(S))[::-1] if S < 7 else [3, 6, 0, 5, 1, 4, 2]
            states2, _ = shard_states(lib, dev, C_, edges, 128, filtered, order=perm)
            out2 = merge(lib, C_, S, states2, stride)
            assert out2[:words(B, C_)].view(B, rw)[:, :2 * C_ + 3].cpu().numpy().tobytes() == st[:, :2 * C_ + 3].tobytes(), what
            # the merged state is a state: shards 0 .. S - 2 merged, the last shard's columns folded into it
            head = merge(lib, C_, S - 1, states, stride)
            fold(lib, dev, C_, head, 0, (edges[-2], edges[-1]), 128, filtered)
            ids3, sc3 = finish(lib, B, C_, head)
            assert (ids3 == want_ids).all() and sc3.tobytes() == want_sc.tobytes(), what
            assert bool((head[words(B, C_):] == POISON).all())


def test_sixty_four_shards_of_one_block_each(lib):
    Bn, Nn, C_, S = 3, 8192, 1024, 64
    rng = np.random.RandomState(3)
    x = (rng.randint(0, 16, (Bn, Nn)).astype(np.float32) / 4 - 2)
    x[1, :] = np.sort(x[1])                                   # ascending: the last shards replace what the first ones gave
    x[2, 4096:] = np.nan                                      # half of the shards hold nothing for session 2
    d = torch.tensor(x).cuda()
    stride = words(Bn, C_) + GAP
    states = torch.full((S * stride,), POISON, dtype=torch.int32, device="cuda")
    for s in range(S):
        assert lib.tcar_retrieve_reset(Bn, C_, ptr(states, s * stride), None) == 0
        assert lib.tcar_retrieve_panel(Bn, 128 * s, 128, ptr(d, 128 * s), Nn, C_, None, 0, None, None, None, ptr(states, s * stride),
                                       None) == 0
    out = merge(lib, C_, S, states, stride, Bn)
    ids, sc = finish(lib, Bn, C_, out)
    want_ids, want_sc = shortlist(x, C_)
    assert (ids == want_ids).all() and sc.tobytes() == want_sc.tobytes()
    assert out[:words(Bn, C_)].view(Bn, -1)[:, 2 * C_].tolist() == [1024, 1024, 1024]


def test_a_session_that_is_not_live_keeps_its_reset_state(lib, dev):
    r = reference()
    live = torch.tensor([0, -1, 0, -1, 0], dtype=torch.int32, device="cuda")
    for C_ in (7, 200):
        rw = 2 * C_ + 4
        a = torch.full((words(B, C_),), POISON, dtype=torch.int32, device="cuda")
        b = a.clone()
        fresh = a.clone()
        for t in (a, b, fresh):
            assert lib.tcar_retrieve_reset(B, C_, ptr(t), None) == 0
        fold(lib, dev, C_, a, 0, (0, N), 256, True)
        fold(lib, dev, C_, b, 0, (0, N), 256, True, live=live)
        torch.cuda.synchronize()
        a, b, fresh = (t.cpu().numpy().reshape(B, rw) for t in (a, b, fresh))
        for s in (0, 2, 4):
            assert b[s].tobytes() == a[s].tobytes(), (C_, s)
        for s in (1, 3):
            assert b[s].tobytes() == fresh[s].tobytes() and a[s].tobytes() != fresh[s].tobytes(), (C_, s)
        ids, _ = finish(lib, B, C_, torch.tensor(b.reshape(-1)).cuda())
        assert (ids[[1, 3]] == -1).all() and (ids[[0, 2, 4]] == r["full"][0][[0, 2, 4], :C_]).all()
