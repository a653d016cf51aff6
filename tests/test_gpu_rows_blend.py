"""tcar_rows_blend on the GPU (include/tcar_warm.h, csrc/warm.hip) against the fp64 statement of the rule (tests/warm_ref.py), with the
bound that follows from its arithmetic — k fmas, a k-term sum and one division in fp32:

    |row[c] - ref[c]| <= (2 k + 2) 2^-24 max_j |x_nj[c]|   over the donors with a weight > 0.

Shapes: U in {1, 5, 9} (one wave of a workgroup, a whole workgroup and a wave, two and a wave), k in {1, 7, 64}; the table N = 300
rows of H = 250 at ld 256 (16-byte loads, the two columns behind the last whole float4 read beside them), H = 7 at ld 8 from a base
that is NOT 16-byte aligned (the scalar path), H = 8 at ld 8 (16-byte loads, no tail) and H = 301 at ld 304 (two passes of 256
columns, the tail in the second).  Every list set holds donor N - 1, empty slots (-1) in the middle of a list, ids outside the table,
negative cosines and cosines below min_sim; with U >= 5 also a list of all -1, one whose cosines are all below min_sim, one of
negative cosines only and one donor repeated k times.  The pad columns of the table and a row that only weightless slots name are
NaN: nothing may read them.  Canary words sit behind row U - 1 of every output and in the pad columns of a scalar-path output."""
import ctypes as C

import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401

import warm_ref
from gpu_util import _need_gpu, lib  # noqa: F401  (lib: the module-scoped fixture)

pytestmark = pytest.mark.gpu

N = 300
MIN_SIM = 0.2
CANARY = -7.5
# (H, ld of the table and of out, base 16-byte aligned)
SHAPES = {"H250-ld256": (250, 256, True), "H7-ld8-unaligned": (7, 8, False), "H8-ld8": (8, 8, True), "H301-ld304": (301, 304, True)}
POISON = N - 2                                   # a table row of NaN: only slots without a weight name it

_TABLES = {}


def _table(H):
    """fp32 [N, H], computed once per H, never written; row POISON is NaN"""
    if H not in _TABLES:
        t = (np.random.RandomState(100 + H).standard_normal((N, H)) * 0.35).astype(np.float32)
        t[POISON] = np.nan
        t.setflags(write=False)
        _TABLES[H] = t
    return _TABLES[H]


def _lists(U, k, seed):
    rng = np.random.RandomState(seed)
    nbr = rng.randint(0, N - 2, (U, k)).astype(np.int32)             # (never POISON, never N - 1: both are planted below)
    sim = rng.uniform(MIN_SIM, 1.0, (U, k)).astype(np.float32)
    nbr[0, 0] = N - 1                                                # the last row of the table
    for u in range(U):
        if k >= 3:
            nbr[u, k // 2] = -1                                      # an empty slot in the middle of a list
            sim[u, k // 2] = np.nan                                  # (the finish leaves its score untouched: it may be anything)
        if k >= 7:
            nbr[u, 1], nbr[u, 3] = N, -5                             # ids outside the table: empty slots, never read
            sim[u, 4] = -0.4                                         # a negative cosine
            sim[u, 5], nbr[u, 5] = MIN_SIM / 2, POISON               # below min_sim: its row is not read
            sim[u, 6] = np.float32(MIN_SIM)                          # equal to min_sim: it donates
    if U >= 5:
        nbr[1] = -1                                                  # all empty
        sim[2] = rng.uniform(0.0, MIN_SIM * 0.99, k)                 # all below min_sim
        nbr[2] = POISON
        sim[3] = -rng.uniform(0.1, 1.0, k)                           # negative cosines only
        nbr[4] = 17                                                  # one donor repeated, in every slot (some of them weightless)
    return nbr, sim


def _on_device(x, ld, aligned, rows_extra=0, fill=np.nan):
    """x [R, H] inside a device matrix [R + rows_extra, ld] of `fill`; not aligned: the matrix starts 4 bytes behind a 16-byte
    boundary -> (the matrix as a view, its storage)"""
    R, H = x.shape
    store = torch.full(((R + rows_extra) * ld + 4,), float(fill), dtype=torch.float32, device="cuda")
    m = store[0 if aligned else 1:][:(R + rows_extra) * ld].view(R + rows_extra, ld)
    assert (m.data_ptr() % 16 == 0) == aligned
    m[:R, :H] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return m, store


def _run(lib, U, k, H, ld, aligned, nbr, sim, min_sim=MIN_SIM):
    table, _keep = _on_device(_table(H), ld, aligned)
    out, _keep2 = _on_device(np.full((U, H), CANARY, np.float32), ld, aligned, rows_extra=2, fill=CANARY)
    support = torch.full((U + 2,), -99, dtype=torch.int32, device="cuda")
    wsum = torch.full((U + 2,), CANARY, dtype=torch.float32, device="cuda")
    n_d, s_d = torch.from_numpy(nbr).cuda(), torch.from_numpy(sim).cuda()
    p = lambda t: C.c_void_p(t.data_ptr())                            # noqa: E731
    rc = lib.tcar_rows_blend(U, k, N, H, p(n_d), p(s_d), min_sim, p(table), ld, p(out), ld, p(support), p(wsum), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu().numpy(), support.cpu().numpy(), wsum.cpu().numpy()


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("k", [1, 7, 64])
@pytest.mark.parametrize("U", [1, 5, 9])
def test_the_blend_against_fp64_within_the_bound_of_its_arithmetic(lib, U, k, shape):
    H, ld, aligned = SHAPES[shape]
    nbr, sim = _lists(U, k, seed=1000 * U + k)
    out, support, wsum = _run(lib, U, k, H, ld, aligned, nbr, sim)
    name = "U=%d k=%d %s" % (U, k, shape)
    _, (ref, ref_support, ref_wsum) = warm_ref.check_rows(out[:U, :H], nbr, sim, _table(H), MIN_SIM, name=name)
    assert not np.isnan(out[:U, :H]).any(), (name, "a NaN of the table was read")
    # support exactly; the sum of the weights within its k - 1 roundings
    assert np.array_equal(support[:U], ref_support), (name, support[:U], ref_support)
    assert (np.abs(wsum[:U].astype(np.float64) - ref_wsum) <= max(k - 1, 0) * warm_ref.EPS * ref_wsum).all(), (name, wsum[:U], ref_wsum)
    # rows without a donor: +0 in every column, support 0, wsum +0
    empty = np.flatnonzero(ref_support == 0)
    for u in empty:
        assert out[u, :H].tobytes() == np.zeros(H, np.float32).tobytes() and wsum[u].tobytes() == np.float32(0).tobytes(), (name, u)
    if U >= 5:
        assert set(empty.tolist()) >= {1, 2, 3} and ref_support[4] >= 1
    # the canaries: rows >= U of out, support and wsum; the pad columns of a scalar-path output stay, those of a vector one are +0
    assert (out[U:] == CANARY).all() and (support[U:] == -99).all() and (wsum[U:] == CANARY).all(), (name, "rows >= U")
    if ld > H:
        pad = out[:U, H:]
        if aligned and H >= 4:
            assert pad.tobytes() == np.zeros_like(pad).tobytes(), (name, "pad columns of a 16-byte output must be +0")
        else:
            assert (pad == CANARY).all(), (name, "pad columns of a scalar output must not be written")


def test_two_runs_give_the_same_bits_and_min_sim_moves_the_lists(lib):
    for shape in ("H250-ld256", "H7-ld8-unaligned"):
        H, ld, aligned = SHAPES[shape]
        nbr, sim = _lists(9, 64, seed=5)
        a, b = _run(lib, 9, 64, H, ld, aligned, nbr, sim), _run(lib, 9, 64, H, ld, aligned, nbr, sim)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes(), shape
        # min_sim = 0 admits the slots below MIN_SIM — but their row is the NaN row: take them out of the lists first
        n0 = np.where(nbr == POISON, 3, nbr)
        low, _, _ = _run(lib, 9, 64, H, ld, aligned, n0, sim, min_sim=0.0)
        warm_ref.check_rows(low[:9, :H], n0, sim, _table(H), 0.0, name="min_sim 0 " + shape)
        assert not np.array_equal(low[0, :H], a[0][0, :H])
        # the result of a row does not depend on the rows beside it: row 5 of U = 9 is the row of U = 1 over the same list
        one, s1, w1 = _run(lib, 1, 64, H, ld, aligned, nbr[5:6].copy(), sim[5:6].copy())
        assert one[0, :H].tobytes() == a[0][5, :H].tobytes() and s1[0] == a[1][5] and w1[0].tobytes() == a[2][5].tobytes()


def test_a_single_donor_gives_its_row_and_a_donor_listed_twice_too(lib):
    """exact cases: with the weight 0.25 the product, the sum and the division are exact, so the row comes back bit for bit; a donor
    listed twice with the weight 0.5 sums to the row itself, over W = 1"""
    H, ld, aligned = SHAPES["H250-ld256"]
    nbr = np.full((2, 7), -1, np.int32)
    sim = np.zeros((2, 7), np.float32)
    nbr[0, 3], sim[0, 3] = N - 1, 0.25
    nbr[1, [1, 5]], sim[1, [1, 5]] = 40, 0.5
    out, support, wsum = _run(lib, 2, 7, H, ld, aligned, nbr, sim)
    t = _table(H)
    assert out[0, :H].tobytes() == t[N - 1].tobytes() and out[1, :H].tobytes() == t[40].tobytes()
    assert support[:2].tolist() == [1, 2] and wsum[:2].tolist() == [0.25, 1.0]
