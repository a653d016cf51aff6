"""tcar_mmr_walk at the op level (include/tcar_mmr.h) against the numpy model of tests/mmr_ref.py.

(a) Exact arithmetic: content rows hold exactly four entries of 0.5, drawn from a few short runs of columns, so every norm is exactly 1
    and every cosine is in {0, 1/4, 1/2, 3/4, 1} in ANY summation order; scores are multiples of 1/8 on 16 levels and mu is 0, 0.5 or 2,
    so every value of the walk is exact too, ties are everywhere and every level of the order is reached.  topk, out_score and msim
    must equal walk_f32 byte for byte.
(b) Random content against fp64.  TOL_SIM = (H + 8) 2^-24 bounds the error of one similarity: an fp32 dot of H products of rows whose
    normalised form has |x| |y| <= 1 (H 2^-24 to first order, whatever the order of the sum), the two square roots, the two divisions
    and the two products of the normalisation (8 more roundings of half an ulp of a value <= 1 each — counted whole).  A value
    v = s - mu m then carries mu TOL_SIM from m and at most two roundings, of mu m and of the difference: tau = mu TOL_SIM +
    2^-23 max(max |s|, mu).  Two values whose fp64 forms differ by more than 2 tau cannot swap places in fp32, so every pick of the
    kernel must lie within 2 tau of the best value that was left (in fp64, given the kernel's own prefix), and where every step of
    the fp64 walk was decided by more than 2 tau the lists must be EQUAL.  Derived, not measured.
(c) Argument errors answer TCAR_E_ARG and write nothing."""
import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401

from cand_ref import rank_model
from gpu_util import lib, ptr  # noqa: F401  (lib: the fixture)
from mmr_ref import tau_greedy, walk_f32, walk_f64

pytestmark = pytest.mark.gpu

B = 6
FILL = -77.0


def _exact_content(rng, N, H):
    """[N, H]: four entries of 0.5 per row, on columns of one of a few runs of seven (the last run ends at H - 1: the partial chunk);
    item 0 is all zero"""
    runs = [0] if H < 14 else [0, H // 4, H // 2, H - 7]
    x = np.zeros((N, H), np.float32)
    for n in range(1, N):
        x[n, runs[rng.randint(len(runs))] + rng.choice(min(7, H), 4, replace=False)] = 0.5
    return x


def _exact_case(C, k, H):
    rng = np.random.RandomState(1000 * C + H)
    N = 300
    content = _exact_content(rng, N, H)
    cand = rng.randint(1, N, (B, C)).astype(np.int32)
    score = (rng.randint(0, 16, (B, C)) / 8.0).astype(np.float32)
    cand[1], score[1] = -1, -np.inf                                   # an all-empty row
    few = rng.rand(C) >= (k // 2) / float(C)                          # fewer than k eligible slots
    cand[2, few], score[2, few] = -1, -np.inf
    cand[3] = rng.randint(1, 4, C)                                    # repeated ids: three items
    score[4, rng.randint(C)] = np.nan                                 # one NaN score
    cand[5, rng.randint(C)] = 0                                       # the all-zero content row ...
    score[5, cand[5] == 0] = 2.0                                      # ... at the top of the scores
    cand[0, rng.rand(C) < 0.1] = N + 5                                # ids past the catalog: ineligible
    return content, cand, score


def _padded(x, extra, fill, lead=0):
    """x [R, n] inside a wider device matrix [R, lead + n + extra], `fill` around it -> (matrix, leading dimension)"""
    t = torch.full((x.shape[0], lead + x.shape[1] + extra), fill, dtype=torch.from_numpy(x).dtype)
    t[:, lead:lead + x.shape[1]] = torch.from_numpy(x)
    return t.cuda(), lead + x.shape[1] + extra


def _order(lib, st, ld_s, ct, ld_c, nb, C):
    order = torch.full((nb, C), -9, dtype=torch.int32, device="cuda")
    assert lib.tcar_cand_rank(nb, C, ptr(st), ld_s, ptr(ct), ld_c, None, 0, None, ptr(order), None, None, None) == 0
    torch.cuda.synchronize()
    return order


def _run(lib, nb, C, k, mu, N, H, content, ldc, ct, ld_c, st, ld_s, order, with_msim=True):
    topk = torch.full((nb, k), -77, dtype=torch.int32, device="cuda")
    out = torch.full((nb, k), FILL, dtype=torch.float32, device="cuda")
    msim = torch.full((nb, k), FILL, dtype=torch.float32, device="cuda")
    rc = lib.tcar_mmr_walk(nb, C, k, mu, N, H, content, ldc, ptr(ct), ld_c, ptr(st), ld_s, ptr(order), ptr(topk), ptr(out),
                           ptr(msim) if with_msim else None, None)
    assert rc == 0
    torch.cuda.synchronize()
    return [t.cpu().numpy().copy() for t in (topk, out, msim)]


@pytest.mark.parametrize("H", [250, 7])
@pytest.mark.parametrize("C,k", [(1, 1), (2, 2), (65, 20), (256, 64), (300, 64), (1024, 20)])
def test_exact_inputs_equal_the_fp32_model_byte_for_byte(lib, C, k, H):
    content, cand, score = _exact_case(C, k, H)
    N = content.shape[0]
    # H = 250: the columns sit at offset 8 of rows of 264 floats (16-byte aligned rows: the vector loads); H = 7: at offset 1 of rows of
    # 9 (no alignment: the scalar loads).  NaN around them, a valid id and a winning score behind the lists.
    xt, ldc = _padded(content, 6 if H == 250 else 1, float("nan"), lead=8 if H == 250 else 1)
    xp = ptr(xt, 8 if H == 250 else 1)
    ct, ld_c = _padded(cand, 1, 5)
    st, ld_s = _padded(score, 3, 7.0)
    order = _order(lib, st, ld_s, ct, ld_c, B, C)
    order_h = order.cpu().numpy()
    for mu in (0.0, 0.5, 2.0):
        want = walk_f32(cand, score, order_h, content, mu, k, fill=FILL)
        got = _run(lib, B, C, k, mu, N, H, xp, ldc, ct, ld_c, st, ld_s, order)
        for name, g, w in zip(("topk", "out_score", "msim"), got, want):
            assert g.tobytes() == w.tobytes(), (name, mu, np.argwhere(g != w)[:5], g[g != w][:5], w[g != w][:5])
        again = _run(lib, B, C, k, mu, N, H, xp, ldc, ct, ld_c, st, ld_s, order)
        assert all(a.tobytes() == g.tobytes() for a, g in zip(again, got))
        bare = _run(lib, B, C, k, mu, N, H, xp, ldc, ct, ld_c, st, ld_s, order, with_msim=False)
        assert bare[0].tobytes() == got[0].tobytes() and bare[1].tobytes() == got[1].tobytes() and (bare[2] == FILL).all()
        if mu == 0.0:                                  # the head of the order, NaN and out-of-catalog slots skipped
            for b in range(B):
                head = [s for s in order_h[b] if s >= 0 and 0 <= cand[b, s] < N and not np.isnan(score[b, s])][:k]
                assert got[0][b, :len(head)].tolist() == cand[b, head].tolist()
    assert (got[0][1] == -1).all() and (got[1][1] == FILL).all() and (got[2][1] == FILL).all()          # the all-empty row
    n2 = int((cand[2] >= 0).sum())
    assert n2 < k or C <= 2
    assert (got[0][2, :n2] >= 0).all() and (got[0][2, n2:] == -1).all() and (got[1][2, n2:] == FILL).all()
    assert (got[2][:, 0][got[0][:, 0] >= 0] == 0).all()                                                # the first pick has met nothing


@pytest.mark.parametrize("H", [32, 33, 128, 129, 256, 257, 300])
def test_every_form_of_the_kernel_equals_the_model_at_its_limits(lib, H):
    """H picks the form — 4, 16 or 32 chunks per lane in registers up to H = 32, 128, 256, and above that the form that keeps no row:
    each at its last H and the next at its first, on the exact inputs of (a), aligned rows and rows at an odd offset"""
    C, k, mu = 65, 20, 0.5
    content, cand, score = _exact_case(C, k, H)
    N = content.shape[0]
    ct, ld_c = _padded(cand, 1, 5)
    st, ld_s = _padded(score, 3, 7.0)
    order = _order(lib, st, ld_s, ct, ld_c, B, C)
    want = walk_f32(cand, score, order.cpu().numpy(), content, mu, k, fill=FILL)
    for lead, extra in ((4, (-H) % 4), (1, 2)):
        xt, ldc = _padded(content, extra, float("nan"), lead=lead)
        got = _run(lib, B, C, k, mu, N, H, ptr(xt, lead), ldc, ct, ld_c, st, ld_s, order)
        for name, g, w in zip(("topk", "out_score", "msim"), got, want):
            assert g.tobytes() == w.tobytes(), (name, H, lead, np.argwhere(g != w)[:5])
    assert (want[2] > 0).any() and (want[0][0] >= 0).all()


# ---- (b) random content against fp64
SEED, NB, H_B, N_B = 7, 32, 250, 3000
TOL_SIM = (H_B + 8) * 2.0 ** -24


def _random_case(C):
    rng = np.random.RandomState(SEED)
    centres = rng.standard_normal((12, H_B))
    content = (centres[rng.randint(0, 12, N_B)] + 0.5 * rng.standard_normal((N_B, H_B))).astype(np.float32)
    cand = np.stack([rng.choice(N_B, C, replace=False) for _ in range(NB)]).astype(np.int32)
    score = (2.0 * rng.standard_normal((NB, C))).astype(np.float32)
    return content, cand, score


def _tau(score, mu):
    return mu * TOL_SIM + 2.0 ** -23 * max(float(np.abs(score).max()), mu)


@pytest.mark.parametrize("C,k,mu", [(65, 20, 0.5), (256, 20, 2.0), (256, 64, 8.0)])
def test_random_content_is_tau_greedy_and_equals_fp64_where_it_is_decisive(lib, C, k, mu):
    content, cand, score = _random_case(C)
    order_h = rank_model(score, cand)[1]
    xt, ldc = _padded(content, 2, float("nan"), lead=4)
    ct, ld_c = _padded(cand, 1, 5)
    st, ld_s = _padded(score, 3, 70.0)
    order = _order(lib, st, ld_s, ct, ld_c, NB, C)
    assert (order.cpu().numpy() == order_h).all()
    topk, out, msim = _run(lib, NB, C, k, mu, N_B, H_B, ptr(xt, 4), ldc, ct, ld_c, st, ld_s, order)
    tau = _tau(score, mu)
    short, m64, count = tau_greedy(cand, score, order_h, content, mu, topk)
    assert (count == k).all()
    print("C=%d k=%d mu=%g: tau %.3e, largest shortfall of a pick %.3e, largest msim error %.3e (TOL_SIM %.3e)"
          % (C, k, mu, tau, short.max(), np.abs(msim - m64).max(), TOL_SIM))
    assert (short <= 2 * tau).all(), (short.max(), 2 * tau)
    assert (np.abs(msim.astype(np.float64) - m64) <= TOL_SIM).all()
    slot_of = lambda b, i: int(np.where(cand[b] == i)[0][0])      # noqa: E731
    assert all(out[b, t].tobytes() == score[b, slot_of(b, topk[b, t])].tobytes() for b in range(NB) for t in range(k))
    if k == 20:
        want, _, _, gap = walk_f64(cand, score, order_h, content, mu, k)
        sure = gap > 2 * tau
        print("  sessions left out of the comparison with walk_f64: %d of %d" % (int((~sure).sum()), NB))
        assert (~sure).sum() <= 3
        assert (topk[sure] == want[sure]).all()


def test_argument_errors_write_nothing(lib):
    C, k, N, H = 30, 20, 50, 8
    content = torch.ones(N, H, device="cuda")
    cand = torch.arange(C, dtype=torch.int32, device="cuda").repeat(2, 1).contiguous()
    score = torch.rand(2, C, device="cuda")
    order = torch.arange(C, dtype=torch.int32, device="cuda").repeat(2, 1).contiguous()
    big = 1100
    topk = torch.full((2, 64), -77, dtype=torch.int32, device="cuda")
    out = torch.full((2, 64), FILL, device="cuda")
    msim = torch.full((2, 64), FILL, device="cuda")
    wide_i, wide_f = torch.zeros(2, big, dtype=torch.int32, device="cuda"), torch.zeros(2, big, device="cuda")
    names = ("B", "C", "k", "mu", "N", "H", "content", "ldc", "cand", "ld_cand", "score", "ld_score", "order", "topk", "out", "msim", "stream")
    base = dict(B=2, C=C, k=k, mu=1.0, N=N, H=H, content=ptr(content), ldc=H, cand=ptr(cand), ld_cand=C, score=ptr(score), ld_score=C,
                order=ptr(order), topk=ptr(topk), out=ptr(out), msim=ptr(msim), stream=None)
    walk = lambda **kw: lib.tcar_mmr_walk(*[dict(base, **kw)[a] for a in names])
    wide = dict(cand=ptr(wide_i), score=ptr(wide_f), order=ptr(wide_i), ld_cand=big, ld_score=big)
    for bad in (dict(C=0), dict(C=1025, **wide), dict(k=0), dict(k=65, C=100, **wide), dict(k=31), dict(mu=-1.0), dict(mu=float("nan")),
                dict(mu=float("inf")), dict(order=None), dict(topk=None)):
        assert walk(**bad) == -1, bad
    torch.cuda.synchronize()
    assert (topk.cpu().numpy() == -77).all() and (out.cpu().numpy() == FILL).all() and (msim.cpu().numpy() == FILL).all()
    assert walk() == 0
    torch.cuda.synchronize()
    assert (topk.flatten()[:2 * k].cpu().numpy() >= 0).all()           # ([B, k] with the stride k): the accepted call does write
