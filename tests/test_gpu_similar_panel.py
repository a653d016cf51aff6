"""tcar_sim_queries / tcar_sim_panel at the op level (include/tcar_similar.h) against the numpy model of tests/similar_ref.py.

The kernel's tile edges, each met one below, at and one above in (a):
  Q   64 query rows per workgroup                                   -> Q in {63, 64, 65}
  n   64 items per workgroup; 16 per store instruction of a wave     -> n in {15, 16, 17, 63, 64, 65, 127, 128, 129}
  H   4 columns per load, 8 per step (one per chain), 32 per K chunk -> H in {3, 4, 5, 7, 8, 9, 31, 32, 33}, and 250 / 257 of the issue
(a) Exact arithmetic: the rows of test_gpu_mmr_walk.py (similar_case.exact_content: four entries of 0.5; item 0 all zero), so every cosine is in
    {0, 1/4, 1/2, 3/4, 1} in ANY summation order and the whole [Q, n] block must equal sims_f32 byte for byte; content at an aligned
    offset and at an odd one with NaN around it; panels that start inside the table and end inside it or at its last row, with rows
    outside [n0, n0 + n) turned to NaN for the panel call (they are not read); a sentinel behind column n; every case twice.
(b) Random content: the bits of tcar_mmr_walk's msim for the same pair, symmetry, and id queries against the same rows as vectors.
(c) Random content against fp64: |sim - cosine| <= TOL_SIM = (H + 8) 2^-24 for every element — the bound test_gpu_mmr_walk.py derives
    (H roundings of a dot of rows with |x^| |y^| <= 1, eight for the normalisation).  Derived, not measured."""
import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401

from gpu_util import lib, ptr  # noqa: F401  (lib: the fixture)
from similar_case import exact_content, padded
from similar_ref import query_rows, rnorm_f32, sims_f32, sims_f64, tol_sim

pytestmark = pytest.mark.gpu

SENT = -77.0


def _table(content, aligned):
    """the [N, H] table inside a wider device matrix, NaN around it: at column 8 (H = 250: rows of 264) or 4 of rows that are a
    multiple of four floats long (the 16-byte loads), or at column 1 of rows of H + 3 (the scalar loads) -> (tensor, offset, ld)"""
    H = content.shape[1]
    lead = (8 if H == 250 else 4) if aligned else 1
    extra = (6 if H == 250 else (-H) % 4) if aligned else 2
    t, ld = padded(content, extra, float("nan"), lead=lead)
    return t, lead, ld


def _queries(lib, Q, N, H, table, qid=None, qrow=None):
    """tcar_sim_queries -> (xq [Q, ldx] device, rq [Q] device, ldx); xq is NaN behind column H"""
    ldx = (H + 3) // 4 * 4 + 4
    xq = torch.full((Q, ldx), float("nan"), device="cuda")
    rq = torch.full((Q,), float("nan"), device="cuda")
    t, lead, ld = table if table is not None else (None, 0, H)
    rc = lib.tcar_sim_queries(Q, N, H, ptr(t, lead) if t is not None else None, ld, ptr(qid) if qid is not None else None,
                              ptr(qrow) if qrow is not None else None, qrow.shape[1] if qrow is not None else 0, ptr(xq), ldx, ptr(rq),
                              None)
    assert rc == 0
    return xq, rq, ldx


def _panel(lib, Q, n0, n, H, table, xq, rq, ldx, ld=None):
    """tcar_sim_panel into a [Q, ld] buffer of sentinels -> the whole buffer as numpy"""
    ld = (n + 3) // 4 * 4 + 4 if ld is None else ld
    out = torch.full((Q, ld), SENT, device="cuda")
    t, lead, ldc = table
    assert lib.tcar_sim_panel(Q, n0, n, H, ptr(t, lead), ldc, ptr(xq), ldx, ptr(rq), ptr(out), ld, None) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy()


N_A = 300


def _content_a(rng, H):
    """exact_content; below four columns, where it has no room for its four entries, one entry of +-2^e per row instead (item 0 all
    zero as there): every norm is a power of two and every cosine is in {-1, 0, 1}, again in any order"""
    if H >= 4:
        return exact_content(rng, N_A, H)
    x = np.zeros((N_A, H), np.float32)
    x[np.arange(1, N_A), rng.randint(0, H, N_A - 1)] = rng.choice([0.5, 1.0, 2.0, -1.0], N_A - 1)
    return x


# (H, aligned, Q, n0, n): every listed value of every parameter at least once; n = N_A - n0 ends at the table's last row
CASES_A = [(250, True, 1, 0, 300), (250, False, 3, 1, 299), (250, True, 65, 37, 263), (250, True, 64, 37, 65), (250, False, 63, 0, 129),
           (7, False, 3, 1, 64), (7, True, 65, 0, 63), (8, True, 3, 37, 128), (8, False, 1, 1, 17), (9, False, 65, 0, 127),
           (9, True, 3, 37, 16), (257, True, 3, 0, 15), (257, False, 65, 37, 263), (3, False, 3, 0, 65), (4, True, 3, 1, 64),
           (5, False, 1, 37, 63), (31, False, 3, 0, 129), (32, True, 64, 1, 299), (33, True, 3, 37, 17), (33, False, 63, 0, 300)]


@pytest.mark.parametrize("H,aligned,Q,n0,n", CASES_A)
def test_exact_inputs_equal_the_fp32_model_byte_for_byte(lib, H, aligned, Q, n0, n):
    rng = np.random.RandomState(10000 * H + 100 * Q + n0)
    content = _content_a(rng, H)
    ids = rng.randint(1, N_A, Q).astype(np.int32)
    if Q >= 3:
        ids[0], ids[1] = 0, -1                             # the all-zero row and the empty query
    ids[Q - 1] = n0 + n - 1                                # a query inside the panel: a cosine of exactly 1
    table = _table(content, aligned)
    xq, rq, ldx = _queries(lib, Q, N_A, H, table, qid=torch.from_numpy(ids).cuda())
    torch.cuda.synchronize()
    rows = query_rows(content, ids)
    xq_h = xq.cpu().numpy()
    assert xq_h[:, :H].tobytes() == rows.tobytes() and np.isnan(xq_h[:, H:]).all()
    assert rq.cpu().numpy().tobytes() == rnorm_f32(rows).tobytes()
    # the panel reads rows n0 .. n0 + n - 1 alone: the others are NaN for this call
    holed = np.full_like(content, np.nan)
    holed[n0:n0 + n] = content[n0:n0 + n]
    htable = _table(holed, aligned)
    want = sims_f32(rows, content[n0:n0 + n])
    assert set(np.unique(want).tolist()) <= ({0.0, 0.25, 0.5, 0.75, 1.0} if H >= 4 else {-1.0, 0.0, 1.0}) and (want == 1.0).any()
    got = _panel(lib, Q, n0, n, H, htable, xq, rq, ldx)
    assert got[:, :n].tobytes() == want.tobytes(), (np.argwhere(got[:, :n] != want)[:5], got[:, :n][got[:, :n] != want][:5])
    assert (got[:, n:] == SENT).all() and got.shape[1] > n                 # the sentinel behind column n survives
    if Q >= 3:
        assert not got[:2, :n].any() and not np.signbit(got[:2, :n]).any()  # +0 against everything
    again = _panel(lib, Q, n0, n, H, htable, xq, rq, ldx)
    assert again.tobytes() == got.tobytes()


# ---- (b), (c): random content
SEED, N_B, H_B = 11, 3000, 250
Q0, NQ, I0, NI = 200, 32, 1000, 64                         # the queries are the rows 200 .. 231, the items the rows 1000 .. 1063
TOL_SIM = tol_sim(H_B)
_RANDOM = {}


def _random():
    """normal rows around twelve centres, as test_gpu_mmr_walk.py draws them: computed once, shared, never written"""
    if not _RANDOM:
        rng = np.random.RandomState(SEED)
        centres = rng.standard_normal((12, H_B))
        content = (centres[rng.randint(0, 12, N_B)] + 0.5 * rng.standard_normal((N_B, H_B))).astype(np.float32)
        _RANDOM.update(content=content, table=_table(content, True))
    return _RANDOM["content"], _RANDOM["table"]


def _block(lib, table, q0, nq, n0, n):
    qid = torch.arange(q0, q0 + nq, dtype=torch.int32, device="cuda")
    xq, rq, ldx = _queries(lib, nq, N_B, H_B, table, qid=qid)
    return _panel(lib, nq, n0, n, H_B, table, xq, rq, ldx)[:, :n]


def test_random_content_has_the_bits_of_the_mmr_kernel(lib):
    content, table = _random()
    t, lead, ldc = table
    got = _block(lib, table, Q0, NQ, I0, NI)
    # one walk per pair: the shortlist (q, n) with scores (1, 0), k = 2, mu = 1 -> msim[1] = max(0, sim(n, q))
    B = NQ * NI
    cand = np.stack([np.repeat(np.arange(Q0, Q0 + NQ), NI), np.tile(np.arange(I0, I0 + NI), NQ)], 1).astype(np.int32)
    score = np.tile(np.asarray([1.0, 0.0], np.float32), (B, 1))
    ct, st = torch.from_numpy(cand).cuda(), torch.from_numpy(score).cuda()
    order = torch.full((B, 2), -9, dtype=torch.int32, device="cuda")
    assert lib.tcar_cand_rank(B, 2, ptr(st), 2, ptr(ct), 2, None, 0, None, ptr(order), None, None, None) == 0
    topk = torch.full((B, 2), -77, dtype=torch.int32, device="cuda")
    msim = torch.full((B, 2), SENT, device="cuda")
    assert lib.tcar_mmr_walk(B, 2, 2, 1.0, N_B, H_B, ptr(t, lead), ldc, ptr(ct), 2, ptr(st), 2, ptr(order), ptr(topk), None, ptr(msim),
                             None) == 0
    torch.cuda.synchronize()
    assert (topk.cpu().numpy() == cand).all()
    m = msim.cpu().numpy()[:, 1].reshape(NQ, NI)
    pos = m > 0
    assert pos.sum() > B // 8 and (~pos).sum() > B // 8                     # both branches are met
    assert got[pos].tobytes() == m[pos].tobytes(), int((got[pos] != m[pos]).sum())
    assert (got[~pos] <= 0).all()
    # symmetry: the items as queries against the queries as items
    back = _block(lib, table, I0, NI, Q0, NQ)
    assert back.T.tobytes() == got.tobytes()
    # the same rows given as vectors (rows of 250 floats: no 16-byte alignment)
    qrow = torch.from_numpy(np.ascontiguousarray(content[Q0:Q0 + NQ])).cuda()
    xq, rq, ldx = _queries(lib, NQ, N_B, H_B, None, qrow=qrow)
    drafts = _panel(lib, NQ, I0, NI, H_B, table, xq, rq, ldx)[:, :NI]
    assert drafts.tobytes() == got.tobytes()


def test_random_content_against_fp64(lib):
    content, table = _random()
    want = sims_f64(content[Q0:Q0 + NQ], content)
    got = _block(lib, table, Q0, NQ, 0, N_B)
    err = np.abs(got.astype(np.float64) - want)
    print("largest error of a similarity %.3e (TOL_SIM %.3e), %d x %d" % (err.max(), TOL_SIM, NQ, N_B))
    assert (err <= TOL_SIM).all(), (err.max(), TOL_SIM)
    assert np.abs(got[np.arange(NQ), Q0 + np.arange(NQ)] - 1.0).max() <= TOL_SIM


def test_argument_errors_write_nothing_and_empty_calls_launch_nothing(lib):
    content, table = _random()
    t, lead, ldc = table
    xq, rq, ldx = _queries(lib, 4, N_B, H_B, table, qid=torch.arange(4, dtype=torch.int32, device="cuda"))
    out = torch.full((4, 72), SENT, device="cuda")
    call = lambda Q=4, n0=0, n=64, H=H_B, ld=72, o=0: lib.tcar_sim_panel(Q, n0, n, H, ptr(t, lead), ldc, ptr(xq), ldx, ptr(rq),  # noqa: E731
                                                                          ptr(out, o), ld, None)
    for bad in (dict(n=73), dict(ld=70, n=64), dict(n=49153, ld=49156), dict(H=0), dict(n0=-1), dict(Q=-1), dict(o=1)):
        assert call(**bad) == -1, bad
    assert call(Q=0) == 0 and call(n=0) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENT).all()
    assert call() == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:, 64:] == SENT).all() and (np.abs(got[:, :64]) <= 1 + TOL_SIM).all()
