"""tcar_dup_rnorm / tcar_dup_reset / tcar_dup_tiles / tcar_dup_finish at the op level (include/tcar_dupes.h).

The reference is existing code: S [N, N] comes from tcar_sim_queries(qid = arange(N)) and ONE tcar_sim_panel over the same table, and
tests/dupes_ref.audit_from_sims turns it into (count, partner, sim) by a loop over the definition.  The audit's three arrays must
equal that byte for byte: the kernels share one K loop (csrc/sim_tile.h), every reduction of the audit is an integer one.

  shapes      (N, H): N one below, at and one above the 64-row block, one row, two and five blocks; H below one load (1), below one
              step of eight (7), one step (8), one column into the second K chunk (33), the issue's 250 (a partial last chunk); and a
              table at column 1 of rows of an odd length, which takes the scalar loads.
  plants      verbatim copies across block edges, a clique of three equal rows (the tie goes to the larger id), a copy scaled by
              0.5, near copies (noise 1e-3), an all-zero row, a row with a NaN and one with an Inf.
  thresholds  0.9; 1.0; the exact fp32 similarity of a near-copy pair (the pair counts) and the next float above it (it does not).
  partition   stripes of 1 block, of 2 blocks and all blocks in one call give equal bytes; so does a second run.
Every output is allocated with sentinels behind N, which must survive."""
import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401

from dupes_ref import audit_from_sims
from gpu_util import lib, ptr  # noqa: F401  (lib: the fixture)
from similar_case import exact_content, padded
from similar_ref import sims_f32

pytestmark = pytest.mark.gpu

PAD = 8
SENT_I, SENT_F, SENT_B = -77, -77.0, -7


def _table(content, aligned=True):
    """the [N, H] table inside a wider device matrix, NaN around it: at column 4 of rows that are a multiple of four floats long
    (the 16-byte loads), or at column 1 of rows of an odd length (the scalar loads) -> (tensor, offset, ld)"""
    H = content.shape[1]
    lead, extra = (4, (-H) % 4) if aligned else (1, 3 if H % 2 else 2)
    t, ld = padded(content, extra, float("nan"), lead=lead)
    assert aligned or ld % 2 == 1
    return t, lead, ld


def _sims(lib, table, N, H):
    """S [N, N] and the rq [N] of the prologue: tcar_sim_queries(qid = arange(N)), then ONE tcar_sim_panel"""
    t, lead, ldc = table
    ldx, ld = (H + 3) // 4 * 4 + 4, (N + 3) // 4 * 4
    qid = torch.arange(N, dtype=torch.int32, device="cuda")
    xq, rq = torch.full((N, ldx), float("nan"), device="cuda"), torch.full((N,), float("nan"), device="cuda")
    out = torch.full((N, ld), float("nan"), device="cuda")
    assert lib.tcar_sim_queries(N, N, H, ptr(t, lead), ldc, ptr(qid), None, 0, ptr(xq), ldx, ptr(rq), None) == 0
    assert lib.tcar_sim_panel(N, 0, N, H, ptr(t, lead), ldc, ptr(xq), ldx, ptr(rq), ptr(out), ld, None) == 0
    torch.cuda.synchronize()
    return np.ascontiguousarray(out.cpu().numpy()[:, :N]), rq.cpu().numpy()


def _audit(lib, table, N, H, t, stripe=None, key=None, lo=0, hi=0):
    """rnorm, reset, the tiles in stripes of `stripe` row blocks (None: one call), finish -> (count, partner, sim, r) as numpy; the
    sentinels behind N are checked here"""
    tb, lead, ldc = table
    r = torch.full((N + PAD,), SENT_F, device="cuda")
    count = torch.full((N + PAD,), SENT_I, dtype=torch.int32, device="cuda")
    best = torch.full((N + PAD,), SENT_B, dtype=torch.int64, device="cuda")
    partner = torch.full((N + PAD,), SENT_I, dtype=torch.int32, device="cuda")
    psim = torch.full((N + PAD,), SENT_F, device="cuda")
    kd = torch.from_numpy(np.asarray(key, np.int32)).cuda() if key is not None else None
    nb = (N + 63) // 64
    stripe = nb if stripe is None else stripe
    assert lib.tcar_dup_rnorm(N, H, ptr(tb, lead), ldc, ptr(r), None) == 0
    assert lib.tcar_dup_reset(N, ptr(count), ptr(best), None) == 0
    for b0 in range(0, nb, stripe):
        assert lib.tcar_dup_tiles(N, H, ptr(tb, lead), ldc, ptr(r), b0, min(b0 + stripe, nb), float(t), ptr(kd) if kd is not None else None,
                                  lo, hi, ptr(count), ptr(best), None) == 0
    assert lib.tcar_dup_finish(N, ptr(best), ptr(partner), ptr(psim), None) == 0
    torch.cuda.synchronize()
    out = [x.cpu().numpy() for x in (count, partner, psim, r, best)]
    for x, s in zip(out, (SENT_I, SENT_I, SENT_F, SENT_F, SENT_B)):
        assert (x[N:] == s).all() and len(x) == N + PAD
    return tuple(x[:N].copy() for x in out[:4])


def _same(got, want, what):
    for name, x, y in zip(("count", "partner", "sim"), got, want):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, name, np.flatnonzero(x != y)[:8], x[x != y][:8], y[x != y][:8])


NEAR = (12, 13)                         # the near-copy pair whose similarity is a threshold


def _planted(N, H):
    """random normal rows with the plants of the module docstring, as far as N has room for them"""
    rng = np.random.RandomState(1000 * N + H)
    x = rng.standard_normal((N, H)).astype(np.float32)
    if N >= 63:
        x[7] = 0.5 * x[8]                                                   # a scaled copy
        for a, b in (NEAR, (40, 41)):
            x[a] = x[b] + np.float32(1e-3) * rng.standard_normal(H).astype(np.float32)
        x[5] = x[N // 2 + 5] = x[N - 3]                                     # a clique of three
        x[15] = 0.0
        x[17, H // 2], x[19, H - 1] = np.nan, np.inf
    if N > 64:
        x[63] = x[64]
    if N > 67:
        x[3] = x[67]
    if N >= 2:
        x[0] = x[N - 1]
    return x


CASES = [(1, 8, True), (2, 1, True), (63, 7, True), (64, 8, True), (65, 33, True), (129, 250, True), (321, 250, True), (200, 31, False)]


@pytest.mark.parametrize("N,H,aligned", CASES)
def test_the_audit_equals_the_model_on_one_panel_call_s_block(lib, N, H, aligned):
    content = _planted(N, H)
    table = _table(content, aligned)
    S, rq = _sims(lib, table, N, H)
    nan = np.isnan(S)
    assert (nan == nan.T).all() and S[~nan].tobytes() == S.T[~nan.T].tobytes()              # sim(i, j) == sim(j, i), bit for bit
    thresholds = [0.9, 1.0]
    if N >= 63:
        exact = S[NEAR]
        assert 0.9 < exact < 1.0
        thresholds += [exact, np.nextafter(exact, np.float32(2))]
    nb = (N + 63) // 64
    seen = {}
    for t in thresholds:
        want = audit_from_sims(S, t)
        got = _audit(lib, table, N, H, t)
        _same(got[:3], want, (N, H, float(t)))
        assert got[3].tobytes() == rq.tobytes()                                               # tcar_dup_rnorm against the prologue
        seen[float(t)] = got
        for stripe in [s for s in (1, 2) if s < nb] if t == 0.9 else []:
            _same(_audit(lib, table, N, H, t, stripe=stripe)[:3], want, (N, H, "stripe", stripe))
    _same(_audit(lib, table, N, H, 0.9)[:3], seen[0.9][:3], "a second run")
    count, partner, sim = seen[0.9][:3]
    if N >= 2:
        assert count[0] >= 1 and count[N - 1] >= 1 and partner[0] == N - 1                    # the verbatim pair (0, N - 1)
    if N == 1:
        assert count.tolist() == [0] and partner.tolist() == [-1] and sim.tolist() == [0.0]
    if N >= 63:
        # the zero row and the rows with a NaN or an Inf are never flagged and nobody's partner
        for n in (15, 17, 19):
            assert count[n] == 0 and partner[n] == -1 and sim[n] == 0 and not np.signbit(sim[n]) and not (partner == n).any()
        a, b, c = 5, N // 2 + 5, N - 3                                                          # the clique: the tie goes to the larger id
        assert partner[a] == c and partner[b] == c and partner[c] == b and min(count[a], count[b], count[c]) >= 2
        assert count[7] >= 1 and count[8] >= 1                                                # the scaled copy is seen
        # the near copy counts at its own similarity and not one float above it
        at, above = seen[float(thresholds[2])], seen[float(thresholds[3])]
        assert at[0][NEAR[0]] == above[0][NEAR[0]] + 1 and at[0][NEAR[1]] == above[0][NEAR[1]] + 1
    if N > 67:
        assert count[3] >= 1 and count[67] >= 1 and count[63] >= 1 and count[64] >= 1         # copies across block edges


def test_a_dense_catalog_flushes_every_row_of_every_tile(lib):
    N, H = 130, 8
    content = np.tile(np.random.RandomState(2).standard_normal((1, H)).astype(np.float32), (N, 1))
    table = _table(content)
    want = (np.full(N, N - 1, np.int32), np.full(N, N - 1, np.int32))
    want[1][N - 1] = N - 2
    for stripe in (None, 1):
        count, partner, sim, _ = _audit(lib, table, N, H, 0.9, stripe=stripe)
        assert (count == want[0]).all() and (partner == want[1]).all(), (count, partner)
        assert len(set(sim.tolist())) == 1 and abs(float(sim[0]) - 1.0) <= 16 * 2.0 ** -24


def test_a_window_audits_its_members_against_each_other(lib):
    N, H = 321, 250
    content = _planted(N, H)
    table = _table(content)
    S, _ = _sims(lib, table, N, H)
    rng = np.random.RandomState(6)
    key = rng.randint(0, 100, N).astype(np.int32)
    key[[0, N - 1, 3, 67, 63]] = 50                                                           # planted pairs inside the window, one of (63, 64) outside
    key[64] = 99
    key[128:192] = 1000                                                                       # a row block without a member: its tiles are skipped
    lo, hi = 25, 75
    member = (key >= lo) & (key < hi)
    assert 100 < member.sum() < 220 and not member[128:192].any()
    plain = audit_from_sims(S, 0.9)
    for stripe in (None, 1):
        got = _audit(lib, table, N, H, 0.9, stripe=stripe, key=key, lo=lo, hi=hi)
        want = audit_from_sims(S, 0.9, member)
        _same(got[:3], want, ("window", stripe))
    assert got[0][0] >= 1 and got[0][63] == 0 and plain[0][63] >= 1 and not got[0][~member].any()
    # an empty window is no error: nothing is a member
    for lo, hi in ((60, 60), (75, 25)):
        count, partner, sim, _ = _audit(lib, table, N, H, 0.9, key=key, lo=lo, hi=hi)
        assert not count.any() and (partner == -1).all() and not sim.any() and not np.signbit(sim).any()


@pytest.mark.parametrize("H", [8, 33, 250])
def test_exact_inputs_equal_the_fp32_model_byte_for_byte(lib, H):
    """similar_case.exact_content: every product and partial sum is exact, so fused and unfused multiply-adds agree and the numpy
    model of similar_ref gives the kernel's bits"""
    N = 200
    rng = np.random.RandomState(77 + H)
    content = exact_content(rng, N, H)
    S = sims_f32(content, content)
    assert set(np.unique(S).tolist()) <= {0.0, 0.25, 0.5, 0.75, 1.0}
    table = _table(content, aligned=H != 33)
    for t in (0.5, 0.75, 1.0):
        want = audit_from_sims(S, t)
        assert want[0].max() >= 2 and want[0][0] == 0
        _same(_audit(lib, table, N, H, t, stripe=2)[:3], want, (H, t))


def test_argument_errors_write_nothing(lib):
    N, H = 130, 8
    table = _table(_planted(N, H))
    tb, lead, ldc = table
    count = torch.full((N,), SENT_I, dtype=torch.int32, device="cuda")
    best = torch.full((N,), SENT_B, dtype=torch.int64, device="cuda")
    r = torch.full((N,), SENT_F, device="cuda")
    call = lambda b0=0, b1=3, t=0.9, lo=0, hi=0, n=N: lib.tcar_dup_tiles(n, H, ptr(tb, lead), ldc, ptr(r), b0, b1, t, None, lo, hi,   # noqa: E731
                                                                         ptr(count), ptr(best), None)
    for bad in (dict(b0=-1), dict(b1=4), dict(b0=2, b1=1), dict(t=0.0), dict(t=float("nan")), dict(t=1.5), dict(lo=1, hi=9), dict(n=0)):
        assert call(**bad) == -1, bad
    assert call(b0=2, b1=2) == 0
    torch.cuda.synchronize()
    assert (count.cpu().numpy() == SENT_I).all() and (best.cpu().numpy() == SENT_B).all()
