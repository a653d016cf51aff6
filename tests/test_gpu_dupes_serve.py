"""The duplicate audit through the engine (TcarEngine.find_duplicates, Seq2SeqAttNN.duplicate_articles, main.py --audit_duplicates;
tcar_dupes_step) on the N = 700, H = 250 setup of tests/serve_case.py.

What is compared with what:
  top-1       similar_items(arange(N), k=1) — existing code, the panels under the fold — lists every row's best partner: where its
              cosine is >= t the audit's partner and sim are those bytes, elsewhere -1 / 0.  count comes from the [N, N] block of ONE
              tcar_sim_panel call (test_gpu_similar_serve.py's _block, restated: a test file is nobody's library) through
              dupes_ref.audit_from_sims.  The fixture's content is random: its largest cosine is about 0.28, so the thresholds here
              are 0.15 (most rows flagged) and 0.22 (few).
  updates     copies planted through update_items(content=...) on a live engine are what the next audit flags, and its bytes are those
              of an engine built from the final table.
  window      the members of a window, against the model restricted to them.
  partition   stripe = 1 and the default stripe: equal bytes.
  fp64        similar_case.planted(): N = 3,000, 32 queries with 24 planted neighbours each at cosines 0.95 - 0.02 j, through
              tcar_dupes_step on a plain table.  Checked here in fp64 before anything is compared: at t = 0.9 there are 97 pairs on
              128 flagged rows and the cosine nearest to t is 4.0e-4 away; at t = 0.8, 538 pairs on 288 rows, the nearest 1.2e-4 away;
              TOL_SIM = (H + 8) 2^-24 = 1.54e-5 bounds one similarity (tests/test_gpu_mmr_walk.py derives it) and the smallest gap
              between the best and the second-best partner of a flagged row is 0.016 — so count and partner must EQUAL the fp64
              audit for every row, and sim lies within TOL_SIM of it.  No row is left out."""
import ctypes as C
import io
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401

from dupes_ref import audit_f64, audit_from_sims
from gpu_util import _need_gpu, _np, ptr
from serve_case import H, N, reference
from similar_case import P_H, P_N, planted
from similar_ref import sims_f64, tol_sim

pytestmark = pytest.mark.gpu

_ENG = {}


def _engine(content=None):
    from tcar_amd.engine import TcarEngine
    r = reference()
    return TcarEngine(r["params"], r["content"] if content is None else content, r["mw"], max_grad=2.0, scoring="bf16x3-mixed")


def _shared():
    """one engine for the tests that only read it, with item keys installed, and the [N, N] block of its content"""
    if not _ENG:
        eng = _engine()
        keys = np.random.RandomState(31).permutation(N).astype(np.int32)
        eng.set_item_keys(keys)
        _ENG.update(eng=eng, keys=keys, S=_block(eng))
    return _ENG


def _block(eng):
    """the [N, N] similarities of the catalog rows from one tcar_sim_queries and ONE tcar_sim_panel over E's content columns"""
    g, lib = eng.geo, eng.lib
    qid = torch.arange(N, dtype=torch.int32, device="cuda")
    xq, rq = torch.zeros(N, g.ldh, device="cuda"), torch.zeros(N, device="cuda")
    out = torch.full((N, N), float("nan"), device="cuda")
    cp = C.c_void_p(eng.E.data_ptr() + 4 * g.ldh)
    torch.cuda.synchronize()
    assert lib.tcar_sim_queries(N, g.N, g.H, cp, g.ek, ptr(qid), None, 0, ptr(xq), g.ldh, ptr(rq), None) == 0
    assert lib.tcar_sim_panel(N, 0, g.N, g.H, cp, g.ek, ptr(xq), g.ldh, ptr(rq), ptr(out), N, None) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _same(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, i, np.flatnonzero(x != y)[:5])


def test_the_audit_lists_the_top_1_of_similar_items_where_it_reaches_the_threshold():
    _need_gpu()
    s = _shared()
    eng, S = s["eng"], s["S"]
    top, sims = _np(*eng.similar_items(np.arange(N), k=1))
    top, sims = top[:, 0], sims[:, 0]
    assert (top >= 0).all() and 0.2 < sims.max() < 0.4
    for t in (0.15, 0.22):
        audit = eng.find_duplicates(t)
        assert isinstance(audit, tuple) and [x.dtype for x in audit] == [torch.int32, torch.int32, torch.float32]
        assert all(x.shape == (N,) and x.is_cuda for x in audit) and audit.count is audit[0] and audit.sim is audit[2]
        count, partner, sim = _np(*audit)
        hit = sims >= np.float32(t)
        assert 5 < hit.sum() < N
        assert (partner[hit] == top[hit]).all() and sim[hit].tobytes() == sims[hit].tobytes()
        assert (partner[~hit] == -1).all() and not sim[~hit].any() and not np.signbit(sim).any() and ((count > 0) == hit).all()
        want = audit_from_sims(S, t)
        _same((count, partner, sim), want, ("against the block", t))
        assert int(count.sum()) % 2 == 0
    _same(_np(*eng.find_duplicates(0.15, stripe=1)), audit_from_sims(S, 0.15), "stripe 1")
    _same(_np(*eng.find_duplicates(0.15, stripe=4)), _np(*eng.find_duplicates(0.15)), "stripe 4 against the default")
    _same(_np(*eng.find_duplicates(np.float32(0.15))), _np(*eng.find_duplicates(0.15)), "a second run")


def test_a_window_audits_its_members():
    _need_gpu()
    s = _shared()
    eng, S, keys = s["eng"], s["S"], s["keys"]
    for lo, hi in ((100, 450), (0, N), (np.int64(690), 2 ** 40)):
        member = (keys >= lo) & (keys < hi)
        got = _np(*eng.find_duplicates(0.15, window=(lo, hi)))
        _same(got, audit_from_sims(S, 0.15, member), ("window", lo, hi))
        assert not got[0][~member].any()
    _same(_np(*eng.find_duplicates(0.15, window=(100, 450), stripe=1)), audit_from_sims(S, 0.15, (keys >= 100) & (keys < 450)), "stripe 1")
    count, partner, sim = _np(*eng.find_duplicates(0.15, window=(300, 300)))
    assert not count.any() and (partner == -1).all() and not sim.any()


def test_the_request_is_validated():
    _need_gpu()
    from tcar_amd import _lib
    eng = _shared()["eng"]
    for kw, text in ((dict(threshold=0), "threshold must be"), (dict(threshold=1.5), "threshold must be"),
                     (dict(threshold=True), "threshold must be"), (dict(threshold=float("nan")), "threshold must be"),
                     (dict(stripe=0), "stripe must be"), (dict(stripe=2.5), "stripe must be"), (dict(window=(1, 2, 3)), "window = "),
                     (dict(window=(np.zeros(2, np.int32), np.ones(2, np.int32))), "window = ")):
        with pytest.raises(ValueError, match=text):
            eng.find_duplicates(**kw)
    fresh = _engine()
    with pytest.raises(ValueError, match="call set_item_keys"):
        fresh.find_duplicates(0.9, window=(0, 5))
    fresh.shard = (0, N // 2)                       # an engine that holds a shard refuses, as similar_items does
    with pytest.raises(_lib.TcarError, match="whole catalog"):
        fresh.find_duplicates(0.9)
    from tcar_amd.sharded import ShardedEngine
    with pytest.raises(_lib.TcarError, match="whole catalog"):
        ShardedEngine.__new__(ShardedEngine).find_duplicates(0.9)


def test_copies_published_into_a_live_engine_are_what_the_next_audit_flags():
    _need_gpu()
    r = reference()
    eng, rng = _engine(), np.random.RandomState(8)
    count, partner, _ = _np(*eng.find_duplicates(0.98))
    assert not count.any() and (partner == -1).all()                                     # random content: nothing to flag
    src = np.asarray([17, 17, 403, 650])                                                 # 17 is copied twice: a clique of three
    dst = np.asarray([100, 699, 64, 63])
    rows = r["content"][1 + src].copy()
    rows[3] = rows[3] * 2 + np.float32(1e-3) * rng.standard_normal(H).astype(np.float32)  # scaled, with a little noise: a near copy
    eng.update_items(dst, content=rows)
    audit = eng.find_duplicates(0.98)
    count, partner, sim = _np(*audit)
    flagged = np.flatnonzero(count)
    assert flagged.tolist() == sorted(set(src.tolist()) | set(dst.tolist()))
    assert count[[17, 100, 699]].tolist() == [2, 2, 2] and count[[403, 64, 650, 63]].tolist() == [1, 1, 1, 1]
    assert partner[[17, 100, 699, 403, 64, 650, 63]].tolist() == [699, 699, 100, 64, 403, 63, 650]
    assert (np.abs(sim[flagged] - 1) <= tol_sim(H) + 1e-6).all() and (sim[count == 0] == 0).all()
    final = r["content"].copy()
    final[1 + dst] = rows
    _same(_np(*audit), _np(*_engine(content=final).find_duplicates(0.98)), "updated engine against one built from the final table")
    from tcar_amd.host.metrics import duplicate_groups
    assert duplicate_groups(partner) == [[17, 100, 699], [63, 650], [64, 403]]


def test_planted_neighbours_are_audited_as_fp64_audits_them_for_every_row():
    _need_gpu()
    from tcar_amd import _lib
    lib = _lib.load()
    content, _ = planted()
    TOL = tol_sim(P_H)
    assert abs(TOL - 1.54e-5) < 1e-7
    s64 = sims_f64(content, content)
    off = s64.copy()
    np.fill_diagonal(off, -np.inf)
    want = {}
    for t, pairs, rows, margin in ((0.9, 97, 128, 4.0e-4), (0.8, 538, 288, 1.2e-4)):
        count, partner, sim = want[t] = audit_f64(content, t)
        nearest = np.abs(off[np.isfinite(off)] - t).min()
        assert count.sum() == 2 * pairs and (count > 0).sum() == rows and nearest >= 0.99 * margin > 6 * TOL, (t, count.sum(), nearest)
        two = np.sort(off[count > 0], 1)[:, -2:]
        assert (two[:, 1] - two[:, 0]).min() >= 0.016 > 1000 * TOL
    # a plain table in the layout of a context: ek = 2 ldh + 5 ldt floats per row, the content columns at ldh
    ldh, ldt = 256, 64
    E = torch.zeros(P_N, 2 * ldh + 5 * ldt)
    E[:, ldh:ldh + P_H] = torch.from_numpy(np.array(content))
    E = E.cuda()
    ctx, d = _lib.Ctx(), _lib.Dupes()
    ctx.d.n_items, ctx.d.H, ctx.d.Ht, ctx.d.ldh, ctx.d.ldt = P_N, P_H, ldt, ldh, ldt
    ctx.E = E.data_ptr()
    r, psim = torch.zeros(P_N, device="cuda"), torch.full((P_N,), -7.0, device="cuda")
    count, partner = (torch.full((P_N,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    best = torch.full((P_N,), -7, dtype=torch.int64, device="cuda")
    d.r, d.count, d.best, d.partner, d.partner_sim = (x.data_ptr() for x in (r, count, best, partner, psim))
    for t, stripe in ((0.9, 16), (0.8, 47)):
        d.t, d.stripe = t, stripe
        torch.cuda.synchronize()
        assert lib.tcar_dupes_step(C.byref(ctx), C.byref(d), None) == 0
        torch.cuda.synchronize()
        got = _np(count, partner, psim)
        assert (got[0] == want[t][0]).all() and (got[1] == want[t][1]).all(), (t, np.flatnonzero(got[0] != want[t][0])[:5])
        err = np.abs(got[2].astype(np.float64) - want[t][2])
        print("t = %.1f: largest error of a reported sim %.3e (TOL_SIM %.3e)" % (t, err.max(), TOL))
        assert (err <= TOL).all()


def test_the_model_groups_the_audit_and_the_command_line_prints_its_line():
    _need_gpu()
    from tcar_amd.host.cli import main
    from tcar_amd.host.metrics import duplicate_groups
    buf = io.StringIO()
    with redirect_stdout(buf):
        model = main(["--synthetic", "400", "--synthetic_train", "1500", "--synthetic_test", "200", "--epoch", "1", "--hidden_size", "48",
                      "--time_hidden_size", "16", "--batch_size", "64", "--audit_duplicates", "0.98"])
    lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith("duplicate audit")]
    assert lines == ["duplicate audit (cosine >= 0.98): 0 articles in 0 groups, largest 0, 0 pairs"], lines
    assert buf.getvalue().index("Recall@20") < buf.getvalue().index("duplicate audit")    # behind training and its evaluation
    # a threshold the random content does reach: the groups are those of the engine's partner array
    eng = model.engine
    content = np.asarray(eng._content)[1:]
    s64 = sims_f64(content, content)
    np.fill_diagonal(s64, -1)
    t = float(np.sort(s64.max(1))[-40])                                                  # about forty rows have a partner
    groups, audit = model.duplicate_articles(t)
    partner = audit.partner.cpu().numpy()
    assert groups == duplicate_groups(partner) and 5 <= len(groups) and 35 <= sum(len(g) for g in groups) <= 80
    assert all(len(g) >= 2 and g == sorted(g) for g in groups) and [g[0] for g in groups] == sorted(g[0] for g in groups)
    assert {i for g in groups for i in g} >= set(np.flatnonzero(partner >= 0).tolist())
    _same(_np(*audit), _np(*eng.find_duplicates(t)), "duplicate_articles against the engine")
    # a window in minutes installs the keys and audits the articles published inside it
    import datetime
    minutes = np.random.RandomState(5).permutation(len(content)) * 7
    model.publish_time = [datetime.datetime(2020, 1, 1) + datetime.timedelta(minutes=int(m)) for m in minutes]
    keys = model._item_keys()
    assert (keys == minutes).all()
    lo, hi = int(np.sort(keys)[100]), int(np.sort(keys)[300])
    groups_w, audit_w = model.duplicate_articles(t, window=(lo, hi))
    member = (keys >= lo) & (keys < hi)
    count = audit_w.count.cpu().numpy()
    assert not count[~member].any() and groups_w == duplicate_groups(audit_w.partner.cpu().numpy())
    assert all(member[i] for g in groups_w for i in g)
    with pytest.raises(ValueError, match="threshold must be"):
        model.duplicate_articles(0)
