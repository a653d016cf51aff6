"""Evaluation-step throughput (forward + rank / top-20 + CE), B = 512, k = 20.
Usage: python tools/eval_bench.py [iters] [--n_items N] [--streamed [--panel P[,P...]] [--window FRAC[,FRAC...]]
                                                               [--cap M[,M...]] [--cats C] [--cap_skew]] [--rounds R]

       python tools/eval_bench.py [iters] [--n_items N] --streamed --sharded W [--panel P[,P...]] [--rounds R]

--sharded W: the per-rank time of one evaluation step of the catalog-sharded engine at the shapes of RANK 0 of a W-rank job, on one GPU
(W > 1: TCAR_SIM_WORLD=W — every all-gather repeats the local rows, so the buffers have the job's shapes and the results mean nothing
beyond them; the collectives' own time is not in the numbers): ShardedEngine.eval_step, which scores the B local sessions against the
WHOLE catalog on the fp32 GEMM, beside ShardedEngine.eval_step_streamed, which scores the W B gathered sessions against the shard's
N / W rows on its split-bf16 planes and merges W states.

Without --streamed: eval_step (materialised [B, N] scores) at the Globo shape, as before.  With --streamed: eval_step and
eval_step_streamed at every panel size named (default: the engine's default panel), alternating in the same process for `rounds`
rounds so that the spread between rounds is visible; the streamed results are compared with eval_step's at the timed size.
--window FRAC: also the windowed streamed step (include/tcar_window.h) with key = item index and [lo, hi) = the last FRAC of the
catalog for every session, timed beside the unwindowed one at every panel size.
--cap M: also the capped streamed step (include/tcar_quota.h) with at most M items of one category in a list, timed beside the uncapped
one.  The categories are the synthetic fold's own table if it has one, else C = --cats random codes.  --cap_skew adds the catalog
whose items all share ONE category at cap 1: one accepted item and one kill pass per fold, however wide the panel.

       python tools/eval_bench.py [iters] [--n_items N] --candidates C[,C...] [--panel P[,P...]] [--rounds R]

--candidates C: TcarEngine.score_candidates (include/tcar_cand.h) with C uniformly drawn candidates per session and a clicked flag on
slot 0, beside eval_step_streamed of the same engine, alternating for `rounds` rounds.  Per C it prints the whole step (session forward,
the upload of the lists, scores, ranks and metrics) and the two kernels alone (device events around tcar_cand_scores and
tcar_cand_rank on the step's operands), with the gathered bytes — B C rows of ek columns in two bf16 planes — over the scores
kernel's time as a share of the 8 TB/s HBM specification.

       python tools/eval_bench.py [iters] [--n_items N] --retrieve C[,C...] [--k K] [--panel P] [--rounds R]

--retrieve C: TcarEngine.recommend (the streamed selection over exact scores), retrieve (include/tcar_retrieve.h: a shortlist of C from
coarse scores) and recommend_two_stage (shortlist C, re-scored exactly, cut to K) on the same host batches, alternating for `rounds`
rounds: ms per step (upload included in all three), the agreement of the two-stage lists with the streamed ones (mean share of a
streamed list found in the two-stage list, and the share of sessions whose lists are equal), and the two selectors alone — device
events around one fold of the panel the last step left in the panel buffer into a fresh state, tcar_select_panel at K beside
tcar_retrieve_panel at C.  --diversity MU adds recommend_two_stage(diversity=MU) (include/tcar_mmr.h) between two runs of the plain
two-stage call, and the tcar_mmr_walk launch alone on the buffers the call left: at k and at k = 1 (the gather with one pick).

       python tools/eval_bench.py [iters] [--n_items N] --retrieve C[,C...] --sharded W [--k K] [--panel P] [--rounds R]

--retrieve C --sharded W: the catalog-sharded engine at the shapes of rank 0 of a W-rank job (the sim world of --streamed --sharded W:
the collectives' own time is not in the numbers, and the W "shards" a rank merges are copies of its own).  Per rank and round, on the
same host batches: ShardedEngine.recommend (the streamed selection over the shard's exact scores, merged) beside shard_retrieve and
shard_recommend_two_stage at every C, and their ratios.  Then the pieces of the two-stage call alone, device events around each on
the buffers the last call left: the shard's fold, tcar_retrieve_merge, the owners' gather (tcar_shard_cand_scores), tcar_cand_combine,
and ONE tcar_retrieve_panel launch over the engine's panel buffer for B sessions; and the fold with 300 of cap = 512 rows live beside
512 live (a padding session must cost nothing: include/tcar_retrieve_shard.h, tcar_retrieve_panel_live).

       python tools/eval_bench.py [iters] [--n_items N] --sections G[,G...] [--k K] [--cats NCAT] [--panel P] [--rounds R]

--sections G: TcarEngine.recommend_sections (include/tcar_sections.h: the G largest categories as sections, K items each) beside one
recommend() and beside the G windowed recommend() calls it replaces (item keys = categories, window = (code, code + 1)), on the same
host batches, alternating for `rounds` rounds: ms per call (upload included), the ratios, whether the sectioned lists equal the G
windowed ones, and the folds alone — device events around tcar_select_panel at K into a fresh state beside tcar_section_panel from an
empty and from a full state, over the panel the last step left in the panel buffer.

       python tools/eval_bench.py [iters] [--n_items N] --ragged LMAX [--k K] [--panel P] [--rounds R]

--ragged LMAX: B = 512 sessions whose lengths are drawn uniformly from 1 .. LMAX (fixed seed).  TcarEngine.recommend once per length
bucket — what a caller of the rectangular entry points has to do, one stream of the catalog per bucket — beside ONE recommend on the
ragged feed of the same sessions (include/tcar_ragged.h), alternating for `rounds` rounds; ms per request batch, uploads included in
both.  Then the head alone, device events around tcar_ragged_forward on resident batches: one ragged head of all 512 sessions beside
the heads of the buckets (each a ragged call of uniform lengths, which runs exactly the launches of the rectangular head).

       python tools/eval_bench.py [iters] [--n_items N] --similar Q [--k K] [--panel P] [--rounds R]

--similar Q: TcarEngine.similar_items (include/tcar_similar.h) for Q random catalog ids, K items each, beside what a user without it
writes in torch on the same content table: normalize(content) @ normalize(content[q]).T, then torch.topk over the [N, Q] matrix it
materialises — once as written (the table normalised in every call) and once with the normalised table kept between calls.  Host
clock around `iters` calls ending in a device synchronise, the upload of the ids included in all three, alternating for `rounds`
rounds.  Then the split of the call on the device: events around the whole tcar_similar_step and around its cosine panels alone
(tcar_sim_panel over every panel, on the buffers the call left); the rest is the folds with the prologue and the finish.

       python tools/eval_bench.py [iters] [--n_items N] --duplicates T [--dup_dense] [--rounds R]

--duplicates T: TcarEngine.find_duplicates(T) (include/tcar_dupes.h: every pair of content rows once), each call synchronised, the
median of max(iters, 3) calls per round, beside the workaround in the same process: similar_items(512 consecutive ids, k=1) over all
N rows, the host clock around the whole sweep ending in a device synchronise.  Above N = 200,000 the workaround is timed on 16 batches
and scaled to ceil(N / 512); the line says so.  Then the split of the audit by device events: tcar_dup_rnorm, the tcar_dup_tiles
launches of the default stripe (with the fp32 FMA rate of the upper triangle, diagonal tiles whole, and the time per launch) and
tcar_dup_reset + tcar_dup_finish.  --dup_dense: afterwards every content row is overwritten with ONE row — every pair matches, every
tile flushes all its 128 rows — and the audit is timed again: what the atomics cost when everything matches.

       python tools/eval_bench.py [iters] [--n_items N] [--scoring MODE] --update U[,U...] [--sharded W] [--rounds R]

--update U: TcarEngine.update_items (include/tcar_catalog.h) of U random distinct rows on an engine whose time block is clean (so the
row refresh runs), for two payloads — content + mwdhm + key, and the item row alone —, beside what an engine without it has to do for
ONE changed row: load_params(params, content) followed by the first recommend(), and beside the whole-catalog time refresh alone
(device events around tcar_cand_time_fwd_bf16 as the steps call it).  An update is timed two ways, the host clock around work that ends
in a device synchronise both times: `iters` calls back to back (ms per call at full rate, staging included) and single calls, each
synchronised (the median: what one publisher waits).  Everything alternates for `rounds` rounds.
With --sharded W: ShardedEngine.shard_update_items(verify=False) (include/tcar_catalog_shard.h) at the shapes of rank 0 of W ranks —
the sim world, so no collective and no agreement — beside load_params() + the first sharded recommend() on the same engine; the
time refresh alone is the shard's.

       python tools/eval_bench.py [iters] [--n_items N] [--scoring MODE] --warm U[,U...] [--donors K] [--rounds R]

--warm U: TcarEngine.warm_start_items (include/tcar_warm.h) of U random distinct rows, K donors each (--donors, default 16), beside the
two calls it is to be read against on the same engine and the same ids: update_items(ids, item_rows = host rows) — what installing
rows costs when they come from the host — and similar_items(ids, k = K) — what the neighbour lists cost.  Each is timed as --update
times a call: `iters` calls back to back and single synchronised calls (the median), the host clock around work that ends in a device
synchronise.  Then tcar_rows_blend alone, device events around `iters` launches on the lists the call left, and its share of the one
synchronised call.  A warm start that costs much more than update_items + similar_items has a problem in the blend or a
synchronisation that should not exist."""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import tcar_amd  # noqa
from tcar_amd.host.synth import SynthFold
from tcar_amd.host.model import initial_variables
from tcar_amd.engine import TcarEngine
from bench import build_batches, CONFIGS

ap = argparse.ArgumentParser()
ap.add_argument("iters", nargs="?", type=int, default=100)
ap.add_argument("--n_items", type=int, default=46033)
ap.add_argument("--streamed", action="store_true")
ap.add_argument("--panel", type=str, default="", help="comma-separated panel sizes (multiples of 128, <= 49152); empty: the default panel")
ap.add_argument("--window", type=str, default="", help="comma-separated fractions of the catalog (its last items) that form every session's pool")
ap.add_argument("--cap", type=str, default="", help="comma-separated caps: at most M items of one category in a list")
ap.add_argument("--cats", type=int, default=300, help="number of category codes when the synthetic fold carries no category table")
ap.add_argument("--cap_skew", action="store_true", help="also cap 1 on a catalog whose items all share one category")
ap.add_argument("--sharded", type=int, default=0, help="W: the catalog-sharded engine at the shapes of rank 0 of W ranks (with --streamed, --retrieve or --update)")
ap.add_argument("--candidates", type=str, default="", help="comma-separated list lengths C (1 .. 1024) for score_candidates")
ap.add_argument("--retrieve", type=str, default="", help="comma-separated shortlist lengths C (1 .. 1024) for retrieve / recommend_two_stage")
ap.add_argument("--sections", type=str, default="", help="comma-separated section counts G (1 .. 16) for recommend_sections")
ap.add_argument("--diversity", type=float, default=0.0,
                help="MU > 0 (with --retrieve, one engine): also time recommend_two_stage(diversity=MU) (include/tcar_mmr.h), interleaved "
                     "with the plain two-stage call, and the tcar_mmr_walk launch alone with the bytes/s of its gather")
ap.add_argument("--k", type=int, default=20, help="length of the lists of recommend / recommend_two_stage (with --retrieve) and of a section (with --sections)")
ap.add_argument("--similar", type=int, default=0, help="Q: similar_items for Q catalog ids beside the torch workaround that materialises [N, Q]")
ap.add_argument("--duplicates", type=float, default=0.0, help="T in (0, 1]: find_duplicates(T) beside similar_items(512 ids, k=1) over all rows")
ap.add_argument("--dup_dense", action="store_true", help="with --duplicates: also the worst case, every content row equal")
ap.add_argument("--ragged", type=int, default=0, help="LMAX (1 .. 40): one ragged recommend beside one recommend per length bucket")
ap.add_argument("--update", type=str, default="", help="comma-separated row counts U for update_items")
ap.add_argument("--warm", type=str, default="", help="comma-separated row counts U for warm_start_items (with --donors K)")
ap.add_argument("--donors", type=int, default=16, help="K: the donors of one warm-started row and the k of similar_items beside it (with --warm)")
ap.add_argument("--scoring", type=str, default="bf16x3-mixed", help="scoring mode of the engine (f32 | bf16x3 | bf16x3-mixed | bf16)")
ap.add_argument("--rounds", type=int, default=2)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("eval_bench needs the GPU: nothing is measured without it")
N, B, iters = a.n_items, 512, a.iters
fold = SynthFold(n_items=N, dim=250, n_train=60000, n_test=1000, seed=2020, **(dict(lean=True) if N > 200000 else {}))
np.random.seed(2020)
params0 = initial_variables(N, 250, 64, 0.002, 0.05, **(dict(lean=True) if N > 200000 and a.update else {}))
if a.sharded:
    if not a.streamed and not a.retrieve and not a.update:
        sys.exit("--sharded W compares the two evaluation steps of the catalog-sharded engine (--streamed), its two recommendation "
                 "calls (--retrieve C) or a catalog update with a rebuild (--update U): it needs one of them")
    if a.sharded > 1:
        os.environ["TCAR_SIM_WORLD"] = str(a.sharded)
    from tcar_amd.sharded import ShardedEngine
    eng = ShardedEngine(params0, fold.content, fold.mwdhm, device="cuda:0", scoring="bf16x3-mixed")
    assert eng.world == a.sharded
else:
    eng = TcarEngine(params0, fold.content, fold.mwdhm, device="cuda:0", scoring=a.scoring)
batches = build_batches(fold, 16, B, 0, np.random.RandomState(1), CONFIGS["globo"])
res = [eng.make_resident(b) for b in batches]


def timed(step):
    for i in range(5):
        step(res[i % len(res)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(iters):
        step(res[i % len(res)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


plain = lambda bt: eng.eval_step(None, bt=bt)
ups = [int(u) for u in a.update.split(",") if u]
if ups:
    import ctypes as C_
    # --sharded W: ShardedEngine.shard_update_items(verify=False) at the shapes of rank 0 of W ranks (the sim world: no collective, so
    # no agreement either), beside load_params() + the first sharded recommend() of the same engine
    update = (lambda ids, **kw: eng.shard_update_items(ids, verify=False, **kw)) if a.sharded else eng.update_items
    uname = "shard_update_items W=%d" % a.sharded if a.sharded else "update_items"
    if a.sharded:
        a.scoring = "bf16x3-mixed, rank 0 of %d (%d rows)" % (a.sharded, eng.nl)
    g, rng = eng.geo, np.random.RandomState(9)
    feed = {n: v for n, v in batches[0].items() if n not in ("label", "neg")}
    eng.set_item_keys(np.arange(N, dtype=np.int32))
    pay = {}
    for U in ups:
        ids = rng.choice(N, U, replace=False)
        pay[U] = dict(ids=ids, content=(rng.standard_normal((U, g.H)) * 0.5).astype(np.float32),
                      item=(rng.standard_normal((U, g.H)) * 0.002).astype(np.float32),
                      mw=np.stack([rng.randint(1, v, U) for v in (13, 32, 8, 25, 61)], -1).astype(np.int32), keys=ids.astype(np.int32))
    forms = (("content + mwdhm + key", lambda q: update(q["ids"], content=q["content"], mwdhm=q["mw"], keys=q["keys"])),
             ("item row", lambda q: update(q["ids"], item_rows=q["item"])))

    def update_times(call, q):
        """(ms per call of `iters` calls back to back, median ms of single synchronised calls)"""
        for _ in range(5):
            call(q)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            call(q)
        torch.cuda.synchronize()
        rate = (time.perf_counter() - t0) / iters
        one = []
        for _ in range(min(iters, 50)):
            t0 = time.perf_counter()
            call(q)
            torch.cuda.synchronize()
            one.append(time.perf_counter() - t0)
        return rate * 1e3, float(np.median(one)) * 1e3

    def refresh_alone():
        lib, p, st = eng.lib, eng._p, eng._stream()
        planes = bool(eng.scoring_code)
        args = (C_.byref(eng.dims_cand), C_.byref(eng._time_ptrs()), p(eng.mwdhm), None if planes else p(eng.E), p(eng.e16h) if planes else None,
                p(eng.e16l) if planes else None, st)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for it in range(5 + iters):
            if it == 5:
                ev[0].record()
            assert lib.tcar_cand_time_fwd_bf16(*args) == 0
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / iters

    def rebuild():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.load_params(params0, fold.content)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        eng.recommend(feed)
        torch.cuda.synchronize()
        return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

    eng.recommend(feed)                       # the workspace exists and the time block is clean: every update refreshes its rows
    torch.cuda.synchronize()
    row_bytes = 4 * 2 * g.ldh + (4 * g.ek if eng.scoring_code else 4 * g.pt)      # item | content in E, then the row of both planes or the fp32 time block
    print("N=%d scoring=%s: ek=%d, %.1f KB written per row that takes content, item row and publish time (+ %.1f KB of moments)"
          % (N, a.scoring, g.ek, row_bytes / 1e3, 8 * g.ldh / 1e3))
    for rnd in range(a.rounds):
        lp, first = rebuild()
        print("N=%d %s round %d rebuild: load_params %.2f ms + first recommend %.3f ms = %.2f ms" % (N, a.scoring, rnd, lp, first, lp + first))
        assert not eng._time_dirty
        print("N=%d %s round %d whole-catalog time refresh alone: %.4f ms" % (N, a.scoring, rnd, refresh_alone()))
        for U in ups:
            for name, call in forms:
                rate, one = update_times(call, pay[U])
                assert not eng._time_dirty
                print("N=%d %s round %d %s U=%d (%s): %.4f ms per call back to back, %.4f ms one synchronised call = 1 / %.0f of the rebuild"
                      % (N, a.scoring, rnd, uname, U, name, rate, one, (lp + first) / one))
        sys.stdout.flush()
    eng.check_forks()
    sys.exit(0)
warms = [int(u) for u in a.warm.split(",") if u]
if warms:
    import ctypes as C_
    if a.sharded:
        sys.exit("--warm needs the whole catalog on one engine: not with --sharded")
    g, rng = eng.geo, np.random.RandomState(9)
    K = a.donors

    def call_times(call):
        """(ms per call of `iters` calls back to back, median ms of single synchronised calls)"""
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            call()
        torch.cuda.synchronize()
        rate = (time.perf_counter() - t0) / iters
        one = []
        for _ in range(min(iters, 50)):
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            one.append(time.perf_counter() - t0)
        return rate * 1e3, float(np.median(one)) * 1e3

    def blend_alone(U):
        """ms of tcar_rows_blend alone, device events, on the lists and the staging rows the last warm start left"""
        lib, st = eng.lib, eng._stream()
        vp = lambda t: C_.c_void_p(t.data_ptr())
        args = (U, K, g.N, g.H, vp(eng.sel_topk), vp(eng.sel_score), 0.0, vp(eng.E), g.ek, vp(eng.warm_rows), (g.H + 3) // 4 * 4,
                vp(eng.warm_support), vp(eng.warm_wsum), st)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for it in range(5 + iters):
            if it == 5:
                ev[0].record()
            assert lib.tcar_rows_blend(*args) == 0
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / iters

    for rnd in range(a.rounds):
        for U in warms:
            ids = rng.choice(N, U, replace=False)
            rows = (rng.standard_normal((U, g.H)) * 0.002).astype(np.float32)
            upd = call_times(lambda: eng.update_items(ids, item_rows=rows))
            sim = call_times(lambda: eng.similar_items(ids, k=K))
            warm = call_times(lambda: eng.warm_start_items(ids, k=K))
            blend = blend_alone(U)
            gathered = U * K * g.H * 4
            print("N=%d %s round %d U=%d k=%d: warm_start_items %.4f ms back to back, %.4f ms one synchronised call; update_items(item "
                  "rows from the host) %.4f / %.4f ms; similar_items(Q=U) %.4f / %.4f ms; their sum %.4f / %.4f ms; tcar_rows_blend alone "
                  "%.4f ms = %.1f%% of the one call (%.1f GB/s of donor rows)"
                  % (N, a.scoring, rnd, U, K, warm[0], warm[1], upd[0], upd[1], sim[0], sim[1], upd[0] + sim[0], upd[1] + sim[1], blend,
                     100 * blend / warm[1], gathered / blend / 1e6))
            sys.stdout.flush()
    eng.check_forks()
    sys.exit(0)
cands = [int(c) for c in a.candidates.split(",") if c]
if cands:
    import ctypes as C_
    if a.sharded:
        sys.exit("--candidates needs the whole catalog on one engine: not with --sharded")
    panels = [int(p) for p in a.panel.split(",") if p] or [0]
    g, rng = eng.geo, np.random.RandomState(3)
    lists = {c: rng.randint(0, N, (B, c)).astype(np.int32) for c in cands}
    clicked = {c: np.concatenate([np.ones((B, 1), np.int32), np.zeros((B, c - 1), np.int32)], 1) for c in cands}

    def kernels_alone(c):
        """ms of tcar_cand_scores and of tcar_cand_rank alone, on the operands and buffers the last step left on the engine"""
        lib, p, st = eng.lib, eng._p, eng._stream()
        vp = lambda t: C_.c_void_p(t.data_ptr())
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        for it in range(5 + iters):
            if it == 5:
                ev[0].record()
            lib.tcar_cand_scores(B, c, g.N, g.ek, None, 0, None, 0, vp(eng.a16h), vp(eng.a16l), g.ek, vp(eng.e16h), vp(eng.e16l), g.ek, 3,
                                 vp(eng.cand_in[0]), c, vp(eng.cand_score), c, st)
        ev[1].record()
        for it in range(iters):
            lib.tcar_cand_rank(B, c, vp(eng.cand_score), c, vp(eng.cand_in[0]), c, vp(eng.cand_in[1]), c, vp(eng.cand_rank[0]),
                               vp(eng.cand_rank[1]), vp(eng.cand_counts), vp(eng.cand_metrics), st)
        ev[2].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / iters, ev[1].elapsed_time(ev[2]) / iters

    for rnd in range(a.rounds):
        for P in panels:
            dt = timed(lambda bt: eng.eval_step_streamed(None, bt=bt, panel=P or None))
            print("N=%d round %d eval_step_streamed panel=%d: %.3f ms = %.0f sessions/s" % (N, rnd, P or eng.default_panel(), dt * 1e3, B / dt))
        for c in cands:
            dc = timed(lambda bt: eng.score_candidates(None, lists[c], clicked[c], bt=bt))
            ks, kr = kernels_alone(c)
            gathered = B * c * g.ek * 4                       # hi + lo plane, 2 bytes each, of every named row
            print("N=%d round %d score_candidates C=%d: %.3f ms per step = %.0f sessions/s, %.3f of the streamed step; kernels alone: "
                  "scores %.4f ms (%.1f MB gathered = %.2f TB/s = %.3f of 8 TB/s), rank %.4f ms" % (
                      N, rnd, c, dc * 1e3, B / dc, dc / dt, ks, gathered / 1e6, gathered / (ks * 1e-3) / 1e12,
                      gathered / (ks * 1e-3) / 8e12, kr))
        sys.stdout.flush()
    sys.exit(0)
shorts = [int(c) for c in a.retrieve.split(",") if c]
if shorts and a.sharded:
    import ctypes as C_
    P = ([int(p) for p in a.panel.split(",") if p] or [0])[0] or None
    K, W, g = a.k, eng.world, eng.geo
    feeds = [{n: v for n, v in b.items() if n not in ("label", "neg")} for b in batches]
    vp = lambda t, off=0: C_.c_void_p(t.data_ptr() + 4 * off)

    def timed_host(step):
        for i in range(5):
            step(feeds[i % len(feeds)])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(iters):
            step(feeds[i % len(feeds)])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters

    def events(fn):
        """ms per call of fn on the step's stream: device events around `iters` calls behind 5 warm ones"""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for it in range(5 + iters):
            if it == 5:
                ev[0].record()
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / iters

    def pieces_alone(c):
        """the pieces of ONE shard_recommend_two_stage on the buffers the call left on the engine"""
        eng.shard_recommend_two_stage(feeds[0], k=K, shortlist=c, panel=P)
        pc, lib, st = eng._retrieve_pc, eng.lib, eng._stream()
        cap, rw = pc.cap, 2 * c + 4
        states, parts, lists = pc._states, pc._parts, pc._lists
        fold = events(pc.fold)
        merge = events(lambda: lib.tcar_retrieve_merge(cap, c, W, vp(states), cap * rw, vp(eng.rs_merged), st))
        gather = events(lambda: pc.scores(lists))
        comb = events(lambda: lib.tcar_cand_combine(cap, c, W, eng.S, g.N, vp(eng.rs_ids), c, vp(parts), cap * c, vp(eng.rs_exact), c, st))
        width = eng.sv_panel.shape[1]
        n = min(width, eng.nl)

        def one_panel():
            lib.tcar_retrieve_reset(cap, c, vp(eng.rs_state), st)
            lib.tcar_retrieve_panel(cap, 0, n, vp(eng.sv_panel), width, c, None, 0, None, None, None, vp(eng.rs_state), st)
        panel = events(one_panel)
        return fold, merge, gather, comb, panel, n

    def fold_live(c, live):
        """ms of the shard's fold alone with `live` of cap = B rows of every rank live (the others padding sessions)"""
        f = {n_: v[:live] for n_, v in feeds[0].items()}
        pc = eng.retrieve_pieces(f, c, K, panel=P, cap=B)
        pc.prepare(eng.xch.all_gather(pc.begin()).view(W * B, -1))
        return events(pc.fold)

    print("N=%d sharded W=%d: shard of %d rows, %d gathered sessions per step, k=%d" % (N, W, eng.nl, W * B, K))
    for rnd in range(a.rounds):
        dt = timed_host(lambda f: eng.recommend(f, k=K, panel=P))
        print("N=%d W=%d round %d sharded recommend k=%d: %.3f ms = %.0f sessions/s" % (N, W, rnd, K, dt * 1e3, B / dt))
        for c in shorts:
            dr = timed_host(lambda f: eng.shard_retrieve(f, c, panel=P))
            d2 = timed_host(lambda f: eng.shard_recommend_two_stage(f, k=K, shortlist=c, panel=P))
            print("N=%d W=%d round %d C=%d: shard_retrieve %.3f ms (%.3f of recommend), shard_recommend_two_stage %.3f ms (%.3f of recommend)"
                  % (N, W, rnd, c, dr * 1e3, dr / dt, d2 * 1e3, d2 / dt))
        sys.stdout.flush()
    for c in shorts:
        fold, merge, gather, comb, panel, n = pieces_alone(c)
        print("N=%d W=%d C=%d pieces alone: fold of the shard %.3f ms, merge of %d states x %d sessions %.4f ms, owners' gather %.4f ms, "
              "combine %.4f ms; one tcar_retrieve_panel of %d columns x %d sessions %.4f ms" % (N, W, c, fold, W, B, merge, gather, comb, n, B, panel))
        f512, f300 = fold_live(c, B), fold_live(c, 300)
        print("N=%d W=%d C=%d fold with cap=%d: %d live %.3f ms, 300 live %.3f ms (%.3f)" % (N, W, c, B, B, f512, f300, f300 / f512))
        sys.stdout.flush()
    sys.exit(0)
if shorts:
    import ctypes as C_
    P = ([int(p) for p in a.panel.split(",") if p] or [0])[0] or None
    K = a.k
    feeds = [{n: v for n, v in b.items() if n not in ("label", "neg")} for b in batches]

    def timed_host(step):
        for i in range(5):
            step(feeds[i % len(feeds)])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(iters):
            step(feeds[i % len(feeds)])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters

    def folds_alone(c):
        """ms of one tcar_select_panel (k = K) and one tcar_retrieve_panel (C = c) over the panel buffer as the last step left it,
        each into a freshly reset state (the reset is inside the timed region of both)"""
        lib, st = eng.lib, eng._stream()
        vp = lambda t: C_.c_void_p(t.data_ptr())
        n = min(eng.panel_buf.shape[1], N)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        for it in range(5 + iters):
            if it == 5:
                ev[0].record()
            lib.tcar_select_reset(B, K, vp(eng.sel_state), st)
            lib.tcar_select_panel(B, 0, n, vp(eng.panel_buf), eng.panel_buf.shape[1], K, None, None, None, 0, vp(eng.sel_state), st)
        ev[1].record()
        for it in range(iters):
            lib.tcar_retrieve_reset(B, c, vp(eng.rt_state), st)
            lib.tcar_retrieve_panel(B, 0, n, vp(eng.panel_buf), eng.panel_buf.shape[1], c, None, 0, None, None, None, vp(eng.rt_state), st)
        ev[2].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / iters, ev[1].elapsed_time(ev[2]) / iters

    for c in shorts:             # agreement on every batch, outside the timed loops
        found, same = [], []
        for f in feeds:
            t0 = eng.recommend(f, k=K, panel=P)[0].clone()
            t1 = eng.recommend_two_stage(f, k=K, shortlist=c, panel=P)[0]
            found.append(((t0[:, :, None] == t1[:, None, :]) & (t0[:, :, None] >= 0)).any(2).float().mean().item())
            same.append((t0 == t1).all(1).float().mean().item())
        print("N=%d k=%d shortlist=%d: share of the streamed lists found in the two-stage lists %.5f, sessions with equal lists %.4f" % (
            N, K, c, float(np.mean(found)), float(np.mean(same))))
    for rnd in range(a.rounds):
        dt = timed_host(lambda f: eng.recommend(f, k=K, panel=P))
        print("N=%d round %d recommend k=%d: %.3f ms = %.0f sessions/s" % (N, rnd, K, dt * 1e3, B / dt))
        for c in shorts:
            dr = timed_host(lambda f: eng.retrieve(f, c, panel=P))
            d2 = timed_host(lambda f: eng.recommend_two_stage(f, k=K, shortlist=c, panel=P))
            fs, fr = folds_alone(c)
            print("N=%d round %d C=%d: retrieve %.3f ms (%.3f of recommend), recommend_two_stage %.3f ms (%.3f of recommend); one fold of "
                  "%d columns alone: select k=%d %.4f ms, retrieve C=%d %.4f ms" % (
                      N, rnd, c, dr * 1e3, dr / dt, d2 * 1e3, d2 / dt, min(eng.panel_buf.shape[1], N), K, fs, c, fr))
            if a.diversity > 0:
                # interleaved with the plain call of the same build: plain, diversified, plain; the walk alone on the buffers the
                # diversified call left (device events around `iters` launches), k = 1 being the gather with no round behind it
                g = eng.geo
                dd = timed_host(lambda f: eng.recommend_two_stage(f, k=K, shortlist=c, panel=P, diversity=a.diversity))
                d3 = timed_host(lambda f: eng.recommend_two_stage(f, k=K, shortlist=c, panel=P))
                eng.recommend_two_stage(feeds[0], k=K, shortlist=c, panel=P, diversity=a.diversity)
                vp = lambda t, off=0: C_.c_void_p(t.data_ptr() + 4 * off)

                def walk_alone(kk):
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                    for it in range(5 + iters):
                        if it == 5:
                            ev[0].record()
                        eng.lib.tcar_mmr_walk(B, c, kk, a.diversity, g.N, g.H, vp(eng.E, g.ldh), g.ek, vp(eng.rt_ids), c, vp(eng.rt_exact), c,
                                              vp(eng.rt_rank[1]), vp(eng.rt_topk), vp(eng.rt_topscore), vp(eng.rt_msim), eng._stream())
                    ev[1].record()
                    torch.cuda.synchronize()
                    return ev[0].elapsed_time(ev[1]) / iters
                wk, w1 = walk_alone(K), walk_alone(1)
                pool = int(((eng.rt_ids[:B] >= 0).sum(1).clamp(max=256)).sum().item())
                gathered = pool * g.H * 4
                print("N=%d round %d C=%d diversity=%g: two-stage %.3f / %.3f ms around diversified %.3f ms (+%.3f ms); walk alone k=%d "
                      "%.4f ms = %.3f of the diversified call; k=1 (the gather and one pick) %.4f ms: %.1f MB of rows = %.2f TB/s; %.4f ms "
                      "per further round" % (N, rnd, c, a.diversity, d2 * 1e3, d3 * 1e3, dd * 1e3, (dd - 0.5 * (d2 + d3)) * 1e3, K, wk,
                                             wk / (dd * 1e3), w1, gathered / 1e6, gathered / (w1 * 1e-3) / 1e12, (wk - w1) / max(K - 1, 1)))
        sys.stdout.flush()
    sys.exit(0)
if a.duplicates:
    import ctypes as C_
    if a.sharded:
        sys.exit("--duplicates needs the whole catalog on one engine: not with --sharded")
    T_, g = a.duplicates, eng.geo
    nb = (N + 63) // 64
    calls = max(iters, 3) if N <= 200000 else 3
    QB = 512
    nbatch = (N + QB - 1) // QB
    sampled = nbatch if N <= 200000 else 16

    def audit_ms():
        out = []
        for _ in range(calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.find_duplicates(T_)
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(out))

    def workaround_ms():
        """similar_items(512 ids, k=1) over `sampled` batches spread over the catalog, scaled to all nbatch of them"""
        starts = np.linspace(0, nbatch - 1, sampled).astype(np.int64) * QB
        eng.similar_items(np.arange(0, min(QB, N), dtype=np.int32), k=1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s0 in starts:
            eng.similar_items(np.arange(s0, min(s0 + QB, N), dtype=np.int32), k=1)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 * nbatch / sampled

    def split_ms():
        """device events around the three parts of one audit, on the buffers the last call left: rnorm | the stripes | reset + finish"""
        lib, st = eng.lib, eng._stream()
        vp = lambda t: C_.c_void_p(t.data_ptr())
        cp = C_.c_void_p(eng.E.data_ptr() + 4 * g.ldh)
        stripe = eng._dupes_request(T_, None, None)[2]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        assert lib.tcar_dup_rnorm(N, g.H, cp, g.ek, vp(eng.dup_r), st) == 0
        ev[1].record()
        launches = 0
        for b0 in range(0, nb, stripe):
            assert lib.tcar_dup_tiles(N, g.H, cp, g.ek, vp(eng.dup_r), b0, min(b0 + stripe, nb), T_, None, 0, 0, vp(eng.dup_count),
                                      vp(eng.dup_best), st) == 0
            launches += 1
        ev[2].record()
        assert lib.tcar_dup_reset(N, vp(eng.dup_count), vp(eng.dup_best), st) == 0
        assert lib.tcar_dup_finish(N, vp(eng.dup_best), vp(eng.dup_partner), vp(eng.dup_sim), st) == 0
        ev[3].record()
        torch.cuda.synchronize()
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(3)] + [launches, stripe]

    def report(what, rnd, with_workaround):
        da = audit_ms()
        dw = workaround_ms() if with_workaround else None
        rn, tiles, fin, launches, stripe = split_ms()
        count = eng.find_duplicates(T_).count
        flagged, pairs = int((count > 0).sum().item()), int(count.sum(dtype=torch.int64).item()) // 2
        flops = 2.0 * (nb * (nb + 1) // 2) * 64 * 64 * ((g.H + 7) // 8 * 8)
        line = ("N=%d t=%g %s round %d: find_duplicates %.3f ms (median of %d synchronised calls; %d rows flagged, %d pairs); on the "
                "device: rnorm %.3f ms, tiles %.3f ms in %d launches of %d row blocks (%.3f ms per launch, %.1f TFLOP/s fp32 over the "
                "upper triangle), reset + finish %.3f ms" % (N, T_, what, rnd, da, calls, flagged, pairs, rn, tiles, launches, stripe,
                                                            tiles / launches, flops / (tiles * 1e-3) / 1e12, fin))
        if dw is not None:
            line += ("; workaround similar_items(%d ids, k=1) over all rows %.1f ms (%s) = %.2fx the audit"
                     % (QB, dw, "all %d batches timed" % nbatch if sampled == nbatch else
                        "%d of %d batches timed, scaled" % (sampled, nbatch), dw / da))
        print(line)
        sys.stdout.flush()

    for rnd in range(a.rounds):
        report("synthetic content", rnd, True)
    if a.dup_dense:
        eng.E[:N, g.ldh:g.ldh + g.H] = eng.E[1, g.ldh:g.ldh + g.H].clone()      # the content is read in place: every row is now one row
        torch.cuda.synchronize()
        for rnd in range(a.rounds):
            report("dense (all rows equal)", rnd, False)
    sys.exit(0)
if a.similar:
    import ctypes as C_
    if a.sharded:
        sys.exit("--similar needs the whole catalog on one engine: not with --sharded")
    Q, K, g = a.similar, a.k, eng.geo
    P = ([int(p) for p in a.panel.split(",") if p] or [0])[0] or None
    rng = np.random.RandomState(5)
    queries = [rng.choice(N, Q, replace=False).astype(np.int32) for _ in range(8)]
    table = eng.E[:N, g.ldh:g.ldh + g.H]                 # the content columns in place (a strided view)
    kept = torch.nn.functional.normalize(table, dim=1)

    def ours(q):
        return eng.similar_items(q, k=K, exclude_self=False, panel=P)

    def as_written(q):
        xn = torch.nn.functional.normalize(table, dim=1)
        return torch.topk(xn @ xn[torch.from_numpy(q).to(eng.dev).long()].T, K, dim=0)

    def table_kept(q):
        return torch.topk(kept @ kept[torch.from_numpy(q).to(eng.dev).long()].T, K, dim=0)

    def timed_host(step):
        for i in range(3):
            step(queries[i % len(queries)])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(iters):
            step(queries[i % len(queries)])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters

    def on_device():
        """ms of the whole tcar_similar_step and of its cosine panels alone, device events, on the buffers the last call left"""
        lib, st = eng.lib, eng._stream()
        vp = lambda t: C_.c_void_p(t.data_ptr())
        ours(queries[0])
        ld = eng.panel_buf.shape[1]
        cp = C_.c_void_p(eng.E.data_ptr() + 4 * g.ldh)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        qd = torch.from_numpy(queries[0]).to(eng.dev)
        from tcar_amd import _lib as L_
        d, s_ = L_.Similar(), eng._serve_desc(K, ld, eng.panel_buf, eng.sel_state, outputs=(eng.sel_topk, eng.sel_score))
        d.qid, d.xq, d.rq = qd.data_ptr(), eng.sm_xq.data_ptr(), eng.sm_rq.data_ptr()
        ctx = eng._catalog_ctx()
        for it in range(3 + iters):
            if it == 3:
                ev[0].record()
            assert lib.tcar_similar_step(C_.byref(ctx), Q, C_.byref(d), C_.byref(s_), None, None, st) == 0
        ev[1].record()
        for it in range(iters):
            for n0 in range(0, N, ld):
                assert lib.tcar_sim_panel(Q, n0, min(ld, N - n0), g.H, cp, g.ek, vp(eng.sm_xq), g.ldh, vp(eng.sm_rq), vp(eng.panel_buf), ld, st) == 0
        ev[2].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / iters, ev[1].elapsed_time(ev[2]) / iters, (N + ld - 1) // ld, ld

    # the same lists?  outside the timed loops; rounding may order near-ties differently, so the share of equal lists is reported
    got = ours(queries[0])[0].clone().cpu().numpy()
    want = table_kept(queries[0])[1].T.cpu().numpy()
    inter = np.mean([len(set(x.tolist()) & set(y.tolist())) / float(K) for x, y in zip(got, want)])
    print("N=%d Q=%d k=%d: lists equal to the workaround's in %.3f of the queries, mean overlap %.4f" % (
        N, Q, K, float((got == want).all(1).mean()), inter))
    for rnd in range(a.rounds):
        do, dw, dk = timed_host(ours), timed_host(as_written), timed_host(table_kept)
        whole, panels, npan, ld = on_device()
        flops = 2.0 * Q * N * ((g.H + 7) // 8 * 8)
        print("N=%d Q=%d k=%d round %d: similar_items %.3f ms; workaround as written %.3f ms (%.2fx), with the normalised table kept "
              "%.3f ms (%.2fx); on the device: the step %.3f ms, its %d cosine panels of %d columns alone %.3f ms (%.1f TFLOP/s fp32), "
              "folds + prologue + finish %.3f ms" % (N, Q, K, rnd, do * 1e3, dw * 1e3, dw / do, dk * 1e3, dk / do, whole, npan, ld, panels,
                                                    flops / (panels * 1e-3) / 1e12, whole - panels))
        sys.stdout.flush()
    sys.exit(0)
sects = [int(g) for g in a.sections.split(",") if g]
if sects:
    # --sections G: TcarEngine.recommend_sections (include/tcar_sections.h: G lists from one pass) beside ONE recommend() and beside
    # the G windowed recommend() calls it replaces — an engine whose item keys are the categories, window = (code, code + 1).  The
    # protocol of the --retrieve table: host clock around `iters` calls ending in a device synchronise, the upload included, rounds
    # alternating; then the folds alone with device events over the panel buffer as the last step left it.
    import ctypes as C_
    from tcar_amd.host import metrics as M_
    if a.sharded:
        sys.exit("--sections needs the whole catalog on one engine: not with --sharded")
    if any(not 1 <= g <= 16 for g in sects):
        sys.exit("--sections G: 1 .. 16")
    P = ([int(p) for p in a.panel.split(",") if p] or [0])[0] or None
    K = a.k
    cat = getattr(fold, "category", None)
    if cat is None or len(cat) != N:
        cat = np.random.RandomState(7).randint(0, a.cats, N)
    cat = np.asarray(cat, dtype=np.int32)
    eng.set_categories(cat)
    eng.set_item_keys(cat)
    feeds = [{n: v for n, v in b.items() if n not in ("label", "neg")} for b in batches]

    def timed_host(step):
        for i in range(5):
            step(feeds[i % len(feeds)])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(iters):
            step(feeds[i % len(feeds)])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters

    def by_windows(f, codes):
        for c in codes:
            eng.recommend(f, k=K, panel=P, window=(int(c), int(c) + 1))

    def folds_alone(codes):
        """ms of one tcar_select_panel (k = K) into a freshly reset state, and of one tcar_section_panel over the same panel buffer
        from an EMPTY state (reset inside the timed region, as for the select fold) and from a FULL one: the state the fold before
        left, folded onto again.  That state is full, and nothing of the same panel can enter it again, only where every section holds
        at least K items in the panel; a shorter section keeps the threshold "nothing" and would admit its items a second time, which
        is neither a full state nor a fold the contract allows (every item once).  Then the third figure is nan and not measured."""
        lib, st = eng.lib, eng._stream()
        vp = lambda t: C_.c_void_p(t.data_ptr())
        G = len(codes)
        arr = (C_.c_int32 * G)(*[int(c) for c in codes])
        n, ld = min(eng.panel_buf.shape[1], N), eng.panel_buf.shape[1]
        sel = torch.empty(B * (2 * K + 4), dtype=torch.int32, device=eng.dev)
        sec = torch.empty(B * G * (2 * K + 4), dtype=torch.int32, device=eng.dev)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        for it in range(5 + iters):
            if it == 5:
                ev[0].record()
            lib.tcar_select_reset(B, K, vp(sel), st)
            lib.tcar_select_panel(B, 0, n, vp(eng.panel_buf), ld, K, None, None, None, 0, vp(sel), st)
        ev[1].record()
        for it in range(iters):
            lib.tcar_select_reset(B * G, K, vp(sec), st)
            lib.tcar_section_panel(B, 0, n, vp(eng.panel_buf), ld, K, G, arr, vp(eng._cat), None, 0, None, None, None, vp(sec), st)
        ev[2].record()
        full = min(int((cat[:n] == c).sum()) for c in codes) >= K          # every row of the state holds K entries
        for it in range(iters if full else 0):
            lib.tcar_section_panel(B, 0, n, vp(eng.panel_buf), ld, K, G, arr, vp(eng._cat), None, 0, None, None, None, vp(sec), st)
        ev[3].record()
        torch.cuda.synchronize()
        return [ev[i].elapsed_time(ev[i + 1]) / iters for i in range(2)] + [ev[2].elapsed_time(ev[3]) / iters if full else float("nan")]

    for G in sects:              # the same lists?  on every batch, outside the timed loops
        codes = M_.largest_categories(cat, G)
        same = []
        for f in feeds[:4]:
            got = eng.recommend_sections(f, codes, k=K, panel=P).topk.clone()
            want = torch.stack([eng.recommend(f, k=K, panel=P, window=(int(c), int(c) + 1))[0].clone() for c in codes], 1)
            same.append((got == want).all().item())
        print("N=%d k=%d G=%d (%d categories, sections of %d .. %d items): sectioned lists equal to the G windowed lists on every batch: %s" % (
            N, K, len(codes), len(np.unique(cat)), min((cat == c).sum() for c in codes), max((cat == c).sum() for c in codes), all(same)))
    for rnd in range(a.rounds):
        dt = timed_host(lambda f: eng.recommend(f, k=K, panel=P))
        print("N=%d round %d recommend k=%d: %.3f ms = %.0f sessions/s" % (N, rnd, K, dt * 1e3, B / dt))
        for G in sects:
            codes = M_.largest_categories(cat, G)
            ds = timed_host(lambda f: eng.recommend_sections(f, codes, k=K, panel=P))
            dw = timed_host(lambda f: by_windows(f, codes))
            fs, fe, ff = folds_alone(codes)
            print("N=%d round %d G=%d: recommend_sections %.3f ms (%.3f of one recommend, %.3f of the G windowed calls), G windowed "
                  "recommend calls %.3f ms; one fold of %d columns alone: select k=%d %.4f ms, sections from an empty state %.4f ms, "
                  "from a full state %.4f ms%s" % (
                      N, rnd, len(codes), ds * 1e3, ds / dt, ds / dw, dw * 1e3, min(eng.panel_buf.shape[1], N), K, fs, fe, ff,
                      "" if ff == ff else " (not measured: a section holds fewer than k = %d items in the panel, so no state of it is full)" % K))
        sys.stdout.flush()
    sys.exit(0)
if a.ragged:
    import ctypes as C_
    from tcar_amd.host.data import PER_ROW, pack_sessions
    if a.sharded:
        sys.exit("--ragged needs the whole catalog on one engine: not with --sharded")
    if not 1 <= a.ragged <= 40:
        sys.exit("--ragged LMAX: 1 .. 40")
    P = ([int(p) for p in a.panel.split(",") if p] or [0])[0] or None
    K, LMAX = a.k, a.ragged
    rng = np.random.RandomState(5)
    lens = rng.randint(1, LMAX + 1, B).astype(np.int32)
    R = int(lens.sum())
    hi = dict(seq=(1, N + 1), pm=(1, 13), pd=(1, 32), pw=(1, 8), ph=(1, 25), pmi=(1, 61), gap=(0, 12))
    ragged = {n: rng.randint(hi[n][0], hi[n][1], R).astype(np.int32) for n in PER_ROW}
    ragged.update(cw=rng.randint(0, 7, B).astype(np.int32), ch=rng.randint(0, 24, B).astype(np.int32), len=lens)
    off = np.concatenate([[0], np.cumsum(lens)])
    buckets, members = [], []
    for L in np.unique(lens):                 # the same sessions, one rectangular feed per length
        idx = np.where(lens == L)[0]
        rows = off[idx][:, None] + np.arange(L)[None, :]
        f = {n: ragged[n][rows] for n in PER_ROW}
        f.update(cw=ragged["cw"][idx], ch=ragged["ch"][idx])
        buckets.append(f)
        members.append(idx)
    print("N=%d B=%d LMAX=%d: %d rows, %d length buckets of %d .. %d sessions" % (
        N, B, LMAX, R, len(buckets), min(len(m) for m in members), max(len(m) for m in members)))
    # the same lists?  (a bucket's panel GEMM has other row counts than the ragged call's: the scores may differ in the last bits)
    tr = eng.recommend(ragged, k=K, panel=P)[0].clone()
    same = np.zeros(B, bool)
    for f, idx in zip(buckets, members):
        same[idx] = (eng.recommend(f, k=K, panel=P)[0] == tr[torch.as_tensor(idx, device=tr.device)]).all(1).cpu().numpy()
    print("N=%d LMAX=%d: sessions whose bucketed and ragged lists are equal %.4f" % (N, LMAX, same.mean()))

    def timed_calls(step):
        for i in range(3):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(iters):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters

    def bucketed():
        for f in buckets:
            eng.recommend(f, k=K, panel=P)

    # the heads alone, on resident batches
    bt_all = eng.make_resident(ragged)
    bt_buckets = [eng.make_resident(pack_sessions([f])) for f in buckets]
    eng._ensure_work(B, LMAX, R)

    def heads_alone(bts):
        lib, st, ctx = eng.lib, eng._stream(), eng._ctx()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for it in range(3 + iters):
            if it == 3:
                ev[0].record()
            for bt in bts:
                rc = lib.tcar_ragged_forward(C_.byref(ctx), C_.byref(bt), C_.byref(bt._rg), 0, st)
                assert rc == 0, rc
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / iters

    for rnd in range(a.rounds):              # the two forms alternate: the spread between rounds is visible
        db = timed_calls(bucketed)
        dr = timed_calls(lambda: eng.recommend(ragged, k=K, panel=P))
        hb, hr = heads_alone(bt_buckets), heads_alone([bt_all])
        print("N=%d LMAX=%d round %d: recommend per bucket (%d calls) %.3f ms, ragged recommend (1 call) %.3f ms = %.3f of the bucketed "
              "form = %.2f bucket calls; heads alone: %d bucket heads %.4f ms, one ragged head %.4f ms" % (
                  N, LMAX, rnd, len(buckets), db * 1e3, dr * 1e3, dr / db, dr / (db / len(buckets)), len(buckets), hb, hr))
        sys.stdout.flush()
    eng.check_forks()
    sys.exit(0)
if not a.streamed:
    dt = timed(plain)
    print("eval step: %.3f ms  = %.0f sessions/s" % (dt * 1e3, B / dt))
    sys.exit(0)
panels = [int(p) for p in a.panel.split(",") if p] or [0]
if a.sharded:
    W = eng.world
    print("N=%d sharded W=%d: shard of %d rows, %d gathered sessions per step" % (N, W, eng.nl, W * B))
    if W == 1 and eng.geo.Npad <= 49152:       # one shard: the two steps see the same catalog, so their results compare
        r0, t0, c0 = [x.clone() for x in eng.eval_step(None, bt=res[0])]
        r1, t1, c1 = eng.eval_step_streamed(None, bt=res[0], panel=panels[0] or None)
        print("N=%d W=1: rank equal %.4f, top-20 rows equal %.4f, max |ce diff| %.2e" % (
            N, (r0 == r1).float().mean().item(), (t0 == t1).all(1).float().mean().item(), (c0 - c1).abs().max().item()))
    # ShardedEngine.eval_step ends in tcar_eval_rows with a CE output, which takes rows of at most 49,152 columns: beyond that the
    # materialised step returns an argument error, so only the streamed step is timed
    wide = eng.geo.Npad > 49152
    if wide:
        print("N=%d W=%d: ShardedEngine.eval_step does not run at this size (tcar_eval_rows takes no CE for rows wider than 49,152 "
              "columns): nothing to set the streamed step beside" % (N, W))
    for rnd in range(a.rounds):
        dt = None
        if not wide:
            dt = timed(plain)
            print("N=%d W=%d round %d sharded eval_step (materialised, whole catalog, fp32): %.3f ms = %.0f sessions/s" % (N, W, rnd, dt * 1e3, B / dt))
        for P in panels:
            ds = timed(lambda bt: eng.eval_step_streamed(None, bt=bt, panel=P or None, cap=B))
            print("N=%d W=%d round %d sharded eval_step_streamed panel=%d: %.3f ms = %.0f sessions/s%s" % (
                N, W, rnd, P or eng.default_panel(), ds * 1e3, B / ds, ", %.3f of the materialised step" % (ds / dt) if dt else ""))
        sys.stdout.flush()
    sys.exit(0)
fracs = [float(f) for f in a.window.split(",") if f]
if fracs:
    eng.set_item_keys(np.arange(N, dtype=np.int32))
windows = [(f, (N - int(round(f * N)), N)) for f in fracs]
caps = [int(m) for m in a.cap.split(",") if m]
cat = getattr(fold, "category", None)
if cat is None or len(cat) != N:
    cat = np.random.RandomState(7).randint(0, a.cats, N)
cat = np.asarray(cat, dtype=np.int32)
quotas = [("cap=%d, %d categories" % (m, len(np.unique(cat))), cat, m) for m in caps]
if a.cap_skew:
    quotas.append(("cap=1, one category", np.zeros(N, np.int32), 1))
# same results?  (the panel GEMM may take another tile than the whole-catalog launch: the scores may differ in the last bits)
r0, t0, c0 = [x.clone() for x in eng.eval_step(None, bt=res[0])]
for P in panels:
    r1, t1, c1 = eng.eval_step_streamed(None, bt=res[0], panel=P or None)
    print("N=%d panel=%s: rank equal %.4f, top-20 rows equal %.4f, max |ce diff| %.2e" % (
        N, P or eng.default_panel(), (r0 == r1).float().mean().item(), (t0 == t1).all(1).float().mean().item(), (c0 - c1).abs().max().item()))
for rnd in range(a.rounds):
    dt = timed(plain)
    print("N=%d round %d eval_step (materialised): %.3f ms = %.0f sessions/s" % (N, rnd, dt * 1e3, B / dt))
    for P in panels:
        dt = timed(lambda bt: eng.eval_step_streamed(None, bt=bt, panel=P or None))
        print("N=%d round %d eval_step_streamed panel=%d: %.3f ms = %.0f sessions/s" % (N, rnd, P or eng.default_panel(), dt * 1e3, B / dt))
        for f, w in windows:
            dw = timed(lambda bt: eng.eval_step_streamed(None, bt=bt, panel=P or None, window=w))
            print("N=%d round %d eval_step_streamed panel=%d window=%g: %.3f ms = %.0f sessions/s, %.3f of the unwindowed step" % (
                N, rnd, P or eng.default_panel(), f, dw * 1e3, B / dw, dw / dt))
        table = None
        for name, c, m in quotas:
            if c is not table:
                eng.set_categories(c)
                table = c
            dq = timed(lambda bt: eng.eval_step_streamed(None, bt=bt, panel=P or None, max_per_category=m))
            print("N=%d round %d eval_step_streamed panel=%d %s: %.3f ms = %.0f sessions/s, %.3f of the uncapped step" % (
                N, rnd, P or eng.default_panel(), name, dq * 1e3, B / dq, dq / dt))
    sys.stdout.flush()
