"""The optimizer half of a training step against independent references (run with -m gpu on an MI355X).

A. Every update kernel of csrc/optim.hip — tcar_clip_adam + tcar_clip_adam_2d, + _2d_bf16, _all, _early + _rest, _early + _rest_keep —
   against the float64 restatement of model_combine.py:155-163 (optim_ref.adam64): m, v, w element-wise inside bounds that count the
   fp32 roundings, the bf16 hi / lo planes of the item table, the bitmap of the split forms, and everything a launch must not touch.
B. The engines' updates against the CPU oracle, one teacher-forced step at a time: Adam moments, clip branch by branch, the weights
   against the engine's own moments and the bias-corrected rate of the step, and an evaluation behind the last update.
tests/test_optimizer_ref.py shows on the CPU that the bounds admit a correct fp32 implementation and reject a wrong clip."""
import ctypes as C

import numpy as np
import pytest
import torch

import optim_ref as R
from gpu_util import _kb32_index, close, lib, ptr, ptr2  # noqa: F401  (lib: the module-scoped fixture)

pytestmark = pytest.mark.gpu

SENT = 0x5A5A5A5A                       # untouched regions: 1.5e16 as a float, 0x5A5A as a bf16
FORMS = ["2d", "2d_bf16", "all", "early_rest", "early_rest_keep"]
_REF = {}


def _reference(shape, clip):
    """float64 targets of one (shape, clip), shared by the five forms; never modified"""
    key = (shape, clip)
    if key not in _REF:
        x = R.a_inputs(shape)
        args = R.adam_args(R.A_STEP, clip)
        sc = lambda slot, dt=np.float64: R.clip_scale(x["sqn_dense"], x["sqn_pieces"], x["use_dense"], slot, args[0], dtype=dt)
        ref = {"item": R.adam64(x["w2"], x["g2"], x["m2"], x["v2"], sc(R.ITEM_SLOT), args)}
        for name, (slot, off, n) in zip("abcd", R.ARENA_SEGS):
            s = slice(off, off + n)
            ref[name] = R.adam64(x["w"][s], x["g"][s], x["m"][s], x["v"][s], sc(slot), args)
        slot_c, off_c, n_c = R.ARENA_SEGS[2]
        s = slice(off_c, off_c + n_c)
        ref["c32"] = R.adam32(x["w"][s], x["g"][s], x["m"][s], x["v"][s], 1.0, args)
        _REF[key] = (x, args, ref)
    return _REF[key]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape,clip", [("rows131", R.A_CLIP), ("rows131", 0.0), ("one_row", R.A_CLIP), ("strided_walk", R.A_CLIP)])
def test_update_kernels_match_the_float64_restatement(lib, shape, clip, form):
    """Bounds (optim_ref.gate_a; every fp32 operation of adam1 / clip_factor rounds once, by at most 2^-24 relative):
    |dm| <= 2^-21 (|b1 m0| + |(1 - b1) gc|), |dv| <= 2^-21 v, |dw| <= 2^-23 |w0| + 2^-20 |lr_t m / (sqrt(v) + eps)|; the largest shape
    takes the factor optim_ref.A_W_FACTOR on w (measured on the CPU with the float32 restatement: 1.46 of the bound, doubled).
    Measured on an MI355X, worst error / bound: m 0.33, v 0.33, w 0.50 — the figures of the float32 restatement on the CPU."""
    from tcar_amd._lib import Segments
    x, args, ref = _reference(shape, clip)
    rows, cols, ldw, ld16, prow = (x[k] for k in ("rows", "cols", "ldw", "ld16", "prow"))
    dev = "cuda"
    t = lambda a: torch.tensor(a, device=dev)
    sent_f = torch.tensor([SENT], dtype=torch.int32).view(torch.float32).item()
    # item table: w [rows, ldw] with a tail, columns >= cols and the tail are sentinels; g, m, v compact
    W2 = torch.full((rows * ldw + 64,), sent_f, dtype=torch.float32, device=dev)
    W2[:rows * ldw].view(rows, ldw)[:, :cols] = t(x["w2"])
    G2, M2, V2 = t(x["g2"]), t(x["m2"]), t(x["v2"])
    planes = form != "2d"
    eh = torch.full((prow * ld16,), SENT & 0xFFFF, dtype=torch.int16, device=dev)
    el = eh.clone()
    # arena: the gaps between the segments are sentinels in every array
    cover = np.zeros(R.ARENA_N, dtype=bool)
    segs = Segments()
    segs.nseg = len(R.ARENA_SEGS)
    for i, (slot, off, n) in enumerate(R.ARENA_SEGS):
        segs.off[i], segs.len[i], segs.slot[i] = off, n, slot
        cover[off:off + n] = True
    arena = {}
    for k in "wgmv":
        a = x[k].copy()
        a.view(np.int32)[~cover] = SENT
        arena[k] = a
    W, G, M, V = (t(arena[k]) for k in "wgmv")
    sd, sp, use = t(x["sqn_dense"]), t(x["sqn_pieces"]), t(x["use_dense"])
    ids_np = R.a_ids(rows)
    ids = t(ids_np)
    nwords = ((rows + 31) // 32 + 15) // 16 * 16
    bm = torch.zeros(nwords, dtype=torch.int32, device=dev)
    item = (ptr(W2), ldw, ptr(G2), ptr(M2), ptr(V2), rows, cols, R.ITEM_SLOT, ptr(sd), ptr(sp), ptr(use)) + args
    pl = (ptr2(eh), ptr2(el), ld16) if planes else (None, None, 0)
    want_bm = np.zeros(nwords, dtype=np.uint32)
    for r in np.unique(ids_np - 1):
        want_bm[r >> 5] |= np.uint32(1 << (r & 31))
    if form in ("2d", "2d_bf16"):
        assert lib.tcar_clip_adam(ptr(W), ptr(G), ptr(M), ptr(V), C.byref(segs), ptr(sd), ptr(sp), ptr(use), *args, None) == 0
        if planes:
            assert lib.tcar_clip_adam_2d_bf16(*item, *pl, None) == 0
        else:
            assert lib.tcar_clip_adam_2d(*item, None) == 0
    elif form == "all":
        assert lib.tcar_clip_adam_all(ptr(W), ptr(G), ptr(M), ptr(V), C.byref(segs), *item, *pl, None) == 0
    else:
        assert lib.tcar_clip_adam_early(ptr(W), ptr(G), ptr(M), ptr(V), C.byref(segs), *item, *pl, ptr(ids), ids.numel(), ptr(bm), None) == 0
        assert np.array_equal(bm.cpu().numpy().view(np.uint32), want_bm)            # after _early alone: exactly the listed rows
        later = ~np.isin(np.arange(rows), ids_np - 1)                               # ... and the other rows wait for the rest pass
        assert np.array_equal(W2[:rows * ldw].view(rows, ldw)[:, :cols].cpu().numpy()[later].view(np.int32), x["w2"][later].view(np.int32))
        rest = lib.tcar_clip_adam_rest if form == "early_rest" else lib.tcar_clip_adam_rest_keep
        assert rest(*item, *pl, ptr(bm), None) == 0
        got_bm = bm.cpu().numpy().view(np.uint32)
        assert np.array_equal(got_bm, want_bm if form == "early_rest_keep" else np.zeros_like(want_bm))
    torch.cuda.synchronize()
    # ---- m, v, w against float64
    w2 = W2[:rows * ldw].view(rows, ldw)
    fac = R.A_W_FACTOR.get(shape, 1.0)
    r = R.gate_a(w2[:, :cols].cpu().numpy(), M2.cpu().numpy(), V2.cpu().numpy(), ref["item"], fac)
    print(shape, clip, form, "item", r)
    worst = {"item": r}
    Wn, Mn, Vn = W.cpu().numpy(), M.cpu().numpy(), V.cpu().numpy()
    for name, (slot, off, n) in zip("abcd", R.ARENA_SEGS):
        s = slice(off, off + n)
        worst[name] = R.gate_a(Wn[s], Mn[s], Vn[s], ref[name], fac)
        print(shape, clip, form, name, worst[name])
    for name, rr in worst.items():
        assert max(rr.values()) <= 1.0, (name, rr)
    # (c) below the clip: sc = 1 exactly, m and v are the unclipped fp32 formula bit for bit; (d) zero gradient, zero moments: nothing moves
    _, off, n = R.ARENA_SEGS[2]
    assert np.array_equal(Mn[off:off + n].view(np.int32), ref["c32"][1].view(np.int32))
    assert np.array_equal(Vn[off:off + n].view(np.int32), ref["c32"][2].view(np.int32))
    _, off, n = R.ARENA_SEGS[3]
    for got, k in ((Wn, "w"), (Mn, "m"), (Vn, "v")):
        assert np.array_equal(got[off:off + n].view(np.int32), arena[k][off:off + n].view(np.int32)), k
    # ---- nothing else moves
    assert bool((_bits(w2[:, cols:]) == SENT).all()) and bool((_bits(W2[rows * ldw:]) == SENT).all())
    assert torch.equal(_bits(G2), _bits(t(x["g2"]))) and torch.equal(_bits(G), _bits(t(arena["g"])))
    gap = torch.tensor(~cover, device=dev)
    for a in (W, M, V):
        assert bool((_bits(a)[gap] == SENT).all())
    # ---- planes
    if not planes:
        return
    idx = torch.tensor(_kb32_index(prow, ld16), device=dev)
    hi, lo = eh[idx], el[idx]                                                       # logical [prow, ld16]
    wn = w2[:, :cols].contiguous()
    want_hi = wn.to(torch.bfloat16)
    want_lo = (wn - want_hi.float()).to(torch.bfloat16)
    assert torch.equal(hi[:rows, :cols], _bits(want_hi)) and torch.equal(lo[:rows, :cols], _bits(want_lo))
    rec = hi[:rows, :cols].contiguous().view(torch.bfloat16).double() + lo[:rows, :cols].contiguous().view(torch.bfloat16).double()
    assert bool(((rec - wn.double()).abs() <= 2.0 ** -16 * wn.double().abs()).all())
    sent16 = SENT & 0xFFFF
    assert bool((hi[rows:] == sent16).all()) and bool((lo[rows:] == sent16).all())
    assert bool((hi[:, cols:] == sent16).all()) and bool((lo[:, cols:] == sent16).all())


# ------------------------------------------------------------------------------------------------ B: the engines, step by step
def _engine(kind, scoring, s):
    from tcar_amd.engine import TcarEngine
    if kind.startswith("sharded"):
        from tcar_amd.sharded import ShardedEngine
        eng = ShardedEngine(s["params"], s["content"], s["mw"], max_grad=s["max_grad"], scoring=scoring, world=1, rank=0)
        assert eng.can_defer or kind == "sharded"
        return eng
    eng = TcarEngine(s["params"], s["content"], s["mw"], max_grad=s["max_grad"], scoring=scoring)
    if kind == "oplevel":
        eng.native = False
    return eng


ENGINES = [  # case, engine kind, scoring
    ("base", "native", "f32"), ("base", "native", "bf16x3"), ("base", "native", "bf16x3-mixed"),
    ("base", "deferred", "f32"), ("base", "deferred", "bf16x3"), ("base", "deferred", "bf16x3-mixed"),
    ("base", "oplevel", "f32"), ("base", "sharded", "bf16x3-mixed"),
    ("wide", "native", "f32"), ("wide", "native", "bf16x3-mixed"), ("wide", "deferred", "bf16x3-mixed"), ("wide", "sharded", "bf16x3-mixed"),
    # the owed update applied by the NEXT deferred step: early part (arena, the item rows that step gathers, its label rows in the
    # anchored softmax form) on the main stream, the rest pass beside its forward
    ("base", "chained", "f32"), ("base", "chained", "bf16x3-mixed"), ("wide", "chained", "bf16x3-mixed"), ("wide", "sharded_chained", "bf16x3-mixed"),
]


@pytest.mark.parametrize("case,kind,scoring", ENGINES)
def test_engine_update_matches_the_oracle_step_by_step(case, kind, scoring):
    """Teacher-forced: before every step the engine loads the fp32 state the oracle started that step from, so both sides take ONE
    update from identical state and the gates follow from those the suite holds on gradients and clip norms (optim_ref.gate_b).
    Deferred engines owe the update to flush(); the state is read behind it.  `chained`: the owed update is applied by a second deferred
    step on the next batch of the sequence (the split update of the step drivers); the state is read behind that step, whose own
    update — never applied — is dropped before the next load_state.
    Measured on an MI355X, worst error / bound over all steps and variables: f32 m 0.03, v 0.30; bf16x3 m 0.13, v 0.30; bf16x3-mixed
    m 0.12 (0.24 at the gradient-only gate of the unclipped variables), v 0.08; w 0.50 everywhere (the rounding of w itself)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    s = R.b_sequence(case)
    eng = _engine(kind, scoring, s)
    order = s["order"]
    chained = kind.endswith("chained")
    if (case, kind) == ("wide", "chained"):
        # here the step takes the anchored softmax form, whose forward reads the label rows: they join the early part
        form = eng.step_form(eng.upload(s["steps"][1]["batch"]))
        print("step form", form)
        assert form["ce_anchored"]
    for i, st in enumerate(s["steps"]):
        clipped, unclipped = R.clip_census(st["sqn"], s["max_grad"], order)
        assert len(clipped) >= 3 and len(unclipped) >= 3 and "item_emb" in clipped and any(R.is_dense_weight(k) for k in clipped), (i, clipped, unclipped)
        eng.load_state(st["state0"])
        loss = eng.train_step(st["batch"], defer_update=kind == "deferred" or chained)
        close(loss.cpu().numpy(), st["loss"], name="loss of step %d" % i)           # the forward pass behind load_state
        if kind == "deferred":
            assert eng._pending_lr is not None
            eng.flush()
        mid = (int(eng.step), np.asarray([eng.b1_pow, eng.b2_pow], dtype=np.float32))     # the host's count and beta powers behind THIS step
        if chained:
            assert eng._pending_lr is not None
            eng.train_step(s["steps"][(i + 1) % len(s["steps"])]["batch"], defer_update=True)
            torch.cuda.synchronize()
            assert eng._pending_lr is not None and int(eng.adam_bitmap.abs().sum()) == 0
            eng.discard_pending_update()                                            # the probe step's own update is never applied
        got = eng.export_state()
        if not chained:
            mid = (int(got["meta/step"]), got["meta/beta_pow"])
        assert mid[0] == int(st["state1"]["meta/step"]) == i + 1
        assert np.array_equal(mid[1], st["state1"]["meta/beta_pow"])
        # the rate of the step that produced the gradient, as TF computes it from the beta powers that step left
        lr_t = R.lr_t_from_beta_pow(mid[1])
        gmax = max(float(np.abs(g).max()) for g in st["grads"].values())
        bad = []
        for k in order:
            r = R.gate_b(got["m/" + k], got["v/" + k], st["ref"][k], scoring, gmax)
            r["w"] = R.gate_w(got["var/" + k], st["state0"]["var/" + k], got["m/" + k], got["v/" + k], lr_t)
            if k in unclipped:
                r["m_unclipped"] = R.gate_b_unclipped(got["m/" + k], st["ref"][k], scoring, gmax)
            print(case, kind, scoring, "step", i, k, {a: round(b, 4) for a, b in r.items()})
            if max(r.values()) > 1.0:
                bad.append((k, r))
        assert not bad, (i, bad)
    # Derived state left stale — item columns of the planes, time planes, the table itself — shows in the LOGITS of an evaluation
    # (test_optimizer_ref.py: a table one update behind fails this gate; the cross-entropy alone would not at the base size).
    # Behind the last UPDATE the reference is the oracle at the state the engine itself exported (in the mixed precision the engine's
    # own update differs from the oracle's by up to lr per coordinate whose gradient is bf16 noise: not what is asked here); behind
    # load_state it is the oracle at the state both loaded.
    lab = torch.as_tensor(s["eval_batch"]["label"], dtype=torch.long)
    for what, want in (("update", R.eval_reference(s, got)), ("load_state", (s["eval_logits"], s["eval_ce"]))):
        if what == "load_state":
            eng.load_state(s["steps"][-1]["state1"])
        rank, topk, ce, logits = eng.eval_step(s["eval_batch"], keep_logits=True)
        close(logits.cpu().numpy(), want[0], name="eval logits behind " + what)
        close(ce.cpu().numpy(), want[1], name="eval ce behind " + what)
        lg = logits.cpu().double()
        assert (rank.cpu().numpy() == ((lg > lg.gather(1, lab[:, None])).sum(1).numpy() + 1)).all()
        _planes_follow_master(eng)


def _planes_follow_master(eng):
    """the item columns of the bf16 planes are the split of the fp32 master, exactly (the one-rank sharded engine evaluates on the
    fp32 GEMM, which reads no plane; the time columns are rebuilt by whoever reads them next)"""
    if not eng.scoring_code:
        return
    g = eng.geo
    idx = torch.tensor(_kb32_index(eng.e16h.shape[0], g.ek), device=eng.dev)[:g.N, :g.H]
    w = eng.E[:g.N, :g.H].contiguous()
    hi = w.to(torch.bfloat16)
    lo = (w - hi.float()).to(torch.bfloat16)
    assert torch.equal(_bits(eng.e16h).flatten()[idx], _bits(hi)) and torch.equal(_bits(eng.e16l).flatten()[idx], _bits(lo))
