"""Reference arithmetic and gates of the optimizer tests (test_optimizer_ref.py on the CPU, test_gpu_optimizer.py on the GPU).

The update is model_combine.py:155-163 as csrc/optim.hip's header states it:
    n2 = use_dense[slot] * sqn_dense[slot] + sqn_pieces[slot];  sc = clip / max(sqrt(n2), clip)  (clip <= 0: sc = 1)
    gc = g * sc;  m = b1 m0 + (1 - b1) gc;  v = b2 v0 + (1 - b2) gc^2;  w = w0 - lr_t m / (sqrt(v) + eps)
`adam64` is that formula in numpy float64, `adam32` the same in float32 in the operation order of the kernels (adam1 / clip_factor
of optim.hip: every operation rounded once, the two multiply-adds fused).  The gates are functions, so that the CPU test can show
what they reject (a wrong clip) and what they admit (a correct fp32 implementation) on the very inputs the GPU tests use.
"""
from collections import OrderedDict

import numpy as np

from step_cases import _case

NSLOT = 32
B1, B2, EPS, LR = 0.9, 0.999, 1e-8, 1e-3
F = np.float32
# `wrong` of clip_scale: the three mistakes the tests must be able to tell from the right clip
WRONG_CLIPS = ("off", "dense_only", "neighbour")


def adam_args(step, clip):
    """(clip, lr_t, b1, b2, eps) of update number `step` + 1, as the engines compute them: fp32 beta powers multiplied once per step,
    lr_t in fp32; every value is the float the C ABI receives."""
    b1p, b2p = F(B1), F(B2)
    for _ in range(step):
        b1p, b2p = F(b1p * F(B1)), F(b2p * F(B2))
    lr_t = F(LR) * np.sqrt(F(1) - b2p) / (F(1) - b1p)
    return tuple(float(F(x)) for x in (clip, lr_t, B1, B2, EPS))


def lr_t_from_beta_pow(beta_pow_after, lr=LR):
    """TF's bias-corrected rate of the update that LEFT the beta powers at `beta_pow_after` (they are multiplied after the update)."""
    b1p, b2p = F(beta_pow_after[0]) / F(B1), F(beta_pow_after[1]) / F(B2)
    return float(F(lr) * np.sqrt(F(1) - F(b2p)) / (F(1) - F(b1p)))


def clip_scale(sqn_dense, sqn_pieces, use_dense, slot, clip, wrong=None, dtype=np.float64):
    """sc of one variable; dtype float32 follows clip_factor's operation order.  wrong: None | one of WRONG_CLIPS."""
    if wrong == "neighbour":
        slot = (slot + 1) % len(sqn_dense)
    if clip <= 0 or wrong == "off":
        return dtype(1)
    d, p = dtype(sqn_dense[slot]), dtype(sqn_pieces[slot])
    n2 = d if wrong == "dense_only" else (d if use_dense[slot] else dtype(0)) + p
    return dtype(clip) / np.maximum(np.sqrt(dtype(n2)), dtype(clip))


def adam64(w0, g, m0, v0, sc, args):
    """-> dict of float64 arrays: w, m, v and the magnitudes the bounds are stated in"""
    _, lr_t, b1, b2, eps = args
    w0, g, m0, v0 = (np.asarray(a, dtype=np.float64) for a in (w0, g, m0, v0))
    gc = g * float(sc)
    a, b = b1 * m0, (1 - b1) * gc
    c, d = b2 * v0, (1 - b2) * gc * gc
    m, v = a + b, c + d
    upd = lr_t * m / (np.sqrt(v) + eps)
    return {"w": w0 - upd, "m": m, "v": v, "m_mag": np.abs(a) + np.abs(b), "v_mag": c + d, "w0": np.abs(w0), "upd": np.abs(upd), "gc": gc}


def _fma32(a, b, c):
    """fp32 fused multiply-add: the product of two floats is exact in float64; one more rounding of the float64 sum (a double
    rounding that differs from the fused one about once in 2^29 operations)"""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F)


def adam32(w0, g, m0, v0, sc, args):
    """adam1 of optim.hip in numpy float32 -> (w, m, v)"""
    _, lr_t, b1, b2, eps = (F(x) for x in args)
    w0, g, m0, v0 = (np.asarray(a, dtype=F) for a in (w0, g, m0, v0))
    gx = g * F(sc)
    m = _fma32(b1, m0, (F(1) - b1) * gx)
    v = _fma32(b2, v0, ((F(1) - b2) * gx) * gx)
    w = w0 - (lr_t * m) / (np.sqrt(v) + eps)
    return w, m, v


# ---- gates of part A: one rounding of 2^-24 per fp32 operation, counted ------------------------------------------------------
A_M, A_V, A_W0, A_UPD = 2.0 ** -21, 2.0 ** -21, 2.0 ** -23, 2.0 ** -20
# w's bound is stated in |update|, so it does not cover an m that cancels (b1 m0 = -(1 - b1) gc to a few digits) beside a small w0.  Among
# the 16.8 M elements of the largest shape such elements exist: the float32 restatement needs 1.46 times the bound there (clip = 0), so
# that shape takes twice that; the other shapes hold the bound as stated (test_optimizer_ref.py measures all of them)
A_W_FACTOR = {"strided_walk": 2 * 1.46}


def gate_a(got_w, got_m, got_v, ref, w_factor=1.0):
    """worst ratio error / bound of m, v, w against adam64's result (<= 1 passes); a zero bound admits a zero error only"""
    out = OrderedDict()
    for name, got, bound in (("m", got_m, A_M * ref["m_mag"]), ("v", got_v, A_V * ref["v_mag"]),
                             ("w", got_w, w_factor * (A_W0 * ref["w0"] + A_UPD * ref["upd"]))):
        err = np.abs(np.asarray(got, dtype=np.float64) - ref[name])
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, 0.0, err / bound)
        out[name] = float(r.max()) if r.size else 0.0
    return out


# ---- gates of part B: derived from the gates the suite already holds on gradients and clip norms --------------------------------
def step_reference(grads, sqn, state0, max_grad, wrong=None, dense_sqn=None, order=None):
    """float64 Adam targets of ONE step from the (fp32) state `state0` for the oracle's gradients and clip norms.
    wrong: the clip mistakes above — `dense_only` takes `dense_sqn` (the dense block alone, the pieces dropped), `neighbour` the next variable's."""
    names = list(order or grads.keys())
    ref = OrderedDict()
    for i, k in enumerate(names):
        kk = names[(i + 1) % len(names)] if wrong == "neighbour" else k
        n2 = dense_sqn[kk] if wrong == "dense_only" else sqn[kk]
        sc = 1.0 if (wrong == "off" or not max_grad) else max_grad / max(np.sqrt(n2), max_grad)
        g = np.asarray(grads[k], dtype=np.float64)
        m0, v0 = (np.asarray(state0[t + k], dtype=np.float64).reshape(g.shape) for t in ("m/", "v/"))
        gc = g * sc
        ref[k] = {"gc": gc, "sc": sc, "m": B1 * m0 + (1 - B1) * gc, "v": B2 * v0 + (1 - B2) * gc * gc, "bm0": np.abs(B1 * m0), "bv0": B2 * v0}
    return ref


def gate_b(got_m, got_v, r, scoring, gmax):
    """worst ratio error / bound of one variable's moments against step_reference's entry `r` (<= 1 passes).
    f32, bf16x3 — element-wise: gradients hold rtol 1e-3 + 5e-5 of the variable's largest and sc 1e-3, so gc holds 2e-3 + 5e-5 max.
    bf16x3-mixed — norm-wise: gradients 1e-2 and sc 1e-2, so gc 2e-2, with check_grads' floor 1e-7 gmax sqrt(size) on the gradient.
    Both carry the fp32 rounding of the loaded terms b1 m0, b2 v0 (2^-22 of their magnitude)."""
    gc = r["gc"]
    gm = float(np.abs(gc).max()) if gc.size else 0.0
    dm = np.abs(np.asarray(got_m, dtype=np.float64).reshape(gc.shape) - r["m"])
    dv = np.abs(np.asarray(got_v, dtype=np.float64).reshape(gc.shape) - r["v"])
    if scoring == "bf16x3-mixed":
        floor = 1e-7 * gmax * np.sqrt(gc.size)
        bm = (1 - B1) * (2e-2 * np.linalg.norm(gc) + floor) + 2.0 ** -22 * np.linalg.norm(r["bm0"])
        bv = (1 - B2) * (4e-2 * np.linalg.norm(gc * gc) + 2 * gm * floor) + 2.0 ** -22 * np.linalg.norm(r["bv0"])
        return {"m": _ratio(np.linalg.norm(dm), bm), "v": _ratio(np.linalg.norm(dv), bv)}
    dg = 2e-3 * np.abs(gc) + 5e-5 * gm
    bm = (1 - B1) * dg + 2.0 ** -22 * r["bm0"]
    bv = (1 - B2) * 2 * np.abs(gc) * dg + 2.0 ** -22 * r["bv0"]
    return {"m": _ratio(dm, bm), "v": _ratio(dv, bv)}


def gate_b_unclipped(got_m, r, scoring, gmax):
    """a variable below the clip has sc = 1 on both sides: its m obeys the GRADIENT gate alone (1e-3 + 5e-5 max; 1e-2 norm-wise)"""
    gc = r["gc"]
    gm = float(np.abs(gc).max()) if gc.size else 0.0
    dm = np.abs(np.asarray(got_m, dtype=np.float64).reshape(gc.shape) - r["m"])
    if scoring == "bf16x3-mixed":
        b = (1 - B1) * (1e-2 * np.linalg.norm(gc) + 1e-7 * gmax * np.sqrt(gc.size)) + 2.0 ** -22 * np.linalg.norm(r["bm0"])
        return _ratio(np.linalg.norm(dm), b)
    return _ratio(dm, (1 - B1) * (1e-3 * np.abs(gc) + 5e-5 * gm) + 2.0 ** -22 * r["bm0"])


def gate_w(got_w, w0, got_m, got_v, lr_t):
    """w against w0 - lr_t m / (sqrt(v) + eps) in float64 from the implementation's OWN m, v, within part A's bound for w"""
    w0, m, v = (np.asarray(a, dtype=np.float64) for a in (w0, got_m, got_v))
    upd = lr_t * m / (np.sqrt(v) + EPS)
    return _ratio(np.abs(np.asarray(got_w, dtype=np.float64) - (w0 - upd)), A_W0 * np.abs(w0) + A_UPD * np.abs(upd))


def _ratio(err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


def is_dense_weight(name):
    """a weight matrix or residual weight (no table, no bias): its clip norm is the dense norm alone"""
    return name.endswith("/w1") or name.endswith("w_3d")


def clip_census(sqn, max_grad, order):
    """(clipped, unclipped) variable names: sqrt(sqn) beyond 1.25 max_grad / below 0.8 max_grad; the band between is not counted"""
    n = {k: float(np.sqrt(sqn[k])) for k in order}
    return [k for k in order if n[k] > 1.25 * max_grad], [k for k in order if n[k] < 0.8 * max_grad]


# ---- inputs of part A (seeded; the same arrays on the CPU and on the GPU) ------------------------------------------------------
ITEM_SLOT = 0
# (slot, offset, length) of the four arena segments, gaps between them; states (a) dense clip, (b) pieces only, (c) below, (d) zero
ARENA_SEGS = ((3, 8, 4), (7, 20, 1000), (12, 1032, 4096 + 4), (20, 5200, 3 * 4096))
ARENA_N = 5200 + 3 * 4096 + 16
A_SHAPES = {"rows131": (131, 256, 832, 832, 256), "one_row": (1, 4, 8, 32, 128), "strided_walk": (65536 + 131, 256, 256, 256, 65536 + 256)}
A_CLIP = 2.0
A_STEP = 6            # the seventh update: lr_t != lr


def a_ids(rows):
    """1-based ids of the split forms: repeats, id 1, id rows, ids sharing a bitmap word (33..64 are rows 32..63 of word 1)"""
    ids = [5, 5, 5, 1, rows, 40, 41, 41, 64, 65, 130, 131, rows, 1]
    return np.asarray([min(max(i, 1), rows) for i in ids], dtype=np.int32)


def a_inputs(shape, seed=11):
    """dict of the fp32 inputs of one part-A run: item table (w2 [rows, ldw], g2 / m2 / v2 [rows, cols]), arena (w, g, m, v [ARENA_N]),
    sqn_dense / sqn_pieces / use_dense [NSLOT].  Untouched regions are left to the caller's sentinel."""
    rows, cols, ldw, ld16, prow = A_SHAPES[shape]
    rng = np.random.RandomState(seed)
    x = {"rows": rows, "cols": cols, "ldw": ldw, "ld16": ld16, "prow": prow}
    x["w2"] = rng.standard_normal((rows, cols)).astype(F)
    x["g2"] = (rng.standard_normal((rows, cols)) * 0.1).astype(F)
    x["m2"] = (rng.standard_normal((rows, cols)) * 0.01).astype(F)
    x["v2"] = (rng.rand(rows, cols) * 1e-3 + 1e-6).astype(F)
    x["w"] = rng.standard_normal(ARENA_N).astype(F)
    x["g"] = (rng.standard_normal(ARENA_N) * 0.1).astype(F)
    x["m"] = (rng.standard_normal(ARENA_N) * 0.01).astype(F)
    x["v"] = (rng.rand(ARENA_N) * 1e-3 + 1e-6).astype(F)
    # every slot gets a norm of its own (a neighbour's factor is never the right one): sqrt(n2) between 3 and 35 for slot != segments
    sd = (9.0 + 37.0 * np.arange(NSLOT)).astype(F)
    sp = np.zeros(NSLOT, dtype=F)
    use = np.ones(NSLOT, dtype=np.int32)
    sd[ITEM_SLOT], sp[ITEM_SLOT] = 30.0, 51.0                  # item table: dense norm AND pieces, sqrt(81) = 9 > clip
    (sa, oa, la), (sb, ob, lb), (sc_, oc, lc), (sz, oz, lz) = ARENA_SEGS
    sd[sa], sp[sa] = 25.0, 0.0                                 # (a) clipped by the dense norm: sc = 2 / 5
    sd[sb], sp[sb], use[sb] = 1e30, 64.0, 0                    # (b) the pieces alone count: sc = 2 / 8; the dense slot must be ignored
    sd[sc_], sp[sc_] = 1.0, 0.44                               # (c) sqrt(1.44) = 1.2 below the clip: sc = 1 exactly
    sd[sz], sp[sz] = 0.0, 0.0                                  # (d) all-zero gradient, zero moments
    x["g"][oz:oz + lz] = 0
    x["m"][oz:oz + lz] = 0
    x["v"][oz:oz + lz] = 0
    x["sqn_dense"], x["sqn_pieces"], x["use_dense"] = sd, sp, use
    return x


# ---- the teacher-forced step sequences of part B (oracle side; computed once per process) ---------------------------------------
# name -> (N, H, Ht, K, parameter seed, max_grad, [(B, T, batch seed, tweak)]).  The clip census (clip_census) holds in every step:
#  * A single session clips the item table at max_grad 2 only when it is short: norm 3.1 at T = 2 with this seed, 1.9 at T = 5, 1.2 at
#    T = 12.  So the B = 1 step has T = 2.
#  * T = 1 is left out: the gradients through the exp-normaliser of a length-1 session are below fp32 resolution.  gpu_util.close
#    has an absolute floor of 1e-9 for them; the gates here have none.
#  * The lone session clicks two DIFFERENT items (tweak "distinct"; _case would repeat the first).  With one item clicked twice the two
#    positions differ by dec_pos only, and the attention weights' gradients are differences of nearly equal terms: the split-bf16 modes'
#    noise in the forward pass then puts them outside the gradient gate.  That is no property of the update: the batch itself is held to
#    the oracle by test_gpu_fused_step.py (case `lone_twice`, at a gate with a cancellation floor derived from the oracle: fused_ref.py).
#  * The wide case runs at max_grad 4: its 64-session steps leave two variables below 0.8 * 2, but seven below 0.8 * 4.
B_CASES = {
    "base": (300, 40, 16, 4, 5, 2.0, [(24, 3, 5, None), (24, 2, 6, "label"), (1, 2, 53, "distinct"), (40, 7, 8, None)]),
    "wide": (1000, 250, 64, 4, 9, 4.0, [(64, 7, 9, None), (64, 2, 10, "label")]),
}
_SEQ = {}


def b_sequence(name):
    """-> dict(params, content, mw, steps); steps[i] = dict(batch, state0 (fp32 state both sides load), state1 (the oracle's fp32
    state after the step), grads, sqn, dense_sqn, ref (step_reference), loss).  Every step starts from the fp32-rounded state the
    oracle reached, so an implementation that loads state0 and takes the step is compared over ONE update."""
    if name in _SEQ:
        return _SEQ[name]
    from oracle.tcar_oracle import TABLES, TcarOracle
    N, H, Ht, K, pseed, max_grad, plan = B_CASES[name]
    params, content, mw, _ = _case(N, H, Ht, plan[0][0], plan[0][1], K, seed=pseed)
    ora = TcarOracle(params, content, mw, max_grad=max_grad)
    steps = []
    for B, T, seed, tweak in plan:
        batch = _case(N, H, Ht, B, T, K, seed=seed)[3]
        if tweak == "label":
            batch["label"][1] = batch["label"][0]            # two sessions with one label (_case repeats an item id in every batch)
        if tweak == "distinct":
            # ... but a lone session of one item clicked twice leaves the attention weights' gradients as differences of nearly
            # equal terms (the two positions differ by dec_pos only): rounding noise of the forward pass, not a property of the update
            batch["seq"][0, 1] = batch["seq"][0, 0] % N + 1
        state0 = ora.export_state()
        ora.load_state(state0)
        out, grads, sqn = ora.loss_and_grads(batch)
        ora.apply_adam(grads, sqn)
        grads = OrderedDict((k, v.numpy().copy()) for k, v in grads.items())
        # what sqn_dense holds in the engines: the dense [1:] block of the item gradient WITHOUT the gathered rows' pieces, nothing for
        # the gathered tables (use_dense = 0), the whole norm for the dense weights
        blk = out["_vals"]["item_emb"][-1].grad
        dense_sqn = {k: float((blk * blk).sum()) if k == "item_emb" else (0.0 if k in TABLES else sqn[k]) for k in grads}
        steps.append({"batch": batch, "state0": state0, "state1": ora.export_state(), "grads": grads, "sqn": dict(sqn), "dense_sqn": dense_sqn,
                      "ref": step_reference(grads, sqn, state0, max_grad), "loss": out["loss"].detach().numpy().copy()})
    _, _, _, fresh = _case(N, H, Ht, 9, 4, K, seed=99)
    _SEQ[name] = {"params": params, "content": content, "mw": mw, "steps": steps, "eval_batch": fresh, "order": list(grads.keys()), "max_grad": max_grad}
    _SEQ[name]["eval_logits"], _SEQ[name]["eval_ce"] = eval_reference(_SEQ[name], steps[-1]["state1"])
    return _SEQ[name]


def eval_reference(s, state):
    """(logits [B, N], ce [B]) of the sequence's evaluation batch by an oracle that holds `state`"""
    from oracle.tcar_oracle import TcarOracle
    ora = TcarOracle(s["params"], s["content"], s["mw"], max_grad=s["max_grad"])
    ora.load_state(state)
    logits, ce = ora.eval_batch(s["eval_batch"])
    return logits.numpy(), ce.numpy()
