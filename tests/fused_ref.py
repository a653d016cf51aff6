"""Cases, batch builders, fp64 references and gates of the fused-step tests (test_fused_step_ref.py on the CPU, test_gpu_fused_step.py on
the GPU).

The fused training step (tcar_train_step / tcar_train_step_deferred: softmax epilogue, anchored fold, one-hot dX / dE, (q, z) pairs,
in-launch slab folds) leaves its own gradients; `loss_and_grads` takes another path (materialised logits).  Every case here is a model
and TWO batches: the first step starts at the initial parameters (its oracle run is cached and shared by the three precisions), the
second is teacher-forced from the parameters the engine exported behind its own update.

The gates are those the suite already holds on gradients (step_cases.check_grads: rtol 1e-3 + 5e-5 of the variable's largest,
clip norms 2e-3; bf16x3-mixed 1e-2 norm-wise, large elements within 10 %, clip norms 2e-2) restated as ratios error / bound so that a
test can print them, plus two things defined from the same constants:
  * a ROW-WISE check of item_emb (`item_row_ratio`): every row whose oracle norm is >= MIXED_BIG_FRAC of the largest holds the
    precision's gradient gate norm-wise (1e-2 mixed, 1e-3 otherwise).  A label row is dominated by its own session's
    (p - 1) attout_b, so a lost session is a 100 % error of one row — which the norm-wise mixed gate alone lets through at B = 513
    (one session is about 1 / sqrt(B) of the norm);
  * the cancellation floor of the lone session that clicks one item twice (`floors`, case `lone_twice` only): the absolute term
    of the gate is stated on max(max |want|, max A), A = |x|^T |dy| the fp64 sum of the MAGNITUDES of the per-row terms of a weight used
    as x @ W — the standard forward bound of a sum whose terms each carry the operand rounding.
Two more places state a bound on an oracle-side quantity, both where the exact gradient is (next to) zero and an implementation returns
the rounding of what cancels:
  * every item on ONE publish time (`time_lo`, `time_hi`): the variables of TIME_PATH take their scale from the gradient of
    sum |dlogits| logits — the contraction over the catalog with magnitudes summed (`cat_floors`);
  * a variable entirely below 2^-24 of the step's largest gradient may be exact zeros in f32 / bf16x3 (`below_fp32`).
"""
from collections import OrderedDict

import numpy as np

from step_cases import CASES, MIXED_BIG_FRAC, MIXED_BIG_RTOL, MIXED_GRAD_RTOL, MIXED_SQNORM_RTOL, _case, check_grads

SCORINGS = ("f32", "bf16x3", "bf16x3-mixed")
MAX_GRAD = 2.0
GRAD_RTOL, GRAD_ATOL = 1e-3, 5e-5            # gpu_util.close as step_cases.check_grads calls it
SQN_RTOL = 2e-3
# the five weights used as x @ W in the attention layers: name -> (x, dy) keys of the oracle's forward
XW = OrderedDict([
    ("multi_attention/input_linear_trans/w_3d", ("seq_ic", "pre1")), ("multi_attention/cont_linear_trans/w_3d", ("seq_content", "pre1")),
    ("multi_attention/inter_linear_trans/w_3d", ("seq_act", "pre1")), ("cont_attention/input_linear_trans/w_3d", ("seq_pt", "pre2")),
    ("cont_attention/cont_linear_trans/w_3d", ("seq_content", "pre2"))])
CANCEL_VAR, CANCEL_MIN = "multi_attention/cont_linear_trans/w_3d", 50.0
# everything behind attout's time half and the candidate-side time columns: where every item has ONE publish time these columns are
# the same for every candidate, the softmax does not see them, and the exact gradient of all of these is ZERO (the oracle's fp64 leaves
# 1e-16) — except the click-time part of week / hour
TIME_PATH = ("month_embedding", "day_embedding", "week_embedding", "hour_embedding", "minute_embedding", "attout_pt_trans/w1",
             "attout_pt_trans/b1", "cont_attention/input_linear_trans/w_3d", "cont_attention/cont_linear_trans/w_3d",
             "cont_attention/res_linear_trans/w_3d")
PLANT_TABLE = "month_embedding"               # plant (d): this table's candidate-side gather without the clip Jacobian


# ---- the case table ------------------------------------------------------------------------------------------------------------
# name -> dict(N, H, Ht, pseed, steps = [(B, T, K, batch seed)] * 2, tweaks = (...), tuning = {TCAR_*: value},
#              both = also through loss_and_grads, floor = the cancellation floor applies, regime = (sign, s, lo, hi, what))
def _mk(N, H, Ht, pseed, steps, tweaks=(), tuning=None, both=False, floor=None, regime=None, mw=None, lr=1e-3):
    return dict(N=N, H=H, Ht=Ht, pseed=pseed, steps=steps, tweaks=tuple(tweaks), tuning=dict(tuning or {}), both=both, floor=floor,
                regime=regime, mw=mw, lr=lr)


def _cases():
    c = OrderedDict()
    # A. the eight shapes of test_step_matches_oracle (same seeds), then the next shape's batch at the same model
    for i, (N, H, Ht, B, T, K) in enumerate(CASES):
        _, _, _, B2, T2, K2 = CASES[(i + 1) % len(CASES)]
        s = N + H + B + T
        c["parity%d" % i] = _mk(N, H, Ht, s, [(B, T, K, s), (B2, T2, K2, s + 1)], tweaks=("tail_label",))
    small = (300, 40, 16)
    # straddles of the driver's thresholds (csrc/step.hip): TCAR_PROJ_SPLIT_ROWS = 1,024 rows B * T; the small-table chunk fold from
    # 2,048 rows; the 128-row plane block; a small batch behind a large one on the same engine (stale padding rows)
    c["rows1024_1028"] = _mk(*small, 21, [(256, 4, 4, 21), (257, 4, 4, 22)], tweaks=("tail_label",))
    c["rows1028_1024"] = _mk(*small, 23, [(257, 4, 4, 23), (256, 4, 4, 24)], tweaks=("tail_label",))
    c["rows2044_2048"] = _mk(*small, 25, [(511, 4, 4, 25), (512, 4, 4, 26)], tweaks=("tail_label",))
    c["rows2048_2044"] = _mk(*small, 27, [(512, 4, 4, 27), (511, 4, 4, 28)], tweaks=("tail_label",))
    c["b128_129"] = _mk(*small, 29, [(128, 2, 4, 29), (129, 2, 4, 30)], tweaks=("tail_label",))
    c["b129_128"] = _mk(*small, 31, [(129, 2, 4, 31), (128, 2, 4, 32)], tweaks=("tail_label",))
    c["b512_then_5"] = _mk(*small, 33, [(512, 2, 4, 33), (5, 2, 4, 34)], tweaks=("tail_label",))
    # catalog edges: first / last column of a ragged catalog in label, negatives and clicks
    for N in (7, 127, 128, 129, 384, 385):
        c["catalog%d" % N] = _mk(N, 40, 16, 40 + N, [(9, 3, 4, 40 + N), (9, 3, 4, 41 + N)], tweaks=("edges",))
    # K: none, one, a full 32-group, one past it; the second step takes the next K
    ks = (0, 1, 32, 33)
    for i, K in enumerate(ks):
        c["k%d" % K] = _mk(*small, 50 + K, [(9, 3, K, 50 + K), (9, 3, ks[(i + 1) % 4], 51 + K)])
    # forms (expected_form): 2 ldh / 64 > TCAR_ANCHOR_COLS = 8 needs ldh = 320, the smallest H for it is 257; ldt is 64 for every Ht
    # the engine accepts (5 ldt <= 512), so the forms without the one-hot backward are reachable by switch only
    c["form_ldh320"] = _mk(129, 257, 16, 61, [(9, 3, 4, 61), (5, 2, 4, 62)])
    # ldh = 128 (H = 100): like ldh = 320 a width at which ldh + 320 is no multiple of the dE tile's 192 columns (64 and 256, the widths
    # of every other case, are) — the ragged last N tile of the (q, z) epilogue
    c["ldh128"] = _mk(129, 100, 16, 59, [(9, 3, 4, 59), (5, 2, 4, 60)])
    c["form_rescale"] = _mk(*small, 63, [(9, 3, 4, 63), (5, 2, 4, 64)], tuning={"TCAR_FUSED_CE": 1})
    c["form_onehot_fwd_only"] = _mk(*small, 65, [(9, 3, 4, 65), (5, 2, 4, 66)], tuning={"TCAR_ONEHOT_TIME": 1})
    c["form_no_onehot"] = _mk(*small, 67, [(9, 3, 4, 67), (5, 2, 4, 68)], tuning={"TCAR_ONEHOT_TIME": 0})
    c["form_unsorted"] = _mk(*small, 69, [(9, 3, 4, 69), (5, 2, 4, 70)], tuning={"TCAR_SORT_SCATTER": 0})
    # B. degenerate batches
    c["lone_twice"] = _mk(*small, 7, [(1, 2, 4, 7), (1, 2, 4, 8)], both=True, floor="lone")
    c["copies130"] = _mk(*small, 71, [(1, 3, 4, 71), (1, 3, 4, 72)], tweaks=("copies130",), both=True)
    c["collisions"] = _mk(*small, 73, [(9, 3, 4, 73), (9, 3, 4, 74)], tweaks=("collisions",), both=True)
    c["time_lo"] = _mk(*small, 75, [(9, 3, 4, 75), (9, 3, 4, 76)], tweaks=("time_extremes",), both=True, mw=(1, 1, 1, 1, 1), floor="catalog")
    c["time_hi"] = _mk(*small, 77, [(9, 3, 4, 77), (9, 3, 4, 78)], tweaks=("time_extremes",), both=True, mw=(12, 31, 7, 24, 60), floor="catalog")
    # softmax regimes: attout_item_cont_trans/b1 = sign * s * sign([item_emb[18] | content[18]]), every label 17, no negatives
    reg = lambda N, H, Ht, sign, s, lo, hi, what: _mk(N, H, Ht, 11, [(5, 3, 0, 11), (5, 3, 0, 12)], tweaks=("label17",), both=True,
                                                      regime=(sign, s, lo, hi, what))
    c["converged"] = reg(*small, +1, 0.5, 0.98, 0.9995, "p")
    c["half"] = reg(*small, +1, 0.25, 0.5, 0.9, "p")
    c["buried"] = reg(*small, -1, 1.0, 30.0, 60.0, "ce")
    c["buried_wide"] = reg(1000, 250, 64, -1, 0.25, 30.0, 60.0, "ce")
    c["converged_wide"] = reg(1000, 250, 64, +1, CONVERGED_WIDE_S, 0.98, 0.9995, "p")
    c["converged_wide"]["tweaks"] += ("shared_clicks",)
    # one update at lr 1e-3 moves 500 coordinates of attout's bias path at once: p goes to 1 - 2e-6, far past the upper bound of the
    # band (fp32's own e_l - S cancellation).  At 3e-5 the second step stays inside (0.9962 to 0.9990); the other regimes stay at 1e-3
    c["converged_wide"]["lr"] = 3e-5
    return c


# Searched on the CPU (test_fused_step_ref.py asserts the band).  At H = 250 the sessions of a random batch spread too far for ANY s
# (s = 0.08: p from 0.65 to 0.998; s = 0.09: 0.90 to 0.9996, past the upper bound), so the ten sessions of this case click the same
# three items (`shared_clicks`; times, dwell and click hour still differ): s = 0.09 then gives 0.9897 to 0.9988
CONVERGED_WIDE_S = 0.09
_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _cases()
    return _CASES


def case_names():
    return list(cases())


def expected_form(scoring, spec):
    """The form csrc/step.hip's predicates give for this case on a single-GPU engine with its default streams (fused_ce, onehot_fwd,
    onehot_bwd, sorted_rows, ce_anchored), from the engine's padding rule ldh = roundup(H, 64) and the case's switches."""
    t = {"TCAR_FUSED_CE": 2, "TCAR_ONEHOT_TIME": 2, "TCAR_SORT_SCATTER": 1, "TCAR_DET_SMALL": 1}
    t.update(spec["tuning"])
    ldh = -(-spec["H"] // 64) * 64
    fused = scoring == "bf16x3-mixed" and t["TCAR_FUSED_CE"] != 0
    srt = t["TCAR_SORT_SCATTER"] != 0 and ldh <= 512
    oh = fused and t["TCAR_ONEHOT_TIME"] != 0
    ohb = oh and t["TCAR_ONEHOT_TIME"] >= 2 and srt and t["TCAR_DET_SMALL"] != 0          # ldt == 64 always
    anch = ohb and t["TCAR_FUSED_CE"] >= 2 and 2 * ldh // 64 <= 8
    return {"fused_ce": fused, "onehot_fwd": oh, "onehot_bwd": ohb, "sorted_rows": srt, "ce_anchored": anch}


# ---- builders ------------------------------------------------------------------------------------------------------------------
def _tweak(b, N, tweaks, B, T, K):
    for t in tweaks:
        if t == "tail_label":
            # the tail session and session 0 own their label rows: no other session's label, no negative, so dropping either session
            # is a 100 % error of one item row in every shape
            if B > 1:
                used = set(b["label"][1:-1].tolist()) | set(np.asarray(b["neg"]).reshape(-1).tolist())
                free = [n for n in range(N) if n not in used]
                if len(free) >= 2:
                    b["label"][0], b["label"][-1] = free[0], free[-1]
        elif t == "edges":
            b["label"][0], b["label"][-1] = 0, N - 1
            b["neg"][1, 0], b["neg"][-2, -1] = 0, N - 1
            b["seq"][2, 0], b["seq"][-1, -1] = 1, N
        elif t == "copies130":
            for k in b:
                b[k] = np.repeat(b[k], 130, axis=0)
        elif t == "collisions":
            b["label"][1] = b["label"][0]                         # two sessions sharing a label
            b["seq"][:, 0] = b["label"] + 1                       # the label among the session's own clicks
            b["neg"][:, 0] = b["label"]                           # ... and among its negatives
            b["neg"][2, :] = b["label"][2]                        # one id K times: the label itself ...
            b["neg"][3, :] = b["neg"][3, 1]                       # ... and another item
        elif t == "time_extremes":
            lo = {"pm": 1, "pd": 1, "pw": 1, "ph": 1, "pmi": 1, "cw": 0, "ch": 0}
            hi = {"pm": 12, "pd": 31, "pw": 7, "ph": 24, "pmi": 60, "cw": 6, "ch": 23}
            for k in lo:
                b[k][0::2] = lo[k]
                b[k][1::2] = hi[k]
            b["gap"][:] = np.asarray([0, 10, 11], dtype=np.int32)[np.arange(B * T).reshape(B, T) % 3]
        elif t == "label17":
            b["label"][:] = 17
    return b


_BUILT = {}


def build(name):
    """-> dict(spec, params, content, mw, batches [2])"""
    if name in _BUILT:
        return _BUILT[name]
    spec = cases()[name]
    N, H, Ht = spec["N"], spec["H"], spec["Ht"]
    (B, T, K, seed), (B2, T2, K2, seed2) = spec["steps"]
    params, content, mw, b1 = _case(N, H, Ht, B, T, K, seed=spec["pseed"])
    if seed != spec["pseed"]:
        b1 = _case(N, H, Ht, B, T, K, seed=seed)[3]
    b2 = _case(N, H, Ht, B2, T2, K2, seed=seed2)[3]
    mult = 130 if "copies130" in spec["tweaks"] else 1
    batches = [_tweak(b1, N, spec["tweaks"], B * mult, T, K), _tweak(b2, N, spec["tweaks"], B2 * mult, T2, K2)]
    if "shared_clicks" in spec["tweaks"]:
        batches[0]["seq"][:] = batches[0]["seq"][0]
        batches[1]["seq"][:] = batches[0]["seq"][0]
    if spec["mw"] is not None:
        mw = np.tile(np.asarray(spec["mw"], dtype=np.int32), (N, 1))
    if spec["regime"] is not None:
        sign, s = spec["regime"][:2]
        row = np.concatenate([params["item_emb"][18], content[18]])
        params["attout_item_cont_trans/b1"] = (sign * s * np.sign(row)).astype(np.float32)
    _BUILT[name] = dict(spec=spec, params=params, content=content, mw=mw, batches=batches)
    return _BUILT[name]


# ---- references ----------------------------------------------------------------------------------------------------------------
def reference(params, content, mw, batch, straight_through=()):
    """One fp64 oracle run -> dict(loss [B], grads, sqn, and what the plants and the floors need).
    floors: max A of the five x @ W weights (XW).  cat_floors: for TIME_PATH, |gradient| of sum_bn |dlogits[b, n]| logits[b, n] — the
    gradient with the contraction over the CATALOG summing magnitudes: what the rounding of that contraction's terms is relative to."""
    import torch
    from oracle.tcar_oracle import TcarOracle
    ora = TcarOracle(params, content, mw, max_grad=MAX_GRAD, straight_through=straight_through)
    out, grads, sqn = ora.loss_and_grads(batch)
    H = ora.H
    r = {"loss": out["loss"].detach().numpy().copy(), "grads": OrderedDict((k, v.numpy().copy()) for k, v in grads.items()), "sqn": dict(sqn),
         "ce": out["ce"].detach().numpy().copy(), "attout_item": out["attout"].detach().numpy()[:, :H].copy(),
         "seq_piece": out["_vals"]["item_emb"][0].grad.numpy().copy()}
    blk = out["_vals"]["item_emb"][-1].grad
    r["dense_block_sqn"] = float((blk * blk).sum())
    r["p_label"] = np.exp(-r["ce"])
    r["floors"] = {}
    for k, (x, dy) in XW.items():
        xv, dv = out[x].detach().abs(), out[dy].grad.abs()
        r["floors"][k] = float((xv.reshape(-1, xv.shape[-1]).t() @ dv.reshape(-1, dv.shape[-1])).max())
    for v in ora.p.values():
        v.grad = None
    o2 = ora.forward(batch, with_neg=False)
    dl = torch.softmax(o2["logits"], 1).detach()
    dl[torch.arange(dl.shape[0]), torch.as_tensor(np.asarray(batch["label"]), dtype=torch.long)] -= 1.0
    (dl.abs() * o2["logits"]).sum().backward()
    r["cat_floors"] = {k: ora.p[k].grad.abs().numpy().copy() for k in TIME_PATH}
    return r


def floors_of(spec, ref):
    """the floors a case's gate takes: None | the lone session's max A (scalars) | the catalog sums of magnitudes (arrays)"""
    return {None: None, "lone": ref["floors"], "catalog": ref["cat_floors"]}[spec["floor"]]


_REF = {}


def first_reference(name):
    """the first step's oracle run at the initial parameters: once per process, shared by the precisions, never modified"""
    if name not in _REF:
        c = build(name)
        _REF[name] = reference(c["params"], c["content"], c["mw"], c["batches"][0])
    return _REF[name]


# ---- gates ---------------------------------------------------------------------------------------------------------------------
def _r(err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


def item_row_ratio(got, want, scoring):
    """worst row-wise rel_norm over the rows of item_emb that carry signal, over the precision's gradient gate"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    rn = np.linalg.norm(want, axis=1)
    if not rn.max() > 0:
        return 0.0
    big = rn >= MIXED_BIG_FRAC * rn.max()
    rel = np.linalg.norm(got - want, axis=1)[big] / rn[big]
    return float(rel.max()) / (MIXED_GRAD_RTOL if scoring == "bf16x3-mixed" else GRAD_RTOL)


def below_fp32(want, got, gmax):
    """A variable whose every oracle element is below 2^-24 of the step's largest gradient while the implementation holds exact zeros:
    the gradient through the exp-normaliser of a length-1 session is proportional to 1 - alpha = 1e-9 / (e + 1e-9), which fp32 rounds to
    0 (gpu_util.close has a floor of 1e-9 for it; at H = 250 the oracle's value is 3e-9).  Zero IS the fp32 answer there."""
    return float(np.abs(want).max()) < 2.0 ** -24 * gmax and not np.asarray(got).any()


def gate_ratios(g_e, sq_e, ref, scoring, floors=None):
    """error / bound (<= 1 passes) of every gradient, every clip norm and the row-wise item check, at check_grads' gates.
    `floors` (name -> max A, or an array A of the variable's shape): the variable's scale is max(max |want|, max A) — in the
    element-wise gates the absolute term; in the mixed precision the floor of the norm-wise gate, the reference of what counts as a
    large element and, for an array A, the norm the relative term is stated on, max(||want||, ||A||).  The clip norm of a dense weight
    with a floor (||g||^2) is allowed what that gate allows its gradient: 2 ||g|| E + E^2, E the norm of the allowed error."""
    from oracle.tcar_oracle import TABLES
    g_o, sq_o = ref["grads"], ref["sqn"]
    floors = floors or {}
    gmax = max(float(np.abs(v).max()) for v in g_o.values())
    mixed = scoring == "bf16x3-mixed"
    out = OrderedDict()
    for k, want in g_o.items():
        want = np.asarray(want, dtype=np.float64)
        got = np.asarray(g_e[k], dtype=np.float64).reshape(want.shape)
        if not mixed and below_fp32(want, got, gmax):
            out[k] = out["sqn " + k] = 0.0
            continue
        top = float(np.abs(want).max())
        A = np.asarray(floors.get(k, 0.0), dtype=np.float64)
        scale = max(top, float(A.max()))
        wn = np.linalg.norm(want)
        if mixed:
            E = MIXED_GRAD_RTOL * max(wn, np.linalg.norm(A) if A.ndim else 0.0) + 1e-7 * max(gmax, scale) * np.sqrt(want.size)
            r = _r(np.linalg.norm(got - want), E)
            big = np.abs(want) >= MIXED_BIG_FRAC * scale
            if big.any() and top > 1e-6 * gmax:
                r = max(r, float((np.abs(got[big] - want[big]) / np.abs(want[big])).max()) / MIXED_BIG_RTOL)
            out[k] = r
        else:
            out[k] = _r(np.abs(got - want), GRAD_RTOL * np.abs(want) + GRAD_ATOL * max(scale, 1e-30) + 1e-9)
            E = GRAD_RTOL * wn + (GRAD_ATOL * scale + 1e-9) * np.sqrt(want.size)
        extra = 2 * wn * E + E * E if (k in floors and k not in TABLES) else 0.0
        out["sqn " + k] = _r(abs(sq_e[k] - sq_o[k]), (MIXED_SQNORM_RTOL if mixed else SQN_RTOL) * sq_o[k] + 1e-12 + extra)
    out["item_emb rows"] = item_row_ratio(g_e["item_emb"], g_o["item_emb"], scoring)
    return out


def worst(r):
    k = max(r, key=r.get)
    return k, r[k]


def check(g_e, sq_e, ref, scoring, floors=None):
    """the assertion of both tests: check_grads itself on every variable without a floor (and not below fp32's resolution: below_fp32),
    the ratios on all of them"""
    gmax = max(float(np.abs(v).max()) for v in ref["grads"].values())
    keep = [k for k in ref["grads"] if not (floors and k in floors)
            and not (scoring != "bf16x3-mixed" and below_fp32(ref["grads"][k], g_e[k], gmax))]
    check_grads({k: g_e[k] for k in keep}, sq_e, OrderedDict((k, ref["grads"][k]) for k in keep), ref["sqn"], scoring)
    r = gate_ratios(g_e, sq_e, ref, scoring, floors)
    k, w = worst(r)
    assert w <= 1.0, (k, w)
    return r


# ---- plants: wrong gradients a correct gate must reject (CPU test) ---------------------------------------------------------------
def plants(name, i=0):
    """-> OrderedDict(plant -> (grads, sqn)) for batch i of the case at the initial parameters; built from oracle runs only"""
    c = build(name)
    ref = first_reference(name) if i == 0 else reference(c["params"], c["content"], c["mw"], c["batches"][i])
    b = c["batches"][i]
    B = b["seq"].shape[0]
    out = OrderedDict()
    copy = lambda: (OrderedDict((k, v.copy()) for k, v in ref["grads"].items()), dict(ref["sqn"]))
    # (a) one session's contribution dropped = the oracle on the batch without it (oracle(batch) - that session's part)
    for tag, s in (("session_last", B - 1), ("session_0", 0)):
        if B == 1:
            if tag == "session_0":
                continue
            out[tag] = (OrderedDict((k, np.zeros_like(v)) for k, v in ref["grads"].items()), {k: 0.0 for k in ref["sqn"]})
            continue
        sub = {k: np.delete(v, s, axis=0) for k, v in b.items()}
        r = reference(c["params"], c["content"], c["mw"], sub)
        out[tag] = (r["grads"], r["sqn"])
    if B > 128 and B % 128:
        # ... and the whole ragged tail of the last 128-row block
        sub = {k: v[:B // 128 * 128] for k, v in b.items()}
        r = reference(c["params"], c["content"], c["mw"], sub)
        out["tail_block"] = (r["grads"], r["sqn"])
    # (b) the label one-hot term of the item block dropped: row label_b + 1 loses -attout_item[b]
    g, sq = copy()
    np.add.at(g["item_emb"], b["label"].astype(np.int64) + 1, ref["attout_item"])
    out["label_onehot"] = (g, sq)
    # (c) a duplicated click counted once: the first repeated id keeps the piece of its first occurrence only
    flat = b["seq"].reshape(-1)
    ids, cnt = np.unique(flat, return_counts=True)
    if (cnt > 1).any():
        where = np.nonzero(flat == flat[np.isin(flat, ids[cnt > 1])][0])[0]
        g, sq = copy()
        g["item_emb"][flat[where[0]]] -= ref["seq_piece"].reshape(flat.size, -1)[where[1:]].sum(0)
        out["duplicate_once"] = (g, sq)
    # (d) one time table's candidate-side gradient without the clip Jacobian
    r = reference(c["params"], c["content"], c["mw"], b, straight_through=((PLANT_TABLE, "cand"),))
    g, sq = copy()
    g[PLANT_TABLE], sq[PLANT_TABLE] = r["grads"][PLANT_TABLE], r["sqn"][PLANT_TABLE]
    out["no_clip_jacobian"] = (g, sq)
    # (e) the clip norm of item_emb without its densified [1:] block
    g, sq = copy()
    sq["item_emb"] = sq["item_emb"] - ref["dense_block_sqn"]
    out["norm_without_dense_block"] = (g, sq)
    return ref, out
