"""CPU companion of test_gpu_optimizer.py: the float64 reference of the clip-and-Adam update, its bounds and the teacher-forced step
sequences, checked WITHOUT a GPU.  The stand-in implementation is `optim_ref.adam32`: numpy float32 in the kernels' operation order.
It must stay inside every gate (the bounds are reachable by a correct fp32 implementation), and every gate must reject the float64
reference computed with a wrong clip — off, from sqn_dense alone, from the neighbouring slot — on the inputs the GPU tests use."""
import numpy as np
import pytest

import optim_ref as R
from gpu_util import close


def _a_blocks(x):
    """(name, slot, w0, g, m0, v0) of the item table and the four arena segments of one part-A input set"""
    yield "item", R.ITEM_SLOT, x["w2"], x["g2"], x["m2"], x["v2"]
    for name, (slot, off, n) in zip("abcd", R.ARENA_SEGS):
        yield name, slot, x["w"][off:off + n], x["g"][off:off + n], x["m"][off:off + n], x["v"][off:off + n]


@pytest.mark.parametrize("clip", [R.A_CLIP, 0.0])
@pytest.mark.parametrize("shape", list(R.A_SHAPES))
def test_fp32_restatement_stays_inside_the_rounding_bounds(shape, clip):
    """Part A's bounds count one rounding of 2^-24 per fp32 operation.  Measured here for the float32 restatement on the seeded
    inputs (worst error / bound over the item table and the arena, both clips): m 0.33, v 0.33 of 2^-21 (|b1 m0| + |(1 - b1) gc|) and
    2^-21 v in every shape; w 0.50 of 2^-23 |w0| + 2^-20 |update| in the two small shapes and 1.46 in the 16.8 M elements of the
    largest (an m that cancels beside a small w0: the bound is stated in |update|), which therefore takes the factor 2 * 1.46
    (optim_ref.A_W_FACTOR)."""
    x = R.a_inputs(shape)
    args = R.adam_args(R.A_STEP, clip)
    assert abs(args[1] / R.LR - 1) > 0.05                                   # a step whose bias-corrected rate is not lr
    worst = {"m": 0.0, "v": 0.0, "w": 0.0}
    for name, slot, w0, g, m0, v0 in _a_blocks(x):
        sc32 = R.clip_scale(x["sqn_dense"], x["sqn_pieces"], x["use_dense"], slot, args[0], dtype=np.float32)
        sc64 = R.clip_scale(x["sqn_dense"], x["sqn_pieces"], x["use_dense"], slot, args[0])
        if name == "c" or clip == 0:
            assert sc32 == 1 and sc64 == 1
        r = R.gate_a(*R.adam32(w0, g, m0, v0, sc32, args), R.adam64(w0, g, m0, v0, sc64, args), R.A_W_FACTOR.get(shape, 1.0))
        print(shape, clip, name, r)
        assert max(r.values()) <= 1.0, (shape, name, r)
        worst = {k: max(worst[k], r[k]) for k in worst}
    print("worst", shape, clip, worst)


# which blocks each wrong clip changes (the others keep their factor: pieces 0, or sc = 1 with a neighbour that clips too, ...)
A_REJECTS = {"off": ("item", "a", "b"), "dense_only": ("item", "b"), "neighbour": ("item", "a", "b", "c")}


@pytest.mark.parametrize("wrong", R.WRONG_CLIPS)
def test_part_a_gates_reject_a_wrong_clip(wrong):
    x = R.a_inputs("rows131")
    args = R.adam_args(R.A_STEP, R.A_CLIP)
    for name, slot, w0, g, m0, v0 in _a_blocks(x):
        sc32 = R.clip_scale(x["sqn_dense"], x["sqn_pieces"], x["use_dense"], slot, args[0], dtype=np.float32)
        bad = R.clip_scale(x["sqn_dense"], x["sqn_pieces"], x["use_dense"], slot, args[0], wrong=wrong)
        r = R.gate_a(*R.adam32(w0, g, m0, v0, sc32, args), R.adam64(w0, g, m0, v0, bad, args))
        if name in A_REJECTS[wrong]:
            assert r["m"] > 1e3 and r["v"] > 1e3 and r["w"] > 1, (wrong, name, r)       # far outside, not at the edge
        else:
            assert max(r.values()) <= 1.0, (wrong, name, r)


def test_oracle_state_round_trip():
    """TcarOracle.export_state / load_state: TcarEngine's keys, fp32 values, and a loaded oracle continues bit for bit"""
    from oracle.tcar_oracle import TcarOracle
    s = R.b_sequence("base")
    st = s["steps"][1]["state0"]
    assert st["meta/step"] == 1 and st["meta/beta_pow"].dtype == np.float32
    assert all(st[t + k].dtype == np.float32 for t in ("var/", "m/", "v/") for k in s["order"])
    assert np.abs(st["m/item_emb"]).max() > 0 and not np.abs(st["m/item_emb"][0]).any()
    ora = TcarOracle(s["params"], s["content"], s["mw"], max_grad=s["max_grad"])
    ora.load_state(st)
    back = ora.export_state()
    assert all(np.array_equal(back[k], st[k]) for k in st)
    ora.train_step(s["steps"][1]["batch"])
    after = ora.export_state()
    assert all(np.array_equal(after[k], s["steps"][1]["state1"][k]) for k in after)
    assert R.lr_t_from_beta_pow(after["meta/beta_pow"]) == pytest.approx(R.adam_args(1, 0)[1], rel=1e-6)


def _standin(s, st, k):
    """one variable's fp32 update from the oracle's gradient and clip norm rounded to fp32"""
    g = st["grads"][k].astype(np.float32)
    sc = np.float32(s["max_grad"]) / np.maximum(np.sqrt(np.float32(st["sqn"][k])), np.float32(s["max_grad"]))
    lr_t = R.lr_t_from_beta_pow(st["state1"]["meta/beta_pow"])
    return R.adam32(st["state0"]["var/" + k], g, st["state0"]["m/" + k].reshape(g.shape), st["state0"]["v/" + k].reshape(g.shape), sc,
                    (s["max_grad"], lr_t, R.B1, R.B2, R.EPS))


@pytest.mark.parametrize("case", list(R.B_CASES))
def test_step_sequences_exercise_both_branches_and_admit_fp32(case):
    """every teacher-forced step clips >= 3 variables (item_emb — norm from pieces — and a dense weight among them), leaves >= 3
    below the clip, and the fp32 stand-in passes the gates of part B at both precisions"""
    s = R.b_sequence(case)
    shapes = set()
    for i, st in enumerate(s["steps"]):
        b = st["batch"]
        shapes.add(b["seq"].shape)
        clipped, unclipped = R.clip_census(st["sqn"], s["max_grad"], s["order"])
        assert len(clipped) >= 3 and len(unclipped) >= 3, (i, clipped, unclipped)
        assert "item_emb" in clipped and any(R.is_dense_weight(k) for k in clipped), (i, clipped)
        assert len(np.unique(b["seq"])) < b["seq"].size or b["seq"].shape[0] == 1     # a repeated item id (not in the lone session)
        gmax = max(float(np.abs(g).max()) for g in st["grads"].values())
        for k in s["order"]:
            w, m, v = _standin(s, st, k)
            for scoring in ("f32", "bf16x3-mixed"):
                r = R.gate_b(m, v, st["ref"][k], scoring, gmax)
                assert max(r.values()) <= 1.0, (i, k, scoring, r)
                if k in unclipped:
                    assert st["ref"][k]["sc"] == 1.0 and R.gate_b_unclipped(m, st["ref"][k], scoring, gmax) <= 1.0, (i, k)
            assert R.gate_w(w, st["state0"]["var/" + k], m, v, R.lr_t_from_beta_pow(st["state1"]["meta/beta_pow"])) <= 1.0, (i, k)
            # the oracle's own fp32 state agrees with its float64 targets (the reference is consistent with itself)
            assert np.allclose(st["state1"]["m/" + k].reshape(m.shape), st["ref"][k]["m"], rtol=1e-6, atol=1e-12), (i, k)
    assert len(shapes) == len(s["steps"])                                   # every step another (B, T)
    if case == "base":
        assert any(sh[0] == 1 for sh in shapes)
        assert any(len(np.unique(st["batch"]["label"])) < st["batch"]["label"].size for st in s["steps"])


@pytest.mark.parametrize("wrong", R.WRONG_CLIPS)
@pytest.mark.parametrize("scoring", ["f32", "bf16x3-mixed"])
def test_part_b_gates_reject_a_wrong_clip(scoring, wrong):
    """In every step of the base sequence the moments of item_emb tell the right clip from each wrong one, at the element-wise gate and
    at the looser norm-wise gate of the mixed precision; a dense weight above the clip shows `off` and `neighbour` too.  (`dense_only`
    drops the IndexedSlices pieces: a dense weight has none, so only the item table and the gathered tables can show it.)  A wrong
    rate is caught by the weights' gate: the rate of the step after moves w beyond its bound."""
    s = R.b_sequence("base")
    for i, st in enumerate(s["steps"]):
        bad = R.step_reference(st["grads"], st["sqn"], st["state0"], s["max_grad"], wrong=wrong, dense_sqn=st["dense_sqn"], order=s["order"])
        gmax = max(float(np.abs(g).max()) for g in st["grads"].values())
        clipped, _ = R.clip_census(st["sqn"], s["max_grad"], s["order"])
        dense = [k for k in clipped if k.endswith("/w1")][0]
        for k in ["item_emb"] + (["dec_pos"] if wrong == "dense_only" else [dense]):
            w, m, v = _standin(s, st, k)
            r = R.gate_b(m, v, bad[k], scoring, gmax)
            print(i, k, scoring, wrong, r, "sc", st["ref"][k]["sc"], bad[k]["sc"])
            assert r["m"] > 1.0 and r["v"] > 1.0, (i, k, scoring, wrong, r)
        k = "item_emb"
        w, m, v = _standin(s, st, k)
        lr_next = R.lr_t_from_beta_pow(st["state1"]["meta/beta_pow"] * np.float32([R.B1, R.B2]))
        assert R.gate_w(w, st["state0"]["var/" + k], m, v, lr_next) > 1.0, i


@pytest.mark.parametrize("case", list(R.B_CASES))
def test_evaluation_gate_rejects_a_stale_item_table(case):
    """The evaluation behind the last update compares LOGITS at the suite's gate (gpu_util.close, 1e-3): an item table left one
    update behind — everything else up to date — fails it, in every row of the table or only in the rows the last batch did not
    gather (a rest pass that never ran).  The cross-entropy alone would let the base size through (3e-4 relative)."""
    s = R.b_sequence(case)
    last = s["steps"][-1]
    close(R.eval_reference(s, last["state1"])[0], s["eval_logits"], name="logits")      # the reference repeats itself
    stale = dict(last["state1"])
    stale["var/item_emb"] = last["state0"]["var/item_emb"]
    with pytest.raises(AssertionError):
        close(R.eval_reference(s, stale)[0], s["eval_logits"], name="logits, whole table stale")
    part = dict(last["state1"])
    part["var/item_emb"] = last["state0"]["var/item_emb"].copy()
    early = np.unique(last["batch"]["seq"])
    part["var/item_emb"][early] = last["state1"]["var/item_emb"][early]
    with pytest.raises(AssertionError):
        close(R.eval_reference(s, part)[0], s["eval_logits"], name="logits, rest rows stale")
