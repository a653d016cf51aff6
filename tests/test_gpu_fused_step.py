"""The fused training step's OWN gradients against the fp64 oracle at edge shapes (run with -m gpu on an MI355X).

`tcar_train_step_deferred` — the driver bench.py times and every training loop runs — takes the softmax epilogue, the anchored fold,
the one-hot dX / dE with (q, z) pairs and the in-launch slab folds; `loss_and_grads` takes the path with materialised logits.  Here
the fused step itself is held to the oracle, per case of fused_ref.cases() and per precision:
  make_resident -> step_form == the form the case table expects -> train_step(defer_update=True) -> per-session loss (1e-3), all 23
  gradients and S5 clip norms (check_grads) + the row-wise item_emb check -> flush() -> a fresh oracle at the engine's exported
  parameters -> a SECOND fused step on the case's second batch, same checks (the split early / rest update and the label-row early
  pass stand between two checked gradients).
tests/test_fused_step_ref.py shows on the CPU what these gates reject: a dropped session (tail tile, session 0), a dropped label
one-hot, a duplicated click counted once, a time table without its clip Jacobian, a clip norm without its densified block.
Every test prints the worst error / bound over the variables before it asserts.
"""
import numpy as np
import pytest
import torch

import fused_ref as F
from gpu_util import close

pytestmark = pytest.mark.gpu


def _engine(c, scoring):
    from tcar_amd.engine import TcarEngine
    eng = TcarEngine(c["params"], c["content"], c["mw"], max_grad=F.MAX_GRAD, scoring=scoring, lr=c["spec"]["lr"])
    if c["spec"]["tuning"]:
        eng.set_tuning(**c["spec"]["tuning"])
    return eng


def _held(tag, eng, loss, ref, scoring, floors):
    close(loss.cpu().numpy(), ref["loss"], rtol=1e-3, name=tag + " loss")
    g_e, sq_e = eng.export_grads(), eng.export_sqnorms()
    r = F.gate_ratios(g_e, sq_e, ref, scoring, floors)
    k, w = F.worst(r)
    print("%s: worst error / bound %.3f (%s); item_emb rows %.3f" % (tag, w, k, r["item_emb rows"]))
    if w > 1.0:
        print("   over the bound:", {a: round(b, 3) for a, b in r.items() if b > 1.0})
    F.check(g_e, sq_e, ref, scoring, floors)


@pytest.mark.parametrize("scoring", F.SCORINGS)
@pytest.mark.parametrize("name", F.case_names())
def test_fused_step_gradients_match_oracle(name, scoring):
    """Two teacher-forced fused steps per case; gates: fused_ref.check — check_grads + the row-wise item_emb check; the cancellation
    floor in `lone_twice`, the catalog's sums of magnitudes behind the time columns where every item has one publish time (the exact
    gradient there is zero: fp64 leaves 1e-16), exact zeros below fp32's resolution (fused_ref.below_fp32).  Without the last two the
    f32 / bf16x3 steps measured 455 to 8,650 times the plain bound on attout_pt_trans (errors 1e-7 to 7e-6 against a zero) and 9.6 on
    cont_attention/res_linear_trans/w_3d at B = T = 1, H = 250 (0 against 3e-9); a second `converged_wide` step at lr 1e-3 left the
    band (p = 1 - 2e-6) and measured 13: it runs at lr 3e-5 and the band is asserted on the second step too.
    Measured on an MI355X, worst error / bound over variables, both steps and the cases of a group (f32 / bf16x3 / bf16x3-mixed):
    eight shapes 0.02 / 0.20 / 0.33; thresholds 0.03 / 0.19 / 0.69; catalog edges 0.02 / 0.17 / 0.32; K 0.02 / 0.22 / 0.44; forms and
    widths 0.02 / 0.21 / 0.70; lone_twice 0.07 / 0.21 / 0.36; copies130 0.01 / 0.10 / 0.55; collisions 0.01 / 0.14 / 0.24; one publish
    time 0.02 / 0.15 / 0.25; softmax regimes 0.62 / 0.73 / 0.45.  The mixed step at ldh = 320 first FAULTED (the dE (q, z) epilogue's
    ragged last N tile, fixed in gemm_bf16.hip; docs/KERNELS.md, "Fused-step gradients at edge shapes").  The file's 153 tests take
    13 s of the suite's 281 s."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = F.build(name)
    want_form = F.expected_form(scoring, c["spec"])
    eng = _engine(c, scoring)
    ref = F.first_reference(name)
    for i, batch in enumerate(c["batches"]):
        bt = eng.make_resident(batch)
        form = eng.step_form(bt)
        assert form == want_form, (name, scoring, i, form, want_form)
        loss = eng.train_step(None, bt=bt, defer_update=True)
        torch.cuda.synchronize()
        assert eng._pending_lr is not None                                  # the update is owed: the gradients are this step's own
        _held("%s %s step %d" % (name, scoring, i), eng, loss, ref, scoring, F.floors_of(c["spec"], ref))
        if i == 0:
            eng.flush()
            ref = F.reference(eng.export_params(), c["content"], c["mw"], c["batches"][1])
            if c["spec"]["regime"] is not None:                             # the second step is still inside the regime's band
                _, _, lo, hi, what = c["spec"]["regime"]
                v = ref["p_label"] if what == "p" else ref["ce"]
                assert lo <= v.min() and v.max() <= hi, (name, what, v)


DEGENERATE = [n for n, s in F.cases().items() if s["both"]]


@pytest.mark.parametrize("scoring", F.SCORINGS)
@pytest.mark.parametrize("name", DEGENERATE)
def test_degenerate_batches_through_loss_and_grads(name, scoring):
    """the degenerate batches of part B through the op-level path too (materialised logits), at the same gates.
    Measured on an MI355X, worst error / bound (f32 / bf16x3 / bf16x3-mixed): lone_twice 0.04 / 0.21 / 0.29; copies130 0.01 / 0.09 /
    0.50; collisions 0.00 / 0.11 / 0.30; one publish time 0.02 / 0.13 / 0.32; softmax regimes 0.46 / 0.48 / 0.35."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = F.build(name)
    eng = _engine(c, scoring)
    ref = F.first_reference(name)
    loss = eng.loss_and_grads(c["batches"][0])
    torch.cuda.synchronize()
    _held("%s %s loss_and_grads" % (name, scoring), eng, loss, ref, scoring, F.floors_of(c["spec"], ref))
