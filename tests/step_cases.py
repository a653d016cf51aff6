"""The training-step cases and the gradient gates that the step tests share (test_gpu_parity.py holds the tests of them; fused_ref.py
and optim_ref.py build their fp64 references on the same inputs and the same tolerances)."""
import numpy as np

from gpu_util import close


def _case(N, H, Ht, B, T, K, seed, emb_std=0.35, w_std=0.12):
    from oracle.tcar_oracle import init_params_numpy
    rng = np.random.RandomState(seed)
    params = init_params_numpy(N, H, Ht, emb_std, w_std, rng)
    content = (rng.standard_normal((N + 1, H)) * 0.5).astype(np.float32)
    content[0] = 0
    mw = np.stack([rng.randint(1, 13, N), rng.randint(1, 32, N), rng.randint(1, 8, N), rng.randint(1, 25, N),
                   rng.randint(1, 61, N)], -1).astype(np.int32)
    b = {"seq": rng.randint(1, N + 1, (B, T)), "label": rng.randint(0, N, B), "pm": rng.randint(1, 13, (B, T)),
         "pd": rng.randint(1, 32, (B, T)), "pw": rng.randint(1, 8, (B, T)), "ph": rng.randint(1, 25, (B, T)),
         "pmi": rng.randint(1, 61, (B, T)), "cw": rng.randint(0, 7, B), "ch": rng.randint(0, 24, B),
         "gap": rng.randint(0, 12, (B, T)), "neg": rng.randint(0, N, (B, K))}
    b = {k: v.astype(np.int32) for k, v in b.items()}
    if T > 1:
        b["seq"][0, 1] = b["seq"][0, 0]            # a repeated item inside one session
    b["seq"][-1, 0] = b["seq"][0, 0]               # and across sessions (scatter collisions)
    return params, content, mw, b


CASES = [  # N, H, Ht, B, T, K
    (50, 12, 8, 1, 1, 3),
    (50, 12, 8, 3, 2, 4),
    (1000, 250, 64, 64, 7, 20),
    (1000, 40, 16, 3, 40, 5),
    (1000, 256, 64, 5, 3, 2),
    (129, 250, 64, 130, 3, 1),          # N just past one 128-row block, B past one 128-row plane block, a single negative
    (1000, 250, 64, 513, 2, 33),        # B = 512 + 1: a second (one-row) M tile in every scoring GEMM; K > 32 negatives
    (1000, 250, 64, 300, 8, 5),         # B * T = 2,400: a LONG bucket — un-split projections (> TCAR_PROJ_SPLIT_ROWS), small-table backward in chunks
]


def rel_norm(got, want):
    """norm-wise relative error ||got - want|| / ||want||"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-300))


# bf16x3-mixed (the precision bench.py and main.py default to): logits / loss at the 1e-3 gate, the two scoring-gradient
# GEMMs on plain bf16 operands -> EVERY gradient within 1e-2 norm-wise, every clip norm within 2e-2
MIXED_GRAD_RTOL = 1e-2
MIXED_SQNORM_RTOL = 2e-2
MIXED_BIG_FRAC, MIXED_BIG_RTOL = 0.1, 0.1


def check_grads(g_e, sq_e, g_o, sq_o, scoring, atol_scale=5e-5):
    """all 23 gradients and their S5 clip norms against the oracle, at the gate of the scoring precision"""
    gmax = max(float(np.abs(np.asarray(v)).max()) for v in g_o.values())
    for k in g_o:
        want = np.asarray(g_o[k], dtype=np.float64)
        if scoring == "bf16x3-mixed":
            # gradients that are rounding noise on both sides (zero in exact arithmetic) are compared on the step's scale
            got = np.asarray(g_e[k], dtype=np.float64)
            err = np.linalg.norm(got - want)
            assert err <= MIXED_GRAD_RTOL * np.linalg.norm(want) + 1e-7 * gmax * np.sqrt(want.size), ("grad " + k, err, np.linalg.norm(want))
            # ... and element-wise where an element carries signal (>= 10 % of the variable's largest): right sign, within 10 % —
            # a norm-wise gate alone would let a wrong-sign coordinate of a large variable through
            big = np.abs(want) >= MIXED_BIG_FRAC * np.abs(want).max()
            if big.any() and np.abs(want).max() > 1e-6 * gmax:
                rel = np.abs(got[big] - want[big]) / np.abs(want[big])
                assert rel.max() <= MIXED_BIG_RTOL, ("grad (large elements) " + k, float(rel.max()), int(big.sum()))
            assert abs(sq_e[k] - sq_o[k]) <= MIXED_SQNORM_RTOL * sq_o[k] + 1e-12, ("sqnorm", k, sq_e[k], sq_o[k])
        else:
            close(g_e[k], want, name="grad " + k, atol_scale=atol_scale)
            assert abs(sq_e[k] - sq_o[k]) <= 2e-3 * sq_o[k] + 1e-12, ("sqnorm", k, sq_e[k], sq_o[k])
