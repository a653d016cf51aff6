"""The N = 700 serving case that the engine-level tests of the serving calls share (test_gpu_serve.py, test_gpu_cand_serve.py,
test_gpu_retrieve_serve.py, test_gpu_ragged_*.py, test_gpu_shard_*.py; ragged_util.py builds its mixed batches on it): the shape,
the inputs with the fp64 oracle's logits / CE of them, the unlabelled feed, item keys and windows, the candidate lists and the band
of a coarse score.  Every test of those modules expects THESE numbers: a change here moves all of them.  Computed once, shared,
never written."""
import numpy as np
import torch

from gpu_util import _kb32_index

N, H, Ht, B, T, K = 700, 250, 64, 41, 3, 5        # the shape of test_gpu_parity.py's Python-sequenced op-level step against the C++ driver
PANEL, TOPK = 256, 20                             # three panels, the last one partial

U = 2.0 ** -8                                     # the coarse band's unit (test_gpu_retrieve_serve.py's header derives it)
SHORT = 128
C_ = 37                                           # slots of a candidate list


_REF = {}


def reference():
    """inputs and the oracle's fp64 logits / CE: computed once, shared, never written"""
    if not _REF:
        from oracle.tcar_oracle import TcarOracle, init_params_numpy
        rng = np.random.RandomState(17)
        params = init_params_numpy(N, H, Ht, 0.35, 0.12, rng)
        content = (rng.standard_normal((N + 1, H)) * 0.5).astype(np.float32)
        content[0] = 0
        mw = np.stack([rng.randint(1, 13, N), rng.randint(1, 32, N), rng.randint(1, 8, N), rng.randint(1, 25, N),
                       rng.randint(1, 61, N)], -1).astype(np.int32)
        b = {"seq": rng.randint(1, N + 1, (B, T)), "label": rng.randint(0, N, B), "pm": rng.randint(1, 13, (B, T)),
             "pd": rng.randint(1, 32, (B, T)), "pw": rng.randint(1, 8, (B, T)), "ph": rng.randint(1, 25, (B, T)),
             "pmi": rng.randint(1, 61, (B, T)), "cw": rng.randint(0, 7, B), "ch": rng.randint(0, 24, B),
             "gap": rng.randint(0, 12, (B, T)), "neg": rng.randint(0, N, (B, K))}
        b = {k: v.astype(np.int32) for k, v in b.items()}
        b["seq"][0, 1] = b["seq"][0, 0]
        logits, ce = TcarOracle(params, content, mw).eval_batch(b)
        s, ce = logits.numpy().astype(np.float64), ce.numpy().astype(np.float64)
        for a in list(b.values()) + [s, ce]:
            a.setflags(write=False)
        _REF.update(params=params, content=content, mw=mw, batch=b, s=s, ce=ce, delta=1e-3 * np.abs(s).max(1))
    return _REF


def _feed():
    return {n: v for n, v in reference()["batch"].items() if n not in ("label", "neg")}


def _keys_and_windows():
    rng = np.random.RandomState(31)
    keys = rng.permutation(N).astype(np.int32)
    lo = rng.randint(0, 300, B).astype(np.int32)
    hi = (lo + rng.randint(30, 400, B)).astype(np.int32)              # pools of 30 .. 400 items: some shorter than 64
    return keys, lo, hi


def _lists():
    """the label in slot 0, 30 random ids, 3 repeats of earlier slots and 3 empty slots (-1, N, -7); clicked: the label and a few more"""
    lab = reference()["batch"]["label"]
    rng = np.random.RandomState(23)
    cand = np.empty((B, C_), np.int32)
    cand[:, 0] = lab
    cand[:, 1:31] = rng.randint(0, N, (B, 30))
    cand[:, 31:34] = np.take_along_axis(cand, rng.randint(0, 31, (B, 3)), 1)
    cand[:, 34:] = [-1, N, -7]
    for b in range(B):                                  # the empty slots and the repeats sit somewhere else in every row
        cand[b, 1:] = cand[b, 1:][rng.permutation(C_ - 1)]
    clicked = (rng.rand(B, C_) < 0.15).astype(np.int32)
    clicked[:, 0] = 1
    return cand, clicked


def beta_of_operands(m):
    """the band of a coarse score, u (|A| |E|^T) + delta_b, from read-back operands m["A"], m["E"]"""
    r = reference()
    return U * (np.abs(m["A"]) @ np.abs(m["E"]).T) + r["delta"][:, None]


def beta_of_engine(eng, delta):
    """the same band from the operands the engine `eng` scored last, with the logits gate `delta` of the caller's own oracle"""
    g = eng.geo
    A = eng.attout[:B].cpu().numpy().astype(np.float64)
    idx = torch.tensor(_kb32_index(eng.e16h.shape[0], g.ek)[:N], device=eng.dev)
    E = (eng.e16h.flatten()[idx].double() + eng.e16l.flatten()[idx].double()).cpu().numpy()
    return U * (np.abs(A) @ np.abs(E).T) + delta[:, None]
