"""The checkers of tests/serve_shapes_ref.py can fail (CPU only).  "Engine" outputs are forged from the fp64 oracle on the cases
`block+1` and `wide`: the numpy model of the select fold (tests/select_ref.py), of the shortlist (tests/retrieve_ref.py) and of the
candidate ranks (tests/cand_ref.py) applied to a score matrix.  The honest matrix (the oracle's scores rounded to fp32; coarse: the
product of the operands rounded to bf16) is accepted by every checker; each matrix below, a mistake the serving composition could
make, is refused.

Seeds and scales: the seeds of CASES with emb_std = 0.35, w_std = 0.12 (the values of tests/test_gpu_parity.py) make every forgery
but one visible from the oracle alone.  The exception is a coarse score off by the FACTOR 1 + 2^-6: on this model
|A| |E|^T >= 4 |s| for every entry, so 2^-6 |s| stays inside beta = 2^-8 |A| |E|^T + delta_b — the largest 2^-6 |s| / beta over the
shortlists was 0.81 (block+1) and 0.86 (wide), and between 0.74 and 1.06 over emb_std in {0.35, 0.7, 1.2} x w_std in
{0.12, 0.25, 0.5}: no scale makes it visible.  That factor is therefore held to the band of the fp32 engine (beta = delta_b), which
refuses it, and the split-bf16 band is shown to refuse an error of 2^-6 relative to what IT is relative to, |A| |E|^T (operands kept
to six bits instead of eight).

The per-case shares of sessions that rule (e) of the two-stage check leaves out are pinned here: none, on any case."""
import numpy as np
import pytest

import serve_shapes_ref as R

FORGED = ("block+1", "wide")
K = R.TOPK


def _refused(check, *a, **kw):
    with pytest.raises(AssertionError):
        check(*a, **kw)


def _bf16(a):
    import torch
    return torch.tensor(a, dtype=torch.float32).bfloat16().double().numpy()


def _outputs(ref, x, name, coarse=None, lab_score=None, excl="seen"):
    """what an engine that scored x would hand the checkers"""
    C = R.shortlist_size(name)
    cand = R.candidate_lists(name, 65)
    coarse = x if coarse is None else coarse
    return dict(eval=R.forge_eval(x, ref["label"], K, lab_score), recommend=R.forge_recommend(x, ref["seen"] if excl == "seen" else None, K),
                cand=(cand,) + R.forge_candidates(x, cand), retrieve=R.forge_retrieve(coarse, C), two=R.forge_two_stage(coarse, x, K, C))


def _check_all(ref, out, name, split):
    C = R.shortlist_size(name)
    R.check_eval(ref, *out["eval"], k=K, name=name)
    R.check_recommend(ref, *out["recommend"], k=K, name=name)
    R.check_candidates(ref, *out["cand"], name=name)
    R.check_coarse(ref, *out["retrieve"], C=C, split=split, name=name)
    R.check_two_stage(ref, *out["two"], k=K, C=C, split=split, name=name)


@pytest.mark.parametrize("name", FORGED)
def test_the_honest_outputs_pass_and_every_forgery_is_refused(name):
    ref = R.reference(name)
    s, lab, seen = ref["s"], ref["label"], ref["seen"]
    B, N = s.shape
    C = R.shortlist_size(name)
    x = s.astype(np.float32)
    honest_coarse = (_bf16(ref["A"]) @ _bf16(ref["E"]).T).astype(np.float32)
    _check_all(ref, _outputs(ref, x, name), name, split=False)                       # the fp32 engine: coarse = its own scores
    _check_all(ref, _outputs(ref, x, name, coarse=honest_coarse), name, split=True)
    assert np.abs(honest_coarse - x).max() > 0

    # one 128-row catalog block scored from its neighbour's plane: items [128, 256) carry the scores of [0, 128)
    wrong = x.copy()
    blk = np.arange(128, min(256, N))
    wrong[:, blk] = x[:, blk - 128]
    out = _outputs(ref, wrong, name)
    _refused(R.check_eval, ref, *out["eval"], k=K)
    _refused(R.check_candidates, ref, *out["cand"])
    _refused(R.check_coarse, ref, *out["retrieve"], C=C, split=True)

    # the last, one-column panel dropped
    assert N % 128 == 1
    wrong = x.copy()
    wrong[:, N - 1] = -np.inf
    out = _outputs(ref, wrong, name)
    _refused(R.check_eval, ref, *out["eval"], k=K)
    _refused(R.check_recommend, ref, *out["recommend"], k=K)
    _refused(R.check_coarse, ref, *out["retrieve"], C=C, split=True)

    # the label score taken from row label + 1
    out = _outputs(ref, x, name, lab_score=x[np.arange(B), (lab + 1) % N])
    _refused(R.check_eval, ref, *out["eval"], k=K)

    # the last session (the second M tile's / plane block's) scored with session 0's attout
    wrong = x.copy()
    wrong[B - 1] = x[0]
    out = _outputs(ref, wrong, name)
    _refused(R.check_eval, ref, *out["eval"], k=K)
    _refused(R.check_recommend, ref, *out["recommend"], k=K)
    _refused(R.check_candidates, ref, *out["cand"])
    _refused(R.check_coarse, ref, *out["retrieve"], C=C, split=True)

    # the seen items left in a recommend list
    out = _outputs(ref, x, name, excl=None)
    _refused(R.check_recommend, ref, *out["recommend"], k=K)

    # a coarse score off by 2^-6 relative (module docstring): the factor against the fp32 band, the operand-relative error against beta
    _refused(R.check_coarse, ref, *R.forge_retrieve(x * np.float32(1 + 2.0 ** -6), C), C=C, split=False)
    off = (honest_coarse + 2.0 ** -6 * ref["absdot"]).astype(np.float32)
    _refused(R.check_coarse, ref, *R.forge_retrieve(off, C), C=C, split=True)
    # ... and a two-stage list that took its k best by the coarse scores is not the top k of the exact ones
    top, top_sc, ids, ex = R.forge_two_stage(honest_coarse, x, K, C)
    by_coarse = np.stack([ids[b, :K] for b in range(B)])
    assert (by_coarse != top).any()
    _refused(R.check_two_stage, ref, by_coarse, np.take_along_axis(ex, np.argsort(-ex, 1)[:, :K], 1), ids, ex, k=K, C=C, split=True)


@pytest.mark.parametrize("name", FORGED)
def test_scores_from_untrained_time_columns_are_refused_after_training(name):
    """phase B: against the oracle of the TRAINED variables, the scores of a candidate-time plane that was never rebuilt and the
    scores of the variables before training both fail every exact call"""
    t = R.trained_reference(name)
    ref = t["after"]
    _check_all(ref, _outputs(ref, ref["s"].astype(np.float32), name), name, split=False)
    assert np.isfinite(t["loss3"]).all()
    for wrong in (t["stale"], t["before"]["s"]):
        out = _outputs(ref, wrong.astype(np.float32), name)
        _refused(R.check_eval, ref, *out["eval"], k=K)
        _refused(R.check_recommend, ref, *out["recommend"], k=K)
        _refused(R.check_candidates, ref, *out["cand"])
        _refused(R.check_coarse, ref, *out["retrieve"], C=R.shortlist_size(name), split=False)


# measured from the oracle alone (u = 2^-8, k = 20, C = min(128, Npad)): the smallest margin gap / (2 max beta) per case, split-bf16
# band / fp32 band; `one` has C > N, so its shortlist is the whole catalog
MARGINS = {"one": (np.inf, np.inf), "block+1": (18.12, 416.2), "tile+1": (4.61, 90.4), "long": (10.29, 139.5), "exact": (5.83, 127.0),
           "wide": (7.80, 167.5)}


@pytest.mark.parametrize("name", list(R.CASES))
def test_rule_e_of_the_two_stage_check_leaves_out_no_session_of_any_case(name):
    ref = R.reference(name)
    for split, floor in zip((True, False), MARGINS[name]):
        keep, margin = R.kept_sessions(ref, K, R.shortlist_size(name), split)
        assert keep.all() and (~keep).mean() == 0.0, (name, split)
        assert margin.min() >= floor and (floor == np.inf or margin.min() <= floor * 1.01), (name, split, margin.min())


def test_the_cases_are_the_shapes_they_are_meant_to_be():
    ek = lambda c: 2 * ((c.H + 63) // 64 * 64) + 5 * 64
    c = R.CASES
    assert [ek(c[n]) for n in c] == [448, 832, 832, 448, 832, 960]
    assert c["one"].B == 1 and c["one"].T == 1 and c["one"].N < 64
    assert c["block+1"].N == 129 and c["block+1"].B == 130 and c["tile+1"].B == 513 and c["tile+1"].N % 128 == 104
    assert c["long"].T == 40 and c["exact"].N % 256 == 0 and c["exact"].H % 64 == 0 and c["wide"].H > 256 and c["wide"].N == 257
    assert len(R.SCORINGS) == 14 and len(R.TRAINED) == 12 and len({v.seed for v in c.values()}) == len(c)
    for name, v in c.items():
        lens = R.lengths(name)
        assert 1 in lens and v.T in lens and lens.max() <= v.T and (len(set(lens.tolist())) > 1) == (v.B > 1)
        cand = R.candidate_lists(name, 65)
        assert (cand[:, 0] == R.inputs(name)[3]["label"]).all() and ((cand < 0) | (cand >= v.N)).sum() == 3 * v.B
        assert R.candidate_lists(name, 1).shape == (v.B, 1)


def test_the_short_list_form_of_check_band_asks_for_exactly_the_eligible_items():
    rng = np.random.RandomState(4)
    s = rng.standard_normal((2, 9))
    delta = 1e-3 * np.abs(s).max(1)
    gone = np.array([[0, 3, -1], [8, -1, -1]])
    want = np.full((2, 12), -1, np.int32)
    for b in range(2):
        left = [n for n in np.argsort(-s[b]) if n not in gone[b]]
        want[b, :len(left)] = left
    R.check_band(s, delta, want, 12, gone=gone, short=True)
    _refused(R.check_band, s, delta, want, 12, gone=gone)                          # the k-entry form still demands k entries
    R.check_band(s, delta, want[:, :5], 5, gone=gone)
    R.check_band(s, delta, want[:, :5], 5, gone=gone, short=True)                  # k or more eligible: the same checks
    for spoil in ("short", "tail", "swap"):
        bad = want.copy()
        if spoil == "short":
            bad[0, 6] = -1                                                         # an eligible item missing
        elif spoil == "tail":
            bad[1, 8] = 8                                                          # an excluded item behind the list
        else:
            bad[0, [0, 6]] = bad[0, [6, 0]]                                        # out of order by far more than 2 delta
        _refused(R.check_band, s, delta, bad, 12, gone=gone, short=True)
    bad = want[:, :5].copy()
    bad[0, 4] = want[0, 6]
    _refused(R.check_band, s, delta, bad, 5, gone=gone, short=True)
