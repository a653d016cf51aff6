"""CPU companion of test_gpu_gemm_small.py: the references, gates and case table of gemm_ref.py, checked WITHOUT a GPU.

 * the numpy stand-in of both kernels stays inside every gate on every real-valued case and is exact on every integer case;
 * every gate refuses planted faults on the suite's own inputs, and a fault that removes ONE k element exceeds the real-valued gate
   in >= 95 % of the outputs it touches;
 * the case table reaches every path of the launchers (both fp32 tiles in all three layouts, x3 stage counts 1 .. 5, both ring
   forms, 1 .. 3 segments, a 10-problem group with holes, a workgroup count that is no multiple of 8), asserted from the Python
   restatement of the tile / stage / split arithmetic.

Worst error / bound of the stand-in per group of real-valued cases, fp32 | x3 (printed per case by the first test):
    edge 0.16 | 0.70   single 0.13 | 0.31   tile128 0.12 | 0.39   segments 0.02 | 0.08   groups 0.14 | 0.41   splitk 0.11 | 0.34
    epilogue 0.11 | 0.35
by K on the x3 gate: 0.55 at 15, 0.70 at 16, 0.54 at 17, 0.42 at 28, 0.36 at 36, 0.12 at 129 .. 132, 0.07 at 256 .. 260.  A dropped k element is
beyond the gate in 96.2 % (K = 260) to 100 % of the outputs.
"""
import numpy as np
import pytest

import gemm_ref as R

CASES = R.all_cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
RUNS = [(c["name"], e) for c in CASES for e in R.entries(c)]
_built = {}


def built(name):
    """operands are drawn once per case and never modified (stand-in and judge copy what they write)"""
    if name not in _built:
        _built[name] = R.build(BY_NAME[name])
    return _built[name]


def plain(case):
    """every output element depends on every k of its problem (no activation, no split)"""
    return all(not p["act"] and not p["dact"] and p["splitk"] <= 1 for p in case["probs"])


@pytest.mark.parametrize("name,entry", RUNS)
def test_standin_passes_every_gate(name, entry):
    case = BY_NAME[name]
    w = R.check(case, built(name), R.standin(case, built(name), entry), entry)
    print("%-34s %-22s worst err / bound %.3f" % (name, entry, w))
    assert w < 1.0 if case["kind"] == "real" else w == 0.0


def test_poison_is_in_place():
    """the builder's promise: NaN around every operand, the sentinel around every output"""
    for name in ("edge-K36-L0-real", "edge-K17-L2-int", "pack-L1-int", "dact2-L0-real", "slab-K96-s7-L2-int"):
        case = BY_NAME[name]
        for p, b in zip(case["probs"], built(name)):
            for s, K in enumerate(p["K"]):
                rows_a, cols_a = (p["M"], K) if case["layout"] != 2 else (K, p["M"])
                rows_b, cols_b = (p["N"], K) if case["layout"] == 1 else (K, p["N"])
                for buf, r, c in ((b["A"][s], rows_a, cols_a), (b["B"][s], rows_b, cols_b)):
                    assert buf.shape[1] % 4 == 0 and buf.shape[0] == r + 2
                    assert np.isfinite(buf[:r, :c]).all() and np.isnan(buf[r:]).all() and np.isnan(buf[:, c:]).all()
            assert (b["C"][b["S"] * p["M"]:] == R.SENT).all() and (b["C"][:, p["N"]:] == R.SENT).all()
            for k in ("plane_hi", "plane_lo", "pack_hi", "pack_lo"):
                assert k not in b or (b[k] == R.SENT16).all()


def _refused(name, entry, fault):
    case = BY_NAME[name]
    fails, ratios = R.judge(case, built(name), R.standin(case, built(name), entry, fault=fault), entry)
    assert fails, (name, entry, fault, "the gate let the fault pass")
    return ratios


def _names(pred):
    return [c["name"] for c in CASES if pred(c)]


DROP_K = _names(lambda c: plain(c) and c["group"] in ("edge", "single", "segments", "groups"))


@pytest.mark.parametrize("entry", [R.F32G, R.X3G])
@pytest.mark.parametrize("name", DROP_K)
def test_a_dropped_k_tail_is_refused(name, entry):
    """the last k element of every problem's last segment is left out"""
    ratios = _refused(name, entry, "k_tail")
    if BY_NAME[name]["kind"] == "real":
        r = np.concatenate([x.ravel() for x in ratios])
        frac = float((r > 1).mean())
        print("%-34s %-22s dropped k beyond the gate in %.1f %% of %d outputs" % (name, entry, 100 * frac, r.size))
        assert frac >= 0.95, (name, entry, frac)
    else:      # an integer product is 0 where an operand is 0 (2 of 17 values each): every other output must differ
        assert np.mean([np.isinf(x).mean() for x in ratios]) > 0.6


@pytest.mark.parametrize("entry", [R.F32G, R.X3G])
@pytest.mark.parametrize("name", _names(lambda c: c["group"] == "segments"))
def test_a_dropped_first_k_of_the_second_segment_is_refused(name, entry):
    ratios = _refused(name, entry, "seg2_first")
    if BY_NAME[name]["kind"] == "real":
        frac = float((ratios[0] > 1).mean())
        print(name, entry, "beyond the gate in %.1f %%" % (100 * frac))
        assert frac >= 0.95, (name, entry, frac)


@pytest.mark.parametrize("fault", ["no_lohi", "hi_only"])
@pytest.mark.parametrize("name", _names(lambda c: c["kind"] == "real" and plain(c)))
def test_a_missing_split_term_is_refused(name, fault):
    """lo*hi missing is ~1e-3 G, some 60 x the x3 bound; integer data cannot see it (lo = 0), which is why the real kind exists"""
    ratios = _refused(name, R.X3G, fault)
    w = R.worst(ratios)
    print(name, fault, "worst err / bound %.1f" % w)
    assert w > 10


FAULT_CASES = {
    "bias_shift": lambda c: any(p["bias"] for p in c["probs"]),
    "row_dup": lambda c: c["group"] == "edge" or c["name"].startswith("tile128"),
    "slab_missing": lambda c: any(p["reduce"] and R.mode_of(p) == 1 for p in c["probs"]),
    "atomic_twice": lambda c: any(p["atomic"] for p in c["probs"]),
    "pad_write": lambda c: c["group"] in ("single", "segments") and c["probs"][0]["wide"],
}
X3_FAULT_CASES = {
    "relu_from_out": lambda c: c["name"].startswith("dact1"),
    "colsum_short": lambda c: c["name"].startswith("dact"),
    "plane_unswizzled": lambda c: any(p["planes"] for p in c["probs"]),
    "pack_no_rebase": lambda c: c["name"].startswith("pack-"),
}


@pytest.mark.parametrize("fault", list(FAULT_CASES))
def test_structural_faults_are_refused_on_both_kernels(fault):
    names = _names(FAULT_CASES[fault])
    assert len(names) >= 4, fault
    for name in names:
        for entry in (R.F32G, R.X3G):
            _refused(name, entry, fault)


@pytest.mark.parametrize("fault", list(X3_FAULT_CASES))
def test_epilogue_faults_are_refused(fault):
    names = _names(X3_FAULT_CASES[fault])
    assert len(names) >= 4, fault
    for name in names:
        _refused(name, R.X3G, fault)


def test_every_fault_is_planted_somewhere():
    planted = {"k_tail", "seg2_first", "no_lohi", "hi_only"} | set(FAULT_CASES) | set(X3_FAULT_CASES)
    assert planted == set(R.FAULTS)


def test_the_x3_gate_needs_several_products():
    """Why a real-valued accumulator contracts at least REAL_KMIN products (gemm_ref's docstring): with ONE product the correct
    split arithmetic hi*hi + hi*lo + lo*hi leaves the x3 gate's 2^-16 |a b| (bf16 rounds to 8 bits, so a lo rounding alone reaches
    2^-16), while it stays inside the rigorous 3 * 2^-16 |a b|.  Measured on 2^20 standard normal products: worst 1.6 * 2^-16."""
    rng = np.random.RandomState(3)
    a, b = rng.standard_normal(1 << 20).astype(R.F), rng.standard_normal(1 << 20).astype(R.F)
    (_, ah), (_, bh) = R._bf(a), R._bf(b)
    (_, al), (_, bl) = R._bf(a - ah), R._bf(b - bh)
    three = ah.astype(np.float64) * bh + ah.astype(np.float64) * bl + al.astype(np.float64) * bh
    rel = np.abs(three - a.astype(np.float64) * b) / np.abs(a.astype(np.float64) * b)
    print("worst relative error of one split product: %.2f * 2^-16" % (rel.max() * 2 ** 16))
    assert 2.0 ** -16 < rel.max() <= 3.01 * 2.0 ** -16
    assert np.abs(a - ah).max() > 0 and (np.abs(a - ah) <= 2.0 ** -8 * np.abs(a)).all()


def test_the_case_table_reaches_every_path():
    """from the restated launcher arithmetic (gemm_ref.paths), not from the kernel"""
    pa = {c["name"]: R.paths(c) for c in CASES}
    for kind in ("int", "real"):
        for L in (0, 1, 2):
            mine = {n: v for n, v in pa.items() if BY_NAME[n]["layout"] == L and BY_NAME[n]["kind"] == kind}
            assert {v["f32_tile"] for v in mine.values()} == {64, 128}                      # both fp32 tiles
            at = {v["big"]: v["f32_tile"] for v in mine.values()}
            assert at[191] == 64 and at[192] == 128                                        # on either side of the switch
            assert {v["ring"] for v in mine.values()} == {1, 2}                            # both ring forms
            assert {max(v["stages"]) for v in mine.values()} >= {1, 2, 3, 4, 5}            # the ring switch at 4 | 5, odd totals
            # launches whose problems disagree on the ring: one stage beside four (ring of 2) and beside five (ring of 1)
            assert mine["mix-1+4-stages-L%d-%s" % (L, kind)]["stages"] == [1, 4] and mine["mix-1+4-stages-L%d-%s" % (L, kind)]["ring"] == 2
            assert mine["mix-1+5-stages-L%d-%s" % (L, kind)]["stages"] == [1, 5] and mine["mix-1+5-stages-L%d-%s" % (L, kind)]["ring"] == 1
            g10 = mine["group10-L%d-%s" % (L, kind)]
            assert g10["nprob"] == R.MAXP and g10["nlive"] == 8 and g10["nwg_x3"] % 8 and g10["nwg_f32"] % 8
            assert len(set(-(-p["M"] // 64) * -(-p["N"] // 64) for p in BY_NAME["group10-L%d-%s" % (L, kind)]["probs"])) >= 5
            if kind == "real":
                continue
            assert {tuple(v["nseg"]) for v in mine.values()} >= {(1,), (2,), (3,)}
            # segments of unequal K flatten to 2 + 1 + 3, 1 + 1 + 1, 4 + 1 and 1 + 1 + 1 stages
            assert [pa["seg-%s-L%d-%s" % (k, L, kind)]["stages"] for k in ("68+4+132", "4+4+4", "256+4", "64+64+64")] == [[6], [3], [5], [3]]
    # split K: requested > effective, and the collapse to one chunk
    assert [R.eff_split(*x) for x in ((96, 7), (40, 3), (28, 3), (4100, 5))] == [(32, 3), (32, 2), (32, 1), (832, 5)]
    assert R.mode_of(R.P(65, 68, 28, splitk=3)) == 0 and R.mode_of(R.P(65, 68, 28, splitk=3, atomic=1)) == 2
    # a real-valued accumulator contracts 15 .. 300 products; everything shorter or longer is integer
    for c in CASES:
        for p in c["probs"]:
            if p["M"] > 0 and p["N"] > 0:
                assert R.kind_of(c, p) == "int" or (R.products(p) >= R.REAL_KMIN and sum(p["K"]) <= R.REAL_KMAX), c["name"]
    # the tcar_gemm_f32 entry runs wherever a case is one plain problem
    assert sum(R.F32 in R.entries(c) for c in CASES) >= 30
