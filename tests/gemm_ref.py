"""Cases, references, gates and a numpy stand-in of the small-GEMM tests (test_gemm_ref.py on the CPU, test_gpu_gemm_small.py on
the GPU): csrc/gemm_f32.hip, i.e. `gemm_f32_kernel` (tcar_gemm_f32 / tcar_gemm_f32_grouped), its split-bf16 twin `gemm_x3_kernel`
(tcar_gemm_x3_grouped) and tcar_splitk_reduce.

A CASE is one grouped launch: a layout, a data kind and a list of problems (`P`).  `build` draws its operands and embeds them in
buffers whose every other element is poison: NaN in the operand columns past M / N / K up to the leading dimension and in two rows
past the logical count, a sentinel in every C, slab, plane, pack and colsum element the call must not write (rows >= M, columns in
[N, ldc), slabs past the effective count).  A NaN that reached a stored element, or a store outside the logical matrix, fails the
case whatever the arithmetic does.

Two data kinds:
  int   operands, bias, dact_y and the initial C are integers in [-8, 8].  Every product and every partial sum is an integer below
        2^24 (`build` asserts it on the magnitudes): exact in fp32 and in the bf16 hi planes (lo = 0), in ANY summation order, so
        plain, slab, slab + reduce and atomic results, relu, both dact forms and colsum equal the int64 reference BIT FOR BIT.  A
        dropped, duplicated or misplaced element cannot hide behind a tolerance.  Every structural case has this kind.
  real  standard normal fp32, 15 <= logical K <= 300.  Gate: the forward bound on the reference-side magnitude
        G = |A| |B| (+ |bias| + |C0|), all in fp64:
            fp32 kernel   |got - want| <= (K + 4) 2^-24 G
            x3 kernel     that + 2^-16 G   (per product: the dropped lo*lo term <= 2^-18, the two lo roundings <= 2^-18 each)
        relu keeps the bound (1-Lipschitz); dact = 1 keeps it, and where the fp32 dact_y is within the bound of 0 either branch
        passes; dact = 2 multiplies it by |1 - y^2| <= 1; tanh keeps it (|tanh'| <= 1) plus 4 * 2^-24 for the device tanhf.
        K is what one accumulator contracts (the chunk of a slab).  colsum and the slab fold add the rounding of their own sums,
        (terms + 4) 2^-24 of the summed magnitudes.  The project's `close` (1e-3, 2e-5 * scale) is asserted on top.
        dact_y of dact = 2 is tanh(n), n standard normal clipped to |n| <= 3: the factor 1 - y^2 is itself rounded in fp32
        (<= 2^-24 |acc|), which the bound above does not name; with |1 - y^2| >= 0.0098 that rounding is below a fifth of the
        2^-16 G |1 - y^2| term.
        B of a tanh problem is standard normal times 1 / (2 sqrt(K)), the size of a layer's weights: with unit B the
        pre-activation has sigma = sqrt(K), five outputs in six saturate and hide the accumulator, and `close`'s absolute term,
        2e-5 on outputs of scale 1, lies below the x3 bound 1.5e-5 G of a correct kernel once G > 1.3 (G = 23 at K = 36).
  Why K <= 300: a fault that removes ONE k element must exceed the gate in >= 95 % of the outputs (test_gemm_ref.py); at
  K = 1,000 it does in 86 %, at K = 5,000 in 15 %.  Long K belongs to the int kind.
  Why K >= 15: the 2^-18 figures above are those of a 9-bit significand.  bf16 keeps 8 bits, its unit roundoff is 2^-8: |lo| <=
  2^-8 |x|, each lo rounding <= 2^-16 |x| and lo*lo <= 2^-16 |a b|, so ONE product of a correct split-bf16 kernel can be off by
  3 * 2^-16 |a b|, three times the x3 gate.  The gate is kept as stated; it holds because the K signed errors do not align: the
  stand-in reaches 0.70 of it at K = 16, 0.54 at 17, 0.42 at 28, 0.36 at 36, 0.07 at 260, but 1.1 .. 1.4 where an accumulator contracts 1,
  2, 4 or 5 products (test_the_x3_gate_needs_several_products).  A problem whose stored accumulators contract fewer than 15
  products (tiny K, the 4-deep last chunk of a split) is therefore drawn from the int kind inside a real-valued case too
  (`kind_of`), like the ballast: it is held bit for bit, not dropped.

Planes: for rows < M and columns [plane_col0, plane_col0 + N), hi == bf16(C_got) and lo == bf16(C_got - hi) bit for bit at the
`_kb32_index` offsets; the packed pair likewise with the columns outside [pack_c0, pack_c1) rebased past the gap; every other
element of the four buffers keeps its sentinel.

`standin` restates both kernels in numpy (fp32 multiply-add per k; bf16 split through torch.bfloat16, lo*hi + hi*lo + hi*hi in
k16 steps, fp32 accumulate) with the epilogues, and can plant one FAULT; `judge` is the one checker of stand-in and device output.
`paths` restates the launchers' tile / stage / ring / split arithmetic so that a CPU test can assert what the table reaches.

Not reachable through the C ABI, left to the step-level tests: TcarOpt::hi_only and the completion flag."""
import zlib

import numpy as np
import torch

from gpu_util import _kb32_index, close

F = np.float32
U = 2.0 ** -24
X3_EXTRA = 2.0 ** -16
TANH_ABS = 4 * U
SENT = F(-777.25)              # C / slab / colsum elements the call must not write
SENT16 = np.int16(0x7FC1)      # plane / pack elements (a bf16 NaN with a payload)
BK, MAXP, X3_ONESHOT = 32, 10, 4
F32, F32G, X3G = "tcar_gemm_f32", "tcar_gemm_f32_grouped", "tcar_gemm_x3_grouped"
FAULTS = ("k_tail", "seg2_first", "no_lohi", "hi_only", "bias_shift", "row_dup", "slab_missing", "atomic_twice", "relu_from_out",
          "colsum_short", "plane_unswizzled", "pack_no_rebase", "pad_write")


def r4(x):
    return (x + 3) // 4 * 4


# ------------------------------------------------------------------------------------------------ launcher arithmetic, restated
def eff_split(K, splitk):
    """fill_prob / tcar_gemm_splitk_effective: (kchunk, number of chunks) — K is cut in multiples of 32"""
    splitk = max(1, splitk)
    kchunk = (K + splitk - 1) // splitk
    kchunk = (kchunk + BK - 1) // BK * BK
    return kchunk, (K + kchunk - 1) // kchunk


def mode_of(p):
    """0 plain, 1 slabs, 2 atomics (fill_prob: a split that collapses to one chunk is plain, or atomic where asked)"""
    _, S = eff_split(max(p["K"]), p["splitk"])
    if p["splitk"] <= 1:
        return 0
    return 2 if p["atomic"] else (1 if S > 1 else 0)


def products(p):
    """the fewest products one stored accumulator of this problem contracts (the last chunk of a slab split; the whole K otherwise)"""
    kchunk, S = eff_split(max(p["K"]), p["splitk"])
    return p["K"][0] - (S - 1) * kchunk if mode_of(p) == 1 else sum(p["K"])


def kind_of(case, p):
    """data kind of one problem: the case's, but int where the problem says so (the ballast) and where a real-valued accumulator
    would contract fewer than REAL_KMIN or more than REAL_KMAX products"""
    if p["kind"] or case["kind"] == "int" or p["M"] <= 0 or p["N"] <= 0:
        return p["kind"] or case["kind"]
    return "real" if REAL_KMIN <= products(p) and sum(p["K"]) <= REAL_KMAX else "int"


def paths(case):
    """what launch_layout / launch_x3 decide for this launch"""
    live = [p for p in case["probs"] if p["M"] > 0 and p["N"] > 0]
    split = [eff_split(max(p["K"]), p["splitk"]) for p in live]
    big = sum(-(-p["M"] // 128) * -(-p["N"] // 128) * s for p, (_, s) in zip(live, split))
    T = 128 if big >= 192 else 64
    stages = [sum((min(k, kc) + 63) // 64 for k in p["K"]) for p, (kc, _) in zip(live, split)]
    return {"f32_tile": T, "big": big, "stages": stages, "ring": 2 if max(stages) <= X3_ONESHOT else 1,
            "nseg": sorted({len(p["K"]) for p in live}), "nprob": len(case["probs"]), "nlive": len(live),
            "nwg_f32": sum(-(-p["M"] // T) * -(-p["N"] // T) * s for p, (_, s) in zip(live, split)),
            "nwg_x3": sum(-(-p["M"] // 64) * -(-p["N"] // 64) * s for p, (_, s) in zip(live, split))}


# ------------------------------------------------------------------------------------------------------------------ the cases
def P(M, N, K, wide=False, bias=False, act=0, beta=0, splitk=1, atomic=0, reduce=False, dact=0, colsum=False, planes=None, pack=None,
      kind=None, tag=""):
    """one problem.  K: int or tuple (segments); planes = (plane_inner, plane_col0); pack = (pack_inner, pack_c0, pack_c1);
    reduce: fold the slabs with tcar_splitk_reduce; kind: overrides the case's data kind (the int ballast of a real case)"""
    K = (K,) if isinstance(K, int) else tuple(K)
    return dict(M=M, N=N, K=K, wide=wide, bias=bias, act=act, beta=beta, splitk=splitk, atomic=atomic, reduce=reduce, dact=dact,
                colsum=colsum, planes=planes, pack=pack, kind=kind, tag=tag or "%dx%dx%s" % (M, N, "+".join(map(str, K))))


def _case(group, name, layout, kind, probs):
    return dict(group=group, name="%s-L%d-%s" % (name, layout, kind), layout=layout, kind=kind, probs=probs)


EDGE_MN = [(1, 130), (3, 129), (63, 65), (64, 64), (65, 63), (129, 3), (130, 1), (130, 129), (65, 65), (1, 1)]
EDGE_K = {0: (4, 28, 36, 60, 64, 68, 128, 132, 256, 260, 320), 1: (4, 28, 36, 60, 64, 68, 128, 132, 256, 260, 320),
          2: (1, 2, 15, 16, 17, 31, 33, 63, 65, 129, 257)}
SEG_K = ((68, 4, 132), (4, 4, 4), (256, 4), (64, 64, 64))
REAL_KMIN, REAL_KMAX = 15, 300


def _tile128(layout, kind, target):
    """problems near 130 x 129 x 36 plus a one-element atomic split-K ballast that brings the launch to `target` 128 x 128 tiles
    (launch_layout switches at 192); the ballast is int data in either kind (its K is far beyond 300)"""
    o = 1 if layout == 2 else 0           # layout 2 takes any K
    ps = [P(130, 129, 36 + o, wide=True, tag="plain"), P(129, 130, 36 + o, bias=True, act=1, tag="bias+relu")]
    if kind == "real":
        ps.append(P(130, 129, 36 + o, bias=True, act=2, wide=True, tag="bias+tanh"))
    ps += [P(65, 129, 68 + o, beta=1, tag="beta"), P(130, 132, 96 + o, splitk=2, reduce=True, tag="slab"),
           P(129, 130, 96 + o, splitk=3, atomic=1, wide=True, tag="atomic")]
    others = paths(dict(probs=ps))["big"]
    sk = target - others
    return [P(1, 1, 32 * sk, splitk=sk, atomic=1, kind="int", tag="ballast")] + ps


def all_cases():
    cs = []
    for kind in ("int", "real"):
        for L in (0, 1, 2):
            o = 1 if L == 2 else 0
            for K in EDGE_K[L]:
                if kind == "real" and not REAL_KMIN <= K <= REAL_KMAX:
                    continue
                cs.append(_case("edge", "edge-K%d" % K, L, kind, [P(M, N, K, wide=bool(i & 1)) for i, (M, N) in enumerate(EDGE_MN)]))
            for M, N, K in ((130, 129, 36 + o), (3, 65, 1 if L == 2 else 4), (65, 130, 257 if L == 2 else 260)):
                cs.append(_case("single", "single-%dx%dx%d" % (M, N, K), L, kind, [P(M, N, K, wide=True)]))
            cs.append(_case("single", "single-bias-relu-beta", L, kind, [P(65, 67, 36 + o, bias=True, act=1, beta=1)]))
            cs.append(_case("tile128", "tile128-at192", L, kind, _tile128(L, kind, 192)))
            cs.append(_case("tile128", "tile64-at191", L, kind, _tile128(L, kind, 191)))
            for Ks in SEG_K:
                cs.append(_case("segments", "seg-" + "+".join(map(str, Ks)), L, kind, [P(70, 66, Ks, wide=True)]))
            ks = [36, 4, 8, 68, 132, 12, 4, 64, 28, 8]
            mn = [(130, 129), (1, 1), (0, 64), (65, 3), (64, 64), (3, 0), (129, 130), (63, 65), (200, 70), (5, 7)]
            cs.append(_case("groups", "group10", L, kind, [P(M, N, k + o, wide=bool(i & 1)) for i, ((M, N), k) in enumerate(zip(mn, ks))]))
            cs.append(_case("groups", "mix-1+4-stages", L, kind, [P(65, 63, 64), P(70, 66, 256, wide=True)]))
            cs.append(_case("groups", "mix-1+5-stages", L, kind, [P(65, 63, 64), P(70, 66, 257 if L == 2 else 260, wide=True)]))
            # split K: requested > effective (96 / 7 -> 3, 40 / 3 -> 2), a split that collapses to ONE chunk (28 / 3), long K in layout 2
            splits = [(96, 7), (40, 3), (28, 3)] if kind == "int" else [(96, 7)]
            if L == 2 and kind == "int":
                splits.append((4100, 5))
            for K, s in splits:
                cs.append(_case("splitk", "slab-K%d-s%d" % (K, s), L, kind, [P(65, 68, K, splitk=s, reduce=True, wide=True)]))
                cs.append(_case("splitk", "atomic-K%d-s%d" % (K, s), L, kind, [P(65, 68, K, splitk=s, atomic=1)]))
            if L == 2:
                continue
            # fused epilogues of the x3 kernel (the fp32 entry runs the same problems without them)
            for d in (1, 2):
                cs.append(_case("epilogue", "dact%d" % d, L, kind, [P(M, 67, 36, dact=d, colsum=c, wide=bool(c)) for M in (65, 130) for c in (False, True)]))
            cs.append(_case("epilogue", "planes", L, kind, [P(130, 65, 36, planes=(96, 7)), P(130, 65, 36, bias=True, act=1, planes=(128, 63), wide=True)]))
            cs.append(_case("epilogue", "pack", L, kind, [P(130, 65, 36, planes=(96, 7), pack=(64, 20, 40), tag="gap inside"),
                                                          P(130, 65, 36, planes=(96, 7), pack=(96, 30, 30), tag="empty gap"),
                                                          P(130, 65, 36, planes=(96, 7), pack=(32, 0, 96), tag="gap covers all")]))
            cs.append(_case("epilogue", "bias-act-planes-pack", L, kind,
                            [P(130, 65, 68, bias=True, act=2 if kind == "real" else 1, planes=(96, 16), pack=(64, 32, 64), wide=True)]))
            cs.append(_case("epilogue", "beta", L, kind, [P(65, 67, 36, beta=1), P(130, 3, 132, beta=1, bias=True, act=1, wide=True)]))
    # a real-valued case none of whose problems can be real-valued (kind_of) would repeat its integer twin
    return [c for c in cs if c["kind"] == "int" or any(kind_of(c, p) == "real" for p in c["probs"])]


def entries(case):
    """the C entry points a case runs through: both grouped ones, and tcar_gemm_f32 where it is a single one-segment problem"""
    ps = case["probs"]
    one = len(ps) == 1 and len(ps[0]["K"]) == 1 and not ps[0]["atomic"] and not ps[0]["dact"] and not ps[0]["planes"]
    return ([F32] if one else []) + [F32G, X3G]


# ---------------------------------------------------------------------------------------------------------------- the operands
def _draw(rng, kind, shape):
    return rng.randint(-8, 9, size=shape).astype(F) if kind == "int" else rng.standard_normal(shape).astype(F)


def _embed(x, ld):
    buf = np.full((x.shape[0] + 2, ld), np.nan, dtype=F)
    buf[:x.shape[0], :x.shape[1]] = x
    return buf


def build(case):
    """-> one dict per problem: the poisoned buffers (A, B, C, bias, y, colsum, plane_*, pack_*: what the device receives) and the
    logical operands a [M, K], b [K, N] per segment, bias, y, c0, colsum0 (what the references read)"""
    rng = np.random.RandomState(zlib.crc32(case["name"].encode()) & 0x7FFFFFFF)
    L, out = case["layout"], []
    for p in case["probs"]:
        kind = kind_of(case, p)
        M, N = p["M"], p["N"]
        b = dict(kind=kind, mode=mode_of(p))
        if M <= 0 or N <= 0:                                   # an empty problem: dropped by the entry point, nothing is touched
            b.update(A=[np.full((2, 4), np.nan, F)], B=[np.full((2, 4), np.nan, F)], lda=[4], ldb=[4], C=np.full((2, 4), SENT, F), ldc=4)
            out.append(b)
            continue
        b["a"], b["b"], b["A"], b["B"], b["lda"], b["ldb"] = [], [], [], [], [], []
        for s, K in enumerate(p["K"]):
            w = 8 if (p["wide"] ^ bool(s & 1)) else 0
            a, bm = _draw(rng, kind, (M, K)), _draw(rng, kind, (K, N))
            if p["act"] == 2 and kind == "real":               # weights of a tanh layer: pre-activations of ~N(0, 1/4) + bias
                bm = (bm * F(0.5 / np.sqrt(sum(p["K"])))).astype(F)
            A = _embed(a, r4(K) + w) if L != 2 else _embed(a.T, r4(M) + w)
            Bm = _embed(bm.T, r4(K) + w) if L == 1 else _embed(bm, r4(N) + w)
            b["a"].append(a); b["b"].append(bm); b["A"].append(A); b["B"].append(Bm)
            b["lda"].append(A.shape[1]); b["ldb"].append(Bm.shape[1])
        _, S = eff_split(max(p["K"]), p["splitk"])
        b["S"] = S if b["mode"] == 1 else 1
        b["ldc"] = r4(N) + (4 if p["wide"] else 0)
        b["C"] = np.full((b["S"] * M + 2, b["ldc"]), SENT, dtype=F)
        b["c0"] = None
        if p["beta"] or b["mode"] == 2:
            b["c0"] = _draw(rng, kind, (M, N))
            b["C"][:M, :N] = b["c0"]
        b["bias"] = b["biasbuf"] = None
        if p["bias"]:
            b["bias"] = _draw(rng, kind, (N,))
            b["biasbuf"] = np.concatenate([b["bias"], np.full(2, np.nan, F)])
        if p["reduce"]:
            b["out"] = np.full((M + 2, b["ldc"]), SENT, dtype=F)
        if p["dact"]:
            y = _draw(rng, kind, (M, N))
            if p["dact"] == 2 and kind == "real":
                y = np.tanh(np.clip(y, -3, 3)).astype(F)
            b["y"], b["Y"] = y, _embed(y, r4(N) + 4)
            if p["colsum"]:
                b["colsum0"] = _draw(rng, kind, (N,))
                b["colsum"] = np.concatenate([b["colsum0"], np.full(2, SENT, F)])
        if p["planes"]:
            rp = (M + 127) // 128 * 128
            b["plane_hi"], b["plane_lo"] = (np.full(rp * p["planes"][0] + 32, SENT16, dtype=np.int16) for _ in range(2))
            if p["pack"]:
                b["pack_hi"], b["pack_lo"] = (np.full(rp * p["pack"][0] + 32, SENT16, dtype=np.int16) for _ in range(2))
        if kind == "int":      # every partial sum below 2^24, whatever the order
            g = sum(np.abs(a.astype(np.float64)) @ np.abs(bm.astype(np.float64)) for a, bm in zip(b["a"], b["b"]))
            g = g + (np.abs(b["bias"]) if p["bias"] else 0) + (np.abs(b["c0"]) if b["c0"] is not None else 0)
            if p["dact"] == 2:
                g = g * np.abs(1 - b["y"].astype(np.float64) ** 2)
            assert g.max() < 2 ** 24 and (not p["colsum"] or (g.sum(0) + np.abs(b["colsum0"])).max() < 2 ** 24), (case["name"], p["tag"])
        out.append(b)
    return out


def _x3_fields(p, entry):
    """the fused-epilogue fields are set for the x3 entry only"""
    x3 = entry == X3G
    return (p["dact"] if x3 else 0, bool(p["colsum"]) and x3 and bool(p["dact"]), p["planes"] if x3 else None, p["pack"] if x3 else None)


# -------------------------------------------------------------------------------------------------------------- the references
def _bf(x):
    """fp32 -> (bf16 bit patterns as int16, the bf16 values as fp32), round to nearest even"""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=F)).to(torch.bfloat16)
    return t.view(torch.int16).numpy().copy(), t.to(torch.float32).numpy()


def expect(p, b, entry):
    """fp64 (exact for int data) reference of one problem -> dict: want / G [S, M, N], K of the bound, y-branch alternative, colsum"""
    dact, colsum, _, _ = _x3_fields(p, entry)
    a64 = [a.astype(np.float64) for a in b["a"]]
    b64 = [x.astype(np.float64) for x in b["b"]]
    kchunk, S = eff_split(max(p["K"]), p["splitk"])
    r = dict(alt=None, factor=None, tanh=False)
    if b["mode"] == 1:
        sl = [slice(s * kchunk, min(p["K"][0], (s + 1) * kchunk)) for s in range(S)]
        r["want"] = np.stack([a64[0][:, s] @ b64[0][s] for s in sl])
        r["G"] = np.stack([np.abs(a64[0][:, s]) @ np.abs(b64[0][s]) for s in sl])
        r["K"] = kchunk
        return r
    z = sum(a @ x for a, x in zip(a64, b64))
    G = sum(np.abs(a) @ np.abs(x) for a, x in zip(a64, b64))
    r["K"] = sum(p["K"])
    if b["mode"] == 2:
        z, G = z + b["c0"], G + np.abs(b["c0"])
    else:
        if p["bias"]:
            z, G = z + b["bias"], G + np.abs(b["bias"].astype(np.float64))
        if p["act"] == 1:
            z = np.maximum(z, 0)
        elif p["act"] == 2:
            z, r["tanh"] = np.tanh(z), True
        if dact == 1:
            y = b["y"].astype(np.float64)
            r["alt"], r["y"] = np.where(y > 0, 0.0, z), y
            z = np.where(y > 0, z, 0.0)
        elif dact == 2:
            r["factor"] = 1 - b["y"].astype(np.float64) ** 2
            z = z * r["factor"]
        if colsum:
            r["colsum_pre"] = z
        if p["beta"]:
            z, G = z + b["c0"], G + np.abs(b["c0"])
    r["want"], r["G"] = z[None], G[None]
    return r


def bound_of(r, entry):
    e = ((r["K"] + 4) * U + (X3_EXTRA if entry == X3G else 0.0)) * r["G"]
    if r["factor"] is not None:
        e = e * np.abs(r["factor"])
    return e + (TANH_ABS if r["tanh"] else 0.0)


def plane_expect(init, c_got, M, N, inner, col_of):
    """the full hi / lo buffers a correct call leaves: sentinel but for (row < M, col_of[n] >= 0) at the KB32 offsets"""
    hi_bits, hi = _bf(c_got)
    lo_bits, _ = _bf(c_got.astype(F) - hi)
    idx = _kb32_index(M, inner)
    eh, el = init.copy(), init.copy()
    keep = col_of >= 0
    o = idx[:, col_of[keep]]
    eh[o], el[o] = hi_bits[:, keep], lo_bits[:, keep]
    return eh, el


def pack_cols(N, col0, c0, c1):
    """packed-plane column of every logical column (-1: inside the gap)"""
    g = col0 + np.arange(N)
    return np.where(g < c0, g, np.where(g >= c1, g - (c1 - c0), -1))


# -------------------------------------------------------------------------------------------------------------------- the judge
def judge(case, built, outs, entry):
    """-> (failures: list of str, ratios: one array err / bound over the logical outputs per live problem; inf = an inexact int)"""
    fails, ratios = [], []
    for i, (p, b, o) in enumerate(zip(case["probs"], built, outs)):
        tag = "%s %s [%d %s]" % (case["name"], entry, i, p["tag"])
        M, N = p["M"], p["N"]
        if M <= 0 or N <= 0:
            if not np.array_equal(o["C"], b["C"]):
                fails.append(tag + ": an empty problem wrote")
            continue
        dact, colsum, planes, pack = _x3_fields(p, entry)
        r = expect(p, b, entry)
        S, ldc = b["S"], b["ldc"]
        got_all = o["C"]
        inside = np.zeros(got_all.shape, dtype=bool)
        inside[:S * M, :N] = True
        if not np.array_equal(got_all[~inside], b["C"][~inside]):
            fails.append(tag + ": wrote outside the logical C (rows >= M, columns [N, ldc) or slabs past the effective count)")
        got = got_all[:S * M].reshape(S, M, ldc)[:, :, :N]

        def gate(name, g, want, bnd, alt=None, do_close=True):
            if b["kind"] == "int":
                ok = g == want.astype(F)
                ratio = np.where(ok, 0.0, np.inf)
            else:
                err = np.abs(g.astype(np.float64) - want)
                if alt is not None:
                    err = np.where(np.abs(r["y"]) <= bnd[0], np.minimum(err, np.abs(g.astype(np.float64) - alt)), err)
                with np.errstate(invalid="ignore", divide="ignore"):
                    ratio = np.where(err == 0, 0.0, err / bnd)
                ratio = np.where(np.isnan(ratio), np.inf, ratio)
                ok = ratio <= 1.0
                if do_close and (alt is None or not (np.abs(r["y"]) <= bnd[0]).any()):
                    try:
                        close(g, want, name=name)
                    except AssertionError as e:
                        fails.append("%s: close: %s" % (tag, e))
            if not ok.all():
                w = np.unravel_index(np.argmax(ratio), ratio.shape)
                fails.append("%s: %s: %d / %d beyond the %s, worst err / bound %.3g at %s (got %r, want %r)" % (
                    tag, name, (~ok).sum(), ok.size, "exact integer" if b["kind"] == "int" else "bound", ratio[w], w, g[w], want[w]))
            return ratio

        bnd = bound_of(r, entry)
        ratios.append(gate("C", got, r["want"], bnd, alt=None if r["alt"] is None else r["alt"][None]))
        if p["reduce"]:
            go = o["out"]
            ins = np.zeros(go.shape, dtype=bool)
            ins[:M, :N] = True
            if not np.array_equal(go[~ins], b["out"][~ins]):
                fails.append(tag + ": the fold wrote outside [M, N]")
            mag = np.abs(r["want"]).sum(0)
            ratios.append(gate("fold", go[:M, :N], r["want"].sum(0), bnd.sum(0) + (S + 4) * U * mag))
        if colsum:
            gc = o["colsum"]
            if not np.array_equal(gc[N:], b["colsum"][N:]):
                fails.append(tag + ": colsum written past N")
            pre = r["colsum_pre"]
            cb = (bnd[0] if not p["beta"] else bound_of(dict(r, G=r["G"] - np.abs(b["c0"])), entry)[0]).sum(0)
            mag = np.abs(pre).sum(0) + np.abs(b["colsum0"])
            ratios.append(gate("colsum", gc[:N], pre.sum(0) + b["colsum0"], cb + (M + 4) * U * mag, do_close=False))
        if planes:
            inner, col0 = planes
            eh, el = plane_expect(b["plane_hi"], got[0], M, N, inner, col0 + np.arange(N))
            if not (np.array_equal(o["plane_hi"], eh) and np.array_equal(o["plane_lo"], el)):
                fails.append("%s: planes differ from bf16 hi / lo of the stored C at the KB32 offsets in %d + %d elements" % (
                    tag, (o["plane_hi"] != eh).sum(), (o["plane_lo"] != el).sum()))
            if pack:
                eh, el = plane_expect(b["pack_hi"], got[0], M, N, pack[0], pack_cols(N, col0, pack[1], pack[2]))
                if not (np.array_equal(o["pack_hi"], eh) and np.array_equal(o["pack_lo"], el)):
                    fails.append("%s: packed planes differ in %d + %d elements" % (tag, (o["pack_hi"] != eh).sum(), (o["pack_lo"] != el).sum()))
    return fails, ratios


def worst(ratios):
    return max([float(r.max()) for r in ratios if r.size] or [0.0])


def check(case, built, outs, entry):
    fails, ratios = judge(case, built, outs, entry)
    assert not fails, "\n".join(fails)
    return worst(ratios)


# ------------------------------------------------------------------------------------------------------------------ the stand-in
def _mac_f32(acc, a, bm):
    for k in range(a.shape[1]):
        acc += a[:, k:k + 1] * bm[k:k + 1, :]


def _mac_x3(acc, a, bm, fault):
    (_, ah), (_, bh) = _bf(a), _bf(bm)
    (_, al), (_, bl) = _bf(a - ah), _bf(bm - bh)
    for k0 in range(0, a.shape[1], 16):
        s = slice(k0, k0 + 16)
        if fault not in ("no_lohi", "hi_only"):
            acc += al[:, s] @ bh[s]
        if fault != "hi_only":
            acc += ah[:, s] @ bl[s]
        acc += ah[:, s] @ bh[s]


def reduce_standin(slabs, S, M, N, out):
    """tcar_splitk_reduce: slabs [S, M, ld] summed in slab order, four columns at a time (N >> 2 groups)"""
    acc = np.zeros((M, N // 4 * 4), dtype=F)
    for s in range(S):
        acc += slabs[s * M:(s + 1) * M, :N // 4 * 4]
    out[:M, :N // 4 * 4] = acc


def standin(case, built, entry, fault=None):
    """numpy restatement of one launch (and of the fold) -> outputs in the form `run_device` returns; fault: one of FAULTS"""
    mac = (lambda acc, a, bm: _mac_x3(acc, a, bm, fault)) if entry == X3G else _mac_f32
    outs = []
    for p, b in zip(case["probs"], built):
        o = {"C": b["C"].copy()}
        outs.append(o)
        M, N = p["M"], p["N"]
        if M <= 0 or N <= 0:
            continue
        dact, colsum, planes, pack = _x3_fields(p, entry)
        a, bm = [x.copy() for x in b["a"]], b["b"]
        if fault == "k_tail":
            a[-1][:, -1] = 0
        if fault == "seg2_first":
            a[1][:, 0] = 0
        kchunk, S = eff_split(max(p["K"]), p["splitk"])
        chunks = []
        for s in range(S):
            acc = np.zeros((M, N), dtype=F)
            for x, w in zip(a, bm):
                sl = slice(s * kchunk, min(x.shape[1], (s + 1) * kchunk))
                mac(acc, x[:, sl], w[sl])
            if fault == "row_dup":
                acc[M - 1] = acc[M - 2]
            chunks.append(acc)
        C = o["C"]
        if b["mode"] == 1:
            for s, acc in enumerate(chunks):
                C[s * M:(s + 1) * M, :N] = acc
        elif b["mode"] == 2:
            for acc in chunks + (chunks[:1] if fault == "atomic_twice" else []):
                C[:M, :N] += acc
        else:
            v = chunks[0]
            if p["bias"]:
                v = v + (np.roll(b["bias"], -1) if fault == "bias_shift" else b["bias"])
            if p["act"] == 1:
                v = np.maximum(v, F(0))
            elif p["act"] == 2:
                v = np.tanh(v)
            if dact == 1:
                v = np.where((v if fault == "relu_from_out" else b["y"]) > 0, v, F(0))
            elif dact == 2:
                v = v * (F(1) - b["y"] * b["y"])
            if colsum:
                o["colsum"] = b["colsum"].copy()
                rows = v[:M - 1] if fault == "colsum_short" else v
                for m in range(rows.shape[0]):
                    o["colsum"][:N] += rows[m]
            if p["beta"]:
                v = v + C[:M, :N]
            C[:M, :N] = v.astype(F)
        if fault == "pad_write":
            C[0, N] = F(1)
        if p["reduce"]:
            o["out"] = b["out"].copy()
            reduce_standin(C[M:] if fault == "slab_missing" else C, b["S"] - (fault == "slab_missing"), M, N, o["out"])
        if planes:
            inner, col0 = planes
            o["plane_hi"], o["plane_lo"] = plane_expect(b["plane_hi"], C[:M, :N], M, N, inner, col0 + np.arange(N))
            if fault == "plane_unswizzled":      # row 5, logical column 9: written without the xor of the 8-column group
                row, g = 5, col0 + 9
                good = int(_kb32_index(M, inner)[row, g])
                bad = ((row >> 7) * (inner // 32) + (g >> 5)) * 4096 + (row & 127) * 32 + (g & 31)
                assert bad != good
                for k in ("plane_hi", "plane_lo"):
                    o[k][bad], o[k][good] = o[k][good], b[k][good]
            if pack:
                cols = pack_cols(N, col0, pack[1], pack[2])
                if fault == "pack_no_rebase":
                    g = col0 + np.arange(N)
                    cols = np.where((g >= pack[2]) & (g < pack[0]), g, cols)
                o["pack_hi"], o["pack_lo"] = plane_expect(b["pack_hi"], C[:M, :N], M, N, pack[0], cols)
    return outs


# -------------------------------------------------------------------------------------------------------------------- the device
def run_device(lib, case, built, entry):
    """one launch of `entry` (+ tcar_splitk_reduce for the problems that ask for the fold) -> the output buffers as numpy arrays"""
    import ctypes as C
    from tcar_amd._lib import GemmDesc

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x)).cuda()

    def ptr(t):
        return t.data_ptr() if t is not None else None

    descs, keep = [], []
    for p, b in zip(case["probs"], built):
        dact, colsum, planes, pack = _x3_fields(p, entry)
        t = dict(A=[dev(x) for x in b["A"]], B=[dev(x) for x in b["B"]], C=dev(b["C"]))
        d = GemmDesc()
        d.nseg = len(p["K"])
        for s, K in enumerate(p["K"]):
            d.A[s], d.B[s], d.lda[s], d.ldb[s], d.K[s] = ptr(t["A"][s]), ptr(t["B"][s]), b["lda"][s], b["ldb"][s], K
        d.C, d.ldc, d.M, d.N = ptr(t["C"]), b["ldc"], p["M"], p["N"]
        d.act, d.beta, d.splitk, d.atomic = p["act"], p["beta"], p["splitk"], p["atomic"]
        if p["M"] > 0 and p["N"] > 0:
            if p["bias"]:
                t["bias"] = dev(b["biasbuf"])
                d.bias = ptr(t["bias"])
            if dact:
                t["Y"] = dev(b["Y"])
                d.dact, d.dact_y, d.ld_dact_y = dact, ptr(t["Y"]), b["Y"].shape[1]
                if colsum:
                    t["colsum"] = dev(b["colsum"])
                    d.colsum = ptr(t["colsum"])
            if planes:
                t["plane_hi"], t["plane_lo"] = dev(b["plane_hi"]), dev(b["plane_lo"])
                d.plane_hi, d.plane_lo, d.plane_inner, d.plane_col0 = ptr(t["plane_hi"]), ptr(t["plane_lo"]), planes[0], planes[1]
                if pack:
                    t["pack_hi"], t["pack_lo"] = dev(b["pack_hi"]), dev(b["pack_lo"])
                    d.pack_hi, d.pack_lo, d.pack_inner, d.pack_c0, d.pack_c1 = ptr(t["pack_hi"]), ptr(t["pack_lo"]), pack[0], pack[1], pack[2]
            if p["reduce"]:
                t["out"] = dev(b["out"])
        descs.append(d)
        keep.append(t)
    if entry == F32:
        (p,), (b,), (t,), d = case["probs"], built, keep, descs[0]
        rc = lib.tcar_gemm_f32(case["layout"], p["M"], p["N"], p["K"][0], C.c_void_p(d.A[0]), b["lda"][0], C.c_void_p(d.B[0]), b["ldb"][0],
                               C.c_void_p(d.C), b["ldc"], C.c_void_p(ptr(t.get("bias"))), p["act"], p["beta"], p["splitk"], None)
    else:
        rc = getattr(lib, entry)(case["layout"], len(descs), (GemmDesc * len(descs))(*descs), None)
    assert rc == 0, (case["name"], entry, rc)
    for p, b, t in zip(case["probs"], built, keep):
        if p["reduce"] and p["M"] > 0 and p["N"] > 0:
            S = lib.tcar_gemm_splitk_effective(p["K"][0], p["splitk"])        # the count the header tells the caller to fold
            assert S == b["S"], (case["name"], S, b["S"])
            rc = lib.tcar_splitk_reduce(C.c_void_p(ptr(t["C"])), S, p["M"], p["N"], b["ldc"], C.c_void_p(ptr(t["out"])), None)
            assert rc == 0, (case["name"], "tcar_splitk_reduce", rc)
    torch.cuda.synchronize()
    return [{k: v.cpu().numpy() for k, v in t.items() if k in ("C", "out", "colsum", "plane_hi", "plane_lo", "pack_hi", "pack_lo")}
            for t in keep]
