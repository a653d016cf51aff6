"""tcar_cand_scores at the op level (include/tcar_cand.h): the [B, C] gathered dots from fp32 rows and from KB32 planes against the fp64
dot of the very operands, and the bit-level promises — a score depends on the session row and the item alone."""
import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401

from cand_ref import bf16_values, kb32_plane
from gpu_util import _need_gpu, lib, ptr  # noqa: F401  (lib: fixture)

pytestmark = pytest.mark.gpu

N = 300                                            # three 128-row blocks of the catalog planes, the last one partial
SPECIAL = [0, 127, 128, N - 1]                     # both sides of a block edge, the first and the last row
EMPTY = [-1, N, -7]
SENTINEL = 12345.0
B0 = 2                                             # the rows [0, B0) and [B0, B) go through two calls as well


def _lists(rng, B, C):
    """[B, C] candidate lists: the special ids, repeats and the empty slots wherever C has room, at other slots in every row"""
    cand = rng.randint(0, N, (B, C)).astype(np.int32)
    for b in range(B):
        must = (SPECIAL + EMPTY + [SPECIAL[1], int(cand[b, 0])])[:C] if C > 1 else [SPECIAL[b % 4]]
        cand[b, rng.permutation(C)[:len(must)]] = must
    return cand


def _plane_t(x, K):
    return torch.from_numpy(kb32_plane(x, K).view(np.int16)).cuda().view(torch.bfloat16)


@pytest.mark.parametrize("mode", ["f32", "hi", "x3"])
@pytest.mark.parametrize("K,inner", [(100, 128), (832, 832)])
@pytest.mark.parametrize("B", [5, 130])
def test_scores_match_the_fp64_dot_and_depend_on_row_and_item_alone(lib, B, K, inner, mode):
    rng = np.random.RandomState(1000 * B + K + len(mode))
    P = 3 if mode == "x3" else 1
    if mode == "f32":
        a, e = (rng.standard_normal(s).astype(np.float32) for s in ((B, inner), (N, inner)))
        a[:, K:], e[:, K:] = np.nan, np.nan                                           # columns >= K are never read as scores
        exact = a[:, :K].astype(np.float64) @ e[:, :K].astype(np.float64).T
        mag = np.abs(a[:, :K]).astype(np.float64) @ np.abs(e[:, :K]).astype(np.float64).T
        at, et = torch.from_numpy(a).cuda(), torch.from_numpy(e).cuda()

        def run(cand_t, out_t, C, rows=slice(0, B)):
            nb = rows.stop - rows.start
            return lib.tcar_cand_scores(nb, C, N, K, ptr(at, rows.start * inner), inner, ptr(et), inner, None, None, 0, None, None, 0, 1,
                                        ptr(cand_t, rows.start * C), C, ptr(out_t, rows.start * (C + 4)), C + 4, None)
    else:
        ah, eh = bf16_values(rng, (B, inner), 1.0), bf16_values(rng, (N, inner), 1.0)
        al, el = bf16_values(rng, (B, inner), 2.0 ** -9), bf16_values(rng, (N, inner), 2.0 ** -9)
        d = lambda x, y: x[:, :K].astype(np.float64) @ y[:, :K].astype(np.float64).T
        exact = d(ah, eh) + (d(ah, el) + d(al, eh) if P == 3 else 0.0)
        mag = np.abs(ah[:, :K]).astype(np.float64) @ np.abs(eh[:, :K]).astype(np.float64).T
        pl = {"ah": _plane_t(ah, K), "al": _plane_t(al, K), "eh": _plane_t(eh, K), "el": _plane_t(el, K),
              "ah2": _plane_t(ah[B0:], K), "al2": _plane_t(al[B0:], K)}              # a second plane set: the rows [B0, B) as rows 0 ..

        def run(cand_t, out_t, C, rows=slice(0, B)):
            nb, second = rows.stop - rows.start, rows.start > 0
            lo = P == 3
            return lib.tcar_cand_scores(nb, C, N, K, None, 0, None, 0, ptr(pl["ah2" if second else "ah"]),
                                        ptr(pl["al2" if second else "al"]) if lo else None, inner, ptr(pl["eh"]),
                                        ptr(pl["el"]) if lo else None, inner, P, ptr(cand_t, rows.start * C), C,
                                        ptr(out_t, rows.start * (C + 4)), C + 4, None)
    bound = 2.0 * P * K * 2.0 ** -24 * mag                     # the worst case of ANY fp32 summation order of P K terms
    bits_of = {}                                               # (row, item) -> the bits of its score, over every list it appears in
    for C in (1, 7, 70):
        cand = _lists(rng, B, C)
        cand_t = torch.from_numpy(cand).cuda()
        outs = []
        for rows_list in ([slice(0, B)], [slice(0, B)], [slice(0, B0), slice(B0, B)]):
            out = torch.full((B, C + 4), SENTINEL, dtype=torch.float32, device="cuda")
            for rows in rows_list:
                assert run(cand_t, out, C, rows) == 0
            torch.cuda.synchronize()
            outs.append(out.cpu().numpy())
        got = outs[0]
        assert (got[:, C:] == SENTINEL).all()                                                           # (d)
        assert got.tobytes() == outs[1].tobytes(), "two runs differ"                                    # (e)
        assert got.tobytes() == outs[2].tobytes(), "the rows in two calls differ from one call"         # (b) the split of the rows
        live = (cand >= 0) & (cand < N)
        assert live.sum() and (~live).sum() >= (B if C >= 7 else 0)
        assert (got[:, :C][~live] == -np.inf).all()                                                     # (c)
        for b in range(B):
            for c in range(C):
                if not live[b, c]:
                    continue
                i, s = int(cand[b, c]), got[b, c]
                err = abs(float(s) - exact[b, i])
                assert err <= bound[b, i], (b, c, i, err, bound[b, i])                                  # (a)
                assert bits_of.setdefault((b, i), s.tobytes()) == s.tobytes(), (b, c, i, C)             # (b) slot, C, rest of the list
    assert len({i for _, i in bits_of} & set(SPECIAL)) == 4
