"""tcar_cand_scores_owned and tcar_cand_combine at the op level (include/tcar_retrieve_shard.h), exactly: the catalog planes of
tcar_cand_scores are cut into three shards at rows 256 and 512; every shard scores the slots whose rows it owns, and the combine of the
three parts must be the bits of ONE tcar_cand_scores call on the whole planes — the summation order of a dot depends on K and nsplit
alone, and the combine copies the owner's word."""
import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401

from cand_ref import bf16_values, kb32_plane
from gpu_util import lib, ptr  # noqa: F401  (lib: the fixture)

pytestmark = pytest.mark.gpu

N, K, INNER = 700, 100, 128                        # K, inner: the small geometry of test_gpu_cand_scores
EDGES = (0, 256, 512, N)
ROWS_PER_SHARD = 256
B = 5
SENTINEL = 12345.0
NEG_INF_BITS = np.float32(-np.inf).view(np.int32)


def _plane_t(x):
    return torch.from_numpy(kb32_plane(x, K).view(np.int16)).cuda().view(torch.bfloat16)


def _lists(rng, C):
    """repeats, -1, ids >= N, both sides of every shard border and the catalog's ends, ids of every shard in every row"""
    cand = rng.randint(0, N, (B, C)).astype(np.int32)
    must = [0, 255, 256, 511, 512, N - 1, -1, N, N + 300, -7, 255, 2 ** 31 - 1, -2 ** 31]
    for b in range(B):
        m = must[:C] if C > 1 else [must[b]]
        cand[b, rng.permutation(C)[:len(m)]] = m
    return cand


@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("C", [1, 7, 70, 1024])
def test_the_owners_scores_combine_into_the_whole_catalogs_bits(lib, nsplit, C):
    rng = np.random.RandomState(100 * C + nsplit)
    ah, eh = bf16_values(rng, (B, INNER), 1.0), bf16_values(rng, (N, INNER), 1.0)
    al, el = bf16_values(rng, (B, INNER), 2.0 ** -9), bf16_values(rng, (N, INNER), 2.0 ** -9)
    lo = nsplit == 3
    pa = (_plane_t(ah), _plane_t(al))
    whole = (_plane_t(eh), _plane_t(el))
    shards = [(_plane_t(eh[a:b]), _plane_t(el[a:b])) for a, b in zip(EDGES, EDGES[1:])]
    cand = _lists(rng, C)
    cand_t = torch.from_numpy(cand).cuda()
    ld = C + 4

    def scores(e, n, id0, out, off=0):
        args = (B, C, n, K, None, 0, None, 0, ptr(pa[0]), ptr(pa[1]) if lo else None, INNER, ptr(e[0]), ptr(e[1]) if lo else None, INNER,
                nsplit, ptr(cand_t), C, ptr(out, off))
        if id0 is None:
            return lib.tcar_cand_scores(*args, ld, None)
        return lib.tcar_cand_scores_owned(*args, C, id0, None)

    want = torch.full((B, ld), SENTINEL, dtype=torch.float32, device="cuda")
    assert scores(whole, N, None, want) == 0
    S = len(shards)
    stride = B * C + 9                                                   # what lies between two parts is never read
    parts = torch.full((S * stride,), SENTINEL, dtype=torch.float32, device="cuda")
    for s, e in enumerate(shards):
        assert scores(e, EDGES[s + 1] - EDGES[s], EDGES[s], parts, s * stride) == 0
    torch.cuda.synchronize()
    w = want.cpu().numpy()
    p = parts.cpu().numpy().reshape(S, stride)
    assert (p[:, B * C:] == SENTINEL).all() and (w[:, C:] == SENTINEL).all()
    p = p[:, :B * C].reshape(S, B, C)
    inside = (cand >= 0) & (cand < N)
    owner = np.where(inside, cand // ROWS_PER_SHARD, -1)
    assert all((owner == s).any() for s in range(S)) or C == 1
    for s in range(S):
        mine = owner == s
        assert p[s][mine].tobytes() == w[:, :C][mine].tobytes(), s       # the owner: the whole-plane call's bits
        assert (p[s][~mine].view(np.int32) == NEG_INF_BITS).all(), s     # everyone else: -inf, nothing read
    # an owned id0 = 0 call over the whole planes is tcar_cand_scores
    again = torch.full((B * C,), SENTINEL, dtype=torch.float32, device="cuda")
    assert scores(whole, N, 0, again) == 0

    # the combine: the owner's word, also a NaN and a -0.0 that an owner wrote
    odd = [(b, c) for b in range(B) for c in range(C) if inside[b, c]][:2]
    marks = np.array([0x7fc01234, 0x80000000], np.uint32).view(np.int32)
    pi = parts.view(torch.int32)
    wi = w[:, :C].copy().view(np.int32)
    for (b, c), m in zip(odd, marks):
        pi[int(owner[b, c]) * stride + b * C + c] = int(m)
        wi[b, c] = m
    out = torch.full((B, ld), SENTINEL, dtype=torch.float32, device="cuda")
    assert lib.tcar_cand_combine(B, C, S, ROWS_PER_SHARD, N, ptr(cand_t), C, ptr(parts), stride, ptr(out), ld, None) == 0
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert again.cpu().numpy().tobytes() == w[:, :C].tobytes()
    assert (o[:, C:] == SENTINEL).all()                                  # columns >= C are unwritten
    assert np.ascontiguousarray(o[:, :C]).view(np.int32).tobytes() == wi.tobytes()
    assert (np.ascontiguousarray(o[:, :C]).view(np.int32)[~inside] == NEG_INF_BITS).all()
    assert (parts.cpu().numpy().reshape(S, stride)[:, B * C:] == SENTINEL).all()


def test_argument_errors_launch_nothing(lib):
    out = torch.full((B, 8), SENTINEL, dtype=torch.float32, device="cuda")
    cand = torch.zeros(B, 8, dtype=torch.int32, device="cuda")
    parts = torch.full((3, B, 8), 1.0, dtype=torch.float32, device="cuda")
    comb = lambda **kw: lib.tcar_cand_combine(*[dict(dict(B=B, C=8, S=3, rps=256, N=N, cand=ptr(cand), ldc=8, parts=ptr(parts), stride=B * 8,
                                                         out=ptr(out), ldo=8, stream=None), **kw)[a]
                                               for a in ("B", "C", "S", "rps", "N", "cand", "ldc", "parts", "stride", "out", "ldo", "stream")])
    assert comb(S=0) == -1 and comb(S=65) == -1 and comb(C=0) == -1 and comb(C=1025) == -1 and comb(stride=B * 8 - 1) == -1
    assert comb(out=None) == -1 and comb(rps=0) == -1 and comb(N=0) == -1 and comb(ldo=7) == -1 and comb(out=ptr(parts, 8)) == -1
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
