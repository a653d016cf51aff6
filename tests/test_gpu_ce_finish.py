"""The cross-entropy finish after the logits GEMM's softmax epilogue, at op level (csrc/ce.hip over csrc/ce_rows.h): the rescale launch
on its own against the one-launch finish, bit for bit, and the label rule of a catalog shard's window against the clamp."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_util import _kb32_index, _planes, close, lib, ptr, ptr2  # noqa: F401  (lib: the module's fixture)

pytestmark = pytest.mark.gpu

# (77, 129, 96): M in neither a 16-row nor a 128-row unit, N one past a 128 block, the last group nearly empty; (300, 1000, 64): three
# 128-row blocks, the last one ragged; (40, 50001, 64): N > 512 * 96 — more than 512 groups at either group width, the smallest N at
# which the fold walks its pairs in a loop instead of holding them in registers (40 * ngroups * 8 bytes: the one-launch form still)
SHAPES = [(77, 129, 96), (300, 1000, 64), (40, 50001, 64)]
_CACHE = {}


def _bits(t):
    return t.view(torch.int16)


def _epilogue(lib, M, N, K):
    """tcar_gemm_bf16_ce on the seeded inputs of test_logits_gemm_softmax_epilogue, then tcar_ce_finish on one copy of the plane (A)
    and tcar_ce_rescale with A's row statistics on another (B).  Computed once per shape; nothing in it is written afterwards."""
    if (M, N, K) in _CACHE:
        return _CACHE[(M, N, K)]
    rng = np.random.RandomState(M + N)
    A = (rng.standard_normal((M, K)) * 0.7).astype(np.float32)
    Bm = (rng.standard_normal((N, K)) * 0.6).astype(np.float32)
    label = rng.randint(0, N, M).astype(np.int32)
    label[0], label[-1] = 0, N - 1
    x = A.astype(np.float64) @ Bm.astype(np.float64).T
    ah, al, ai, ar = _planes(lib, A)
    bh, bl, bi, br = _planes(lib, Bm)
    Np, Mp = (N + 127) // 128 * 128, (M + 127) // 128 * 128
    e = torch.full((Mp * Np,), float("nan"), dtype=torch.bfloat16, device="cuda")
    nstat = M * ((N + 63) // 64 + 8) * 2
    stats = torch.full((nstat,), float("nan"), device="cuda")
    lab_d = torch.tensor(label).cuda()
    lab_logit = torch.zeros(M, device="cuda")
    gw, ng = C.c_int32(0), C.c_int32(0)
    assert lib.tcar_gemm_bf16_ce(M, N, K, ptr2(ah), ptr2(al), ai, ar, ptr2(bh), ptr2(bl), bi, br, K, None, None, None, 0, ptr2(e), Np, Mp,
                                 ptr(stats), nstat, ptr2(lab_d), ptr(lab_logit), 3, C.byref(gw), C.byref(ng), None) == 0
    c = dict(M=M, N=N, Np=Np, Mp=Mp, x=x, label=label, e=e, stats=stats, lab_logit=lab_logit, gw=gw.value, ng=ng.value,
             idx=torch.tensor(_kb32_index(Mp, Np), device="cuda"))
    m = x.max(1, keepdims=True)
    c["lse"] = m[:, 0] + np.log(np.exp(x - m).sum(1))
    c["rowstat"], c["ce"], c["A"] = torch.zeros(2 * M, device="cuda"), torch.zeros(M, device="cuda"), e.clone()
    assert lib.tcar_ce_finish(M, N, c["gw"], c["ng"], ptr(stats), ptr(lab_logit), ptr2(lab_d), ptr(c["rowstat"]), ptr(c["ce"]),
                              ptr2(c["A"]), Np, None) == 0
    c["B"] = _rescale(lib, c, label, 0, 0)
    _CACHE[(M, N, K)] = c
    return c


def _rescale(lib, c, label, lab_off, lab_window):
    plane = c["e"].clone()
    lab_d = torch.tensor(np.asarray(label, dtype=np.int32)).cuda()
    assert lib.tcar_ce_rescale(c["M"], c["N"], c["gw"], c["ng"], ptr(c["stats"]), ptr(c["rowstat"]), ptr2(lab_d), lab_off, lab_window,
                               ptr2(plane), c["Np"], None) == 0
    return plane


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_rescale_alone_equals_the_finish_bitwise(lib, M, N, K):
    """With the default TCAR_CE_FOLD the finish is ce_fold_rescale_kernel and the rescale ce_rescale_kernel: the two front ends of
    ce_rescale_piece leave the same bits in the WHOLE buffer, padding rows and columns included.  At ngroups > 512 — which the parity
    test never reaches — the loss and the plane are held to the fp64 reference with that test's bounds."""
    c = _epilogue(lib, M, N, K)
    assert torch.equal(_bits(c["A"]), _bits(c["B"]))
    if (M, N, K) != SHAPES[2]:
        return
    assert c["ng"] > 512, c["ng"]
    x, label, lse = c["x"], c["label"], c["lse"]
    close(c["ce"].cpu().numpy(), lse - x[np.arange(M), label], name="ce", rtol=1e-4, atol_scale=1e-5)
    d = c["A"][c["idx"]].float().cpu().numpy()
    want = np.exp(x - lse[:, None])
    want[np.arange(M), label] -= 1.0
    # bf16 plane of a value rounded twice (exp to bf16, product to bf16): 2^-7 relative, 2^-9 absolute at the label (p - 1)
    err = np.abs(d[:M, :N] - want)
    assert (err <= 2.0 ** -7 * np.abs(want) + 1e-30 + 2.0 ** -8 * (np.arange(N)[None, :] == label[:, None])).all(), float(err.max())
    assert (d[:M, N:] == 0).all() and (d[M:] == 0).all()                      # padding columns and the k-rows of dE
    rel = np.linalg.norm(d[:M, :N] - want) / np.linalg.norm(want)
    assert rel < 4e-3, rel


def test_rescale_label_window_against_the_clamp(lib):
    """A catalog shard that starts at item n0: labels inside [n0, n0 + N) are columns of the plane; one below the window and one at
    its end match NOTHING under lab_window = 1 — the entry at the row's own label column stays bf16(e * scale) — and CLAMP to column
    0 / N - 1 under lab_window = 0, where the -1 then lands: the one difference between the two label rules."""
    M, N, K = SHAPES[1]
    n0 = 5000
    c = _epilogue(lib, M, N, K)
    L, x, lse, idx = c["label"], c["x"], c["lse"], c["idx"]
    rows = np.arange(M)
    odd = rows % 2 == 1
    outside = np.where((rows // 2) % 2 == 0, n0 - 1, n0 + N)
    lab = np.where(odd, outside, L + n0).astype(np.int32)
    Mp, Np = c["Mp"], c["Np"]

    def at(col):            # mask over the whole [Mp, Np] buffer: (odd row, its col[row])
        return np.pad(odd, (0, Mp - M))[:, None] & (np.arange(Np)[None, :] == np.pad(col, (0, Mp - M))[:, None])

    p = np.exp(x - lse[:, None])
    B = _bits(c["B"][idx]).cpu().numpy()                              # [Mp, Np]: padding rows and columns included
    Wt = _rescale(lib, c, lab, n0, 1)
    W = _bits(Wt[idx]).cpu().numpy()
    own = at(L)                                                       # an odd row's own label column: the one entry that differs
    assert (W[~own] == B[~own]).all()
    assert (np.abs(Wt[idx].float().cpu().numpy()[own] - p[own[:M, :N]]) <= 2.0 ** -7 * p[own[:M, :N]] + 1e-30).all()      # nothing subtracted
    Ct = _rescale(lib, c, lab, n0, 0)
    hit = at(np.where(outside < n0, 0, N - 1))                        # where the clamp puts the -1 of an odd row
    assert (_bits(Ct[idx]).cpu().numpy()[~hit] == W[~hit]).all()
    want = p[hit[:M, :N]] - 1.0
    assert (np.abs(Ct[idx].float().cpu().numpy()[hit] - want) <= 2.0 ** -7 * np.abs(want) + 2.0 ** -8).all()
