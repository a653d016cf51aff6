"""The two streamed selectors decide ELIGIBILITY with the same code (csrc/panel_fold.h: padding columns, exclusion lists, the window
lo <= key < hi, the unaligned key slice), so on the same matrix, the same `excl` and the same window the first k entries of the
shortlist (tcar_retrieve_*) ARE the unlabelled select list (tcar_select_*): ids and scores, byte for byte.

Inputs: those of retrieve_select_case.reference() — B = 5, N = 5,000, ld = 5,120, X = 24 — with the NaN entries of row 3 made
finite (the select fold reserves NaN for dead candidates; its +inf, -inf, -0.0 and +0.0 entries stay).  Row 4 with the filters keeps
its pool of 180 items, so every list of k <= 64 is full.  The host half compares the two numpy models and runs without a GPU; the GPU
half compares the two kernels with each other and with the model, over "panels of 128" and "1001 + 3999, copied" (a key slice that is
not 16-byte aligned, and a partial last group)."""
import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401

import retrieve_select_case as rs
import select_ref
from gpu_util import lib, ptr  # noqa: F401  (lib: the fixture)
from retrieve_ref import eligible_mask, shortlist

B, N, LD, X = rs.B, rs.N, rs.LD, rs.X
KS = (1, 20, 64)
CS = (64, 1024)
PARTITIONS = ("panels of 128", "1001 + 3999, copied")

_REF = {}


def reference():
    """the inputs and, per (filtered, k), the select model's list (ids [B, k] int32, scores [B, k] fp32): computed once, never written"""
    if _REF:
        return _REF
    r = rs.reference()
    x = np.array(r["x"])
    nan = np.isnan(x[3])
    assert nan.sum() == 40
    x[3, nan] = -0.5 - 0.25 * np.arange(40, dtype=np.float32)
    lists = {}
    for filtered in (False, True):
        f = dict(excl=r["excl"], key=r["key"], lo=r["lo"], hi=r["hi"]) if filtered else {}
        pools = [eligible_mask(N, b, None, f.get("key"), f.get("lo"), f.get("hi")) for b in range(B)]
        if filtered:
            assert int((eligible_mask(N, 4, **f)).sum()) == 180
        for k in KS:
            ids, sc = np.empty((B, k), np.int32), np.empty((B, k), np.float32)
            for b in range(B):
                with np.errstate(invalid="ignore", over="ignore"):          # (row 3's +inf in the model's softmax pair: not compared)
                    st = select_ref.fold_state(np.arange(N), x[b, :N], k, pool=pools[b], excl=r["excl"][b] if filtered else ())
                assert len(st["ids"]) == k, (filtered, k, b)                  # every list is full
                ids[b], sc[b] = select_ref.finish(st, k)[0], st["scores"]
            lists[filtered, k] = (ids, sc)
    _REF.update(x=x, key=r["key"], lo=r["lo"], hi=r["hi"], excl=r["excl"], lists=lists)
    for v in [x] + [a for p in lists.values() for a in p]:
        v.setflags(write=False)
    return _REF


@pytest.mark.parametrize("k", KS)
def test_the_models_agree_the_shortlist_starts_with_the_select_list(k):
    r = reference()
    for filtered in (False, True):
        f = dict(excl=r["excl"], key=r["key"], lo=r["lo"], hi=r["hi"]) if filtered else {}
        want_ids, want_sc = r["lists"][filtered, k]
        for C_ in CS:
            ids, sc = shortlist(r["x"][:, :N], C_, **f)
            assert (ids[:, :k] == want_ids).all(), (k, C_, filtered)
            assert sc[:, :k].tobytes() == want_sc.tobytes(), (k, C_, filtered)


@pytest.fixture(scope="module")
def dev(lib):
    r = reference()
    return {n: torch.tensor(np.array(r[n])).cuda() for n in ("x", "key", "lo", "hi", "excl")}


def run_select(lib, dev, k, panels, copied, filtered):
    """tcar_select_reset, one unlabelled tcar_select_panel_quota per panel, tcar_select_finish -> (topk, score) as numpy arrays"""
    x = dev["x"]
    state = torch.full((int(lib.tcar_select_state_bytes(B, k)) // 4,), 0x7f7f7f7f, dtype=torch.int32, device="cuda")
    topk = torch.full((B, k), -7, dtype=torch.int32, device="cuda")
    score = torch.full((B, k), -7.0, device="cuda")
    assert lib.tcar_select_reset(B, k, ptr(state), None) == 0
    for n0, n in panels:
        if copied:
            ld = (n + 3) // 4 * 4
            buf = torch.full((B, ld), 1e9, device="cuda")
            buf[:, :n] = x[:, n0:n0 + n]
            pp = ptr(buf)
        else:
            ld, pp = LD, ptr(x, n0)
        if filtered:
            rc = lib.tcar_select_panel_quota(B, n0, n, pp, ld, k, None, None, ptr(dev["excl"]), X, ptr(state), None, ptr(dev["key"]),
                                             ptr(dev["lo"]), ptr(dev["hi"]), None, 0)
        else:
            rc = lib.tcar_select_panel_quota(B, n0, n, pp, ld, k, None, None, None, 0, ptr(state), None, None, None, None, None, 0)
        assert rc == 0, (n0, n, rc)
    assert lib.tcar_select_finish(B, k, ptr(state), None, ptr(topk), ptr(score), None, None, None) == 0
    torch.cuda.synchronize()
    return topk.cpu().numpy(), score.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_the_kernels_agree_with_each_other_and_with_the_model_bit_for_bit(lib, dev, k):
    r = reference()
    for filtered in (False, True):
        want_ids, want_sc = r["lists"][filtered, k]
        for name in PARTITIONS:
            panels, copied = rs.PARTITIONS[name]
            what = (k, name, "excl + window" if filtered else "plain")
            topk, score = run_select(lib, dev, k, panels, copied, filtered)
            assert (topk == want_ids).all(), what
            assert score.tobytes() == want_sc.tobytes(), what
            for C_ in CS:
                ids, sc, _ = rs.run(lib, dev, C_, panels, copied, filtered)
                assert (ids[:, :k] == topk).all(), what + (C_,)
                assert np.ascontiguousarray(sc[:, :k]).tobytes() == score.tobytes(), what + (C_,)
