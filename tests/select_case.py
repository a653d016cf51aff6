"""What the op-level tests of the streamed selection share (test_gpu_select.py, test_gpu_select_merge.py; include/tcar_serve.h:
tcar_select_reset / _panel / _finish): one fp32 matrix x [B, ldn] per catalog size with its numpy reference, the run over a partition
into panels, and the check of a list against the reference's."""
import numpy as np
import torch

from gpu_util import ptr

# N -> panel sizes: the largest allowed (ceil128(N), at most 49,152) and a smaller one
PANELS = {7: (128,), 1003: (1024, 128), 20001: (20096, 4096), 49200: (49152, 8192), 70001: (49152, 8192)}
KS = (1, 20, 64)


_CASES = {}


def case(N):
    """inputs and the numpy reference of one catalog size: computed once, shared by every k and partition, never written"""
    if N in _CASES:
        return _CASES[N]
    from oracle.metrics_oracle import topk_list
    rng = np.random.RandomState(N)
    B = 6
    ldn = (N + 127) // 128 * 128
    x = (rng.standard_normal((B, ldn)) * 2).astype(np.float32)      # rows 0 and 4: random
    x[1, :N] = -0.75                                      # all-tie row: top-k is the highest indices
    x[2, : N // 2] = x[2, 0]                              # half the row tied at one value
    x[3, N - 1] = 50.0                                    # the winner sits in the last column
    P = min(PANELS[N])
    if N > P:                                             # the 20 largest values straddle the first panel boundary
        x[5, P - 10:P + 10] = 100.0 + rng.permutation(20).astype(np.float32)
    if N > 49152:                                         # and the next 20 the boundary of the largest panel
        x[5, 49152 - 10:49152 + 10] = 60.0 + rng.permutation(20).astype(np.float32)
    x[:, N:] = 1e9                                        # padding columns must never be picked
    lab = np.array([0, N - 1, N // 3, N - 1, min(5, N - 1), N // 2], np.int32)
    xv = x[:, :N].astype(np.float64)
    ref = {"x": x, "lab": lab, "B": B, "ldn": ldn,
           "top": [topk_list(x[b, :N], 64) for b in range(B)],
           "rank": ((xv > xv[np.arange(B), lab][:, None]).sum(1) + 1).astype(np.int32),
           "ce": np.log(np.exp(xv - xv.max(1, keepdims=True)).sum(1)) + xv.max(1) - xv[np.arange(B), lab]}
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CASES[N] = ref
    return ref


def run(lib, ref, N, k, P, excl=None):
    """reset, one tcar_select_panel per panel of P columns (the last one partial), finish -> numpy outputs"""
    B, ldn = ref["B"], ref["ldn"]
    d = torch.tensor(ref["x"]).cuda()
    dl = torch.tensor(ref["lab"]).cuda()
    ls = d[torch.arange(B), dl.long()].contiguous()       # gathered from x: exact
    state = torch.empty(int(lib.tcar_select_state_bytes(B, k)) // 4, dtype=torch.int32, device="cuda")
    topk = torch.full((B, k), -7, dtype=torch.int32, device="cuda")
    score = torch.full((B, k), -7.0, device="cuda")
    rank = torch.empty(B, dtype=torch.int32, device="cuda")
    ce = torch.empty(B, device="cuda")
    de, X = (torch.tensor(excl).cuda(), excl.shape[1]) if excl is not None else (None, 0)
    rc = lib.tcar_select_reset(B, k, ptr(state), None)
    assert rc == 0, ("tcar_select_reset", rc, B, k)
    for n0 in range(0, N, P):
        rc = lib.tcar_select_panel(B, n0, min(P, N - n0), ptr(d, n0), ldn, k, ptr(dl), ptr(ls), ptr(de) if X else None, X,
                                   ptr(state), None)
        assert rc == 0, ("tcar_select_panel", rc, n0, min(P, N - n0), k)
    rc = lib.tcar_select_finish(B, k, ptr(state), ptr(ls), ptr(topk), ptr(score), ptr(rank), ptr(ce), None)
    assert rc == 0, ("tcar_select_finish", rc, B, k)
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == ref["x"]).all(), ("the scores were written", N, k, P)            # the scores are left untouched
    return topk.cpu().numpy(), score.cpu().numpy(), rank.cpu().numpy(), ce.cpu().numpy()


def check_lists(ref, N, k, tk, sc, want_lists):
    x = ref["x"]
    for b in range(ref["B"]):
        want = want_lists[b][:k]
        assert tk[b].tolist() == want + [-1] * (k - len(want)), (b, tk[b].tolist(), want)
        n = len(want)
        assert (sc[b, :n].view(np.int32) == x[b, want].view(np.int32)).all(), b           # bit for bit
        assert (sc[b, n:] == -7.0).all(), b                                               # untouched where the list ends
