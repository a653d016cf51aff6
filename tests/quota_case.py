"""What the tests of per-category caps share (test_gpu_quota_serve.py, test_gpu_ragged_serve.py): the list length, the cap, a category
table over the N = 700 items of window_case.py, and the capped lists that follow from a session's uncapped best 64."""
import numpy as np

from select_ref import capped_walk
from window_case import N

K, M = 10, 2
CAT = (np.arange(N) % 8).astype(np.int32)
CAT.setflags(write=False)


def walk_of_the_best_64(tk64, sc64):
    """the capped lists (ids, score bits) that follow from the uncapped 64 best of every session"""
    ids_out, sc_out = [], []
    for b in range(tk64.shape[0]):
        ids = tk64[b][tk64[b] >= 0].astype(np.int64)
        assert len(ids) == 64, b                                    # 64 items, so everything else scores lower
        s = np.full(N, -np.inf, np.float32)
        s[ids] = sc64[b, :len(ids)]
        el = np.zeros(N, bool)
        el[ids] = True
        want = capped_walk(s, CAT, K, M, el)
        assert len(want) == K, (b, want)                            # the precondition: the walk is over before the 64 are
        ids_out.append(want)
        sc_out.append(s[want])
    return np.array(ids_out, np.int32), np.array(sc_out, np.float32)
