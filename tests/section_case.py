"""What the tests of sectioned selection share (include/tcar_sections.h): the numpy model of a section list — select_ref.fold_state
with the pool "the section's category, inside the window, not NaN" — and the comparison of a device result with it."""
import numpy as np

from select_ref import fold_state

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def section_lists(scores, cat, sections, k, window=None, key=None, excl=()):
    """the G lists of ONE session over the items 0 .. N - 1: [(ids, scores fp32)] in section order.  window = (lo, hi) over `key`."""
    scores, cat = np.asarray(scores, dtype=np.float32), np.asarray(cat)
    ids = np.arange(scores.shape[0])
    ok = ~np.isnan(scores)
    if window is not None:
        ok &= (window[0] <= np.asarray(key, dtype=np.int64)) & (np.asarray(key, dtype=np.int64) < window[1])
    out = []
    for code in sections:
        pool = ok & (cat == code)
        with np.errstate(invalid="ignore", over="ignore"):                 # (the model's softmax pair is not compared)
            st = fold_state(ids[pool], scores[pool], k, excl=excl)          # NaN rows never reach the model's sort
        out.append((st["ids"], st["scores"]))
    return out


def check_sections(x_row, want, tk, sc, k, tag, untouched=-7.0):
    """device lists tk [G, k] / sc [G, k] of one session against the model's `want`: ids, -1 behind the end, the scores' own bits
    where an id is, and `untouched` behind the end"""
    for g, (ids, _) in enumerate(want):
        n = len(ids)
        assert tk[g].tolist() == list(ids) + [-1] * (k - n), (tag, g, tk[g].tolist(), ids)
        assert sc[g, :n].view(np.int32).tolist() == np.asarray(x_row, np.float32)[ids].view(np.int32).tolist(), (tag, g)
        if untouched is not None:
            assert (sc[g, n:] == untouched).all(), (tag, g)
