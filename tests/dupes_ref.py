"""The model of the duplicate audit (include/tcar_dupes.h) that the host and the GPU tests share: a direct loop over the definition.

audit_from_sims takes ANY [N, N] fp32 matrix of similarities — the numpy model's (similar_ref.sims_f32), or the block one
tcar_sim_panel call wrote — so the audit's logic (threshold, members, both sides of a pair, the list order of the partner) is checked
apart from the arithmetic of the cosine.  audit_f64 is the same loop over the fp64 cosines of the definition."""
import numpy as np

from similar_ref import sims_f64


def audit_from_sims(S, t, member=None):
    """S [N, N] similarities, t the threshold, member [N] bool (None: every item) -> (count int32 [N], partner int32 [N], sim [N] of
    S's dtype): count[i] = #{j in M, j != i, S[i, j] >= t} (0 for i outside M), partner[i] = the first such j by (S[i, j], j)
    descending (-1: none), sim[i] = S[i, partner[i]] (+0: none).  NaN is never >= t."""
    S = np.asarray(S)
    N = S.shape[0]
    assert S.shape == (N, N)
    member = np.ones(N, bool) if member is None else np.asarray(member, bool)
    count, partner, sim = np.zeros(N, np.int32), np.full(N, -1, np.int32), np.zeros(N, S.dtype)
    t = S.dtype.type(t)
    for i in np.flatnonzero(member):
        with np.errstate(invalid="ignore"):
            ok = member & (S[i] >= t)
        ok[i] = False
        js = np.flatnonzero(ok)
        count[i] = len(js)
        if len(js):
            best = js[S[i, js] == S[i, js].max()].max()          # the largest similarity; among equals the larger id
            partner[i], sim[i] = best, S[i, best]
    return count, partner, sim


def audit_f64(content, t, member=None):
    """the audit of the rows of content [N, H] over the fp64 cosines of the definition"""
    return audit_from_sims(sims_f64(content, content), t, member)
