"""The ragged gather and the ragged attention pools at the op level (include/tcar_ragged.h: tcar_gather_clip_fwd_ragged,
tcar_attn_pool_fwd_ragged, tcar_attn_pool_fwd_slabs_ragged) against their rectangular twins, at the shape of
serve_case.reference(): N = 700, H = 250, Ht = 64, B = 41.

One wave owns a session in both forms and runs the same operations on the same rows in the same order, and the gather is per row:
every session of the mix must carry the BITS the rectangular launch gives the sub-batch of its length — no band."""
import ctypes as C

import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401

from ragged_util import MIX_SMALL, SET, group, offsets, random_ragged
from gpu_util import _need_gpu, ptr
from serve_case import B, reference

pytestmark = pytest.mark.gpu

N1, N2 = 7, 5           # split-K slabs of the two projections, as the step launches them at ldh = 256, ldt = 64


def test_the_mix_is_what_the_kernels_can_go_wrong_on():
    lens = MIX_SMALL
    assert len(lens) == B and set(lens.tolist()) == set(SET) and lens[0] != lens[-1]
    assert any(len(set(lens[i:i + 4].tolist())) == 4 for i in range(0, B - 3, 4))       # the four waves of a workgroup loop differently
    assert {1, 3, 4, 5, 7, 40} <= set(lens.tolist())        # T = 1; below, at, above the 4 cached positions; odd; the whole table


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def test_every_session_carries_the_bits_of_the_rectangular_kernels_of_its_length():
    _need_gpu()
    from tcar_amd import _lib
    from tcar_amd.engine import TcarEngine
    r = reference()
    eng = TcarEngine(r["params"], r["content"], r["mw"], max_grad=2.0, scoring="f32")
    lib, g, dev, st = eng.lib, eng.geo, eng.dev, eng._stream()
    feed = random_ragged(MIX_SMALL, 11)
    off, pos = offsets(MIX_SMALL)
    R = int(off[-1])
    f32 = dict(dtype=torch.float32, device=dev)
    tab, dims = eng._tables(), eng.dims

    def gather(bt, rows, rg=None):
        out = [torch.full((rows, c), float("nan"), **f32) for c in (g.ic, g.pt, g.ldt)] + [torch.full((bt.B, g.ct), float("nan"), **f32)]
        if rg is None:
            rc = lib.tcar_gather_clip_fwd(C.byref(dims), C.byref(tab), C.byref(bt), *[ptr(t) for t in out], st)
        else:
            rc = lib.tcar_gather_clip_fwd_ragged(C.byref(dims), C.byref(tab), C.byref(bt), C.byref(rg), *[ptr(t) for t in out], st)
        assert rc == 0
        return out

    bt = eng.make_resident(feed)
    assert bt.B == B and bt.T == 40 and bt._rg.R == R
    up = bt._keep[:bt._keep.numel()].cpu().numpy()             # off | pos ride behind the feed in the same buffer
    tail = up[7 * R + 3 * B:7 * R + 3 * B + B + 1 + R]
    assert tail[:B + 1].tolist() == off.tolist() and tail[B + 1:].tolist() == pos.tolist()
    x_icp, x_pt, x_act, click = gather(bt, R, bt._rg)
    torch.cuda.synchronize()
    assert not any(bool(torch.isnan(t).any()) for t in (x_icp, x_pt, x_act, click))       # every row was written

    # the pools' inputs: random projections (finished rows, and as split-K slabs), the gathered rows, a random query
    gen = torch.Generator(device="cpu").manual_seed(3)
    rnd = lambda *shape: torch.randn(*shape, generator=gen).to(dev)
    pre1, pre2, q = rnd(R, g.ldh), rnd(R, g.ldh), torch.tanh(rnd(B, g.ic))
    slabs = rnd(N1 + N2, R, g.ldh)
    w1, w2 = eng._w("m_wres"), eng._w("s_wres")

    def pool(nb, rows, xi, xp, p1, p2, qq, rg=None, T=0):
        pooled, alpha = torch.full((nb, g.ek), float("nan"), **f32), torch.full((3, rows), float("nan"), **f32)
        a = (ptr(xi), ptr(xp), ptr(p1), ptr(p2), ptr(qq), w1, w2, ptr(pooled), ptr(alpha), st)
        rc = lib.tcar_attn_pool_fwd(C.byref(dims), nb, T, *a) if rg is None else lib.tcar_attn_pool_fwd_ragged(C.byref(dims), nb, C.byref(rg), *a)
        assert rc == 0
        return pooled, alpha

    def pool_slabs(nb, rows, xi, xp, sl, qq, rg=None, T=0):
        pooled, alpha = torch.full((nb, g.ek), float("nan"), **f32), torch.full((3, rows), float("nan"), **f32)
        o1, o2 = torch.full((rows, g.ldh), float("nan"), **f32), torch.full((rows, g.ldh), float("nan"), **f32)
        sl = sl.contiguous()
        a = (ptr(xi), ptr(xp), ptr(sl), N1, ptr(sl, N1 * rows * g.ldh), N2, rows * g.ldh, ptr(o1), ptr(o2), ptr(qq), w1, w2, ptr(pooled),
             ptr(alpha), st)
        rc = lib.tcar_attn_pool_fwd_slabs(C.byref(dims), nb, T, *a) if rg is None else \
            lib.tcar_attn_pool_fwd_slabs_ragged(C.byref(dims), nb, C.byref(rg), *a)
        assert rc == 0
        return pooled, alpha, o1, o2

    po, al = pool(B, R, x_icp, x_pt, pre1, pre2, q, bt._rg)
    ps, als, o1, o2 = pool_slabs(B, R, x_icp, x_pt, slabs, q, bt._rg)
    torch.cuda.synchronize()
    assert not any(bool(torch.isnan(t).any()) for t in (po, al, ps, als, o1, o2))

    seen = np.zeros(B, bool)
    for L in sorted(set(MIX_SMALL.tolist())):
        idx, sub = group(feed, L)
        rows = torch.tensor((off[idx][:, None] + np.arange(L)[None, :]).reshape(-1).astype(np.int64), device=dev)
        sid = torch.tensor(idx.astype(np.int64), device=dev)
        nb = len(idx)
        # the gather: the rows the rectangular launch writes for the sub-batch of this length
        want = gather(eng.make_resident(sub), nb * L)
        for name, got, w in (("x_icp", x_icp[rows], want[0]), ("x_pt", x_pt[rows], want[1]), ("x_act", x_act[rows], want[2]),
                             ("click_t", click[sid], want[3])):
            assert _bits(got) == _bits(w), (L, name)
        # the pools, on the same pre1 / pre2 / x rows and q
        xi, xp, qq = x_icp[rows].contiguous(), x_pt[rows].contiguous(), q[sid].contiguous()
        wp, wa = pool(nb, nb * L, xi, xp, pre1[rows].contiguous(), pre2[rows].contiguous(), qq, T=L)
        assert _bits(po[sid]) == _bits(wp), (L, "pooled")
        assert _bits(al[:, rows]) == _bits(wa), (L, "alpha")
        wp, wa, w1o, w2o = pool_slabs(nb, nb * L, xi, xp, slabs[:, rows], qq, T=L)
        assert _bits(ps[sid]) == _bits(wp), (L, "pooled, slabs")
        assert _bits(als[:, rows]) == _bits(wa), (L, "alpha, slabs")
        assert _bits(o1[rows]) == _bits(w1o) and _bits(o2[rows]) == _bits(w2o), (L, "folded projections")
        seen[idx] = True
    assert seen.all()                                    # no session left out
    # (the slab fold and the finished rows differ: the two forms were not fed the same projections)
    assert _bits(po) != _bits(ps)

    # argument errors, before any launch: R < B, T = 41, NULL off
    def rg(R_=R, off_=bt._rg.off, pos_=bt._rg.pos):
        d = _lib.Ragged()
        d.R, d.off, d.pos = R_, off_, pos_
        return d
    outs = [ptr(t) for t in (x_icp, x_pt, x_act, click)]
    t41 = eng._without_neg(bt)
    t41.T = 41
    for bad_bt, bad in ((bt, rg(R_=B - 1)), (bt, rg(off_=None)), (t41, rg())):
        assert lib.tcar_gather_clip_fwd_ragged(C.byref(dims), C.byref(tab), C.byref(bad_bt), C.byref(bad), *outs, st) == -1
    a = (ptr(x_icp), ptr(x_pt), ptr(pre1), ptr(pre2), ptr(q), w1, w2, ptr(po), ptr(al), st)
    for bad in (rg(R_=B - 1), rg(off_=None)):
        assert lib.tcar_attn_pool_fwd_ragged(C.byref(dims), B, C.byref(bad), *a) == -1
    eng._ensure_work(B, 40, R)
    for bad_bt, bad in ((bt, rg(R_=B - 1)), (bt, rg(off_=None)), (t41, rg())):
        assert lib.tcar_ragged_forward(C.byref(eng._ctx()), C.byref(bad_bt), C.byref(bad), 0, st) == -1
    torch.cuda.synchronize()
