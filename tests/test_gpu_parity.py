"""GPU parity tests (run with -m gpu on an MI355X): every HIP kernel, through the C-ABI, against the fp64 CPU
oracle on the same seeded inputs, the committed golden fixture, and size-independent properties at the full
Globo-like size.  Tolerance: 1e-3 relative (BASELINE.json north_star) — the fp32 path is typically ~1e-5."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import tcar_amd  # noqa: F401
from tcar_amd import _lib
from gpu_util import RTOL, _kb32_index, _need_gpu, _planes, close, lib, ptr, ptr2  # noqa: F401  (lib: the module-scoped fixture)
from helpers import GOLD
from step_cases import CASES, _case, check_grads, rel_norm

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("M,N,K", [(1, 1, 4), (5, 7, 8), (130, 129, 36), (128, 128, 32), (512, 300, 832),
                                   (257, 64, 1000), (64, 832, 2052)])


def test_gemm_layouts(lib, layout, M, N, K):
    rng = np.random.RandomState(M * 7 + N * 3 + K + layout)
    ld = lambda x: (x + 3) // 4 * 4 + 4
    a_shape = (M, ld(K)) if layout != 2 else (K, ld(M))
    b_shape = (K, ld(N)) if layout != 1 else (N, ld(K))
    A = rng.standard_normal(a_shape).astype(np.float32)
    Bm = rng.standard_normal(b_shape).astype(np.float32)
    Al = A[:, :K] if layout != 2 else A[:, :M].T
    Bl = Bm[:, :N] if layout != 1 else Bm[:, :K].T
    want = Al.astype(np.float64) @ Bl.astype(np.float64)
    dA, dB = torch.tensor(A).cuda(), torch.tensor(Bm).cuda()
    ldc = ld(N)
    dC = torch.full((M, ldc), 7.0, device="cuda")
    rc = lib.tcar_gemm_f32(layout, M, N, K, ptr(dA), A.shape[1], ptr(dB), Bm.shape[1], ptr(dC), ldc, None, 0, 0, 1, None)
    assert rc == 0
    torch.cuda.synchronize()
    got = dC.cpu().numpy()
    close(got[:, :N], want, name="gemm")
    assert (got[:, N:] == 7.0).all()                      # nothing outside [M, N] is written


def test_gemm_epilogues_and_splitk(lib):
    rng = np.random.RandomState(5)
    M, N, K = 200, 192, 4096
    A = rng.standard_normal((M, K)).astype(np.float32) * 0.05
    Bm = rng.standard_normal((K, N)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    C0 = rng.standard_normal((M, N)).astype(np.float32)
    dA, dB, db = torch.tensor(A).cuda(), torch.tensor(Bm).cuda(), torch.tensor(bias).cuda()
    z = A.astype(np.float64) @ Bm.astype(np.float64) + bias
    for act, f in ((1, lambda x: np.maximum(x, 0)), (2, np.tanh)):
        dC = torch.tensor(C0).cuda()
        assert lib.tcar_gemm_f32(0, M, N, K, ptr(dA), K, ptr(dB), N, ptr(dC), N, ptr(db), act, 0, 1, None) == 0
        close(dC.cpu().numpy(), f(z), name="act%d" % act)
    dC = torch.tensor(C0).cuda()
    assert lib.tcar_gemm_f32(0, M, N, K, ptr(dA), K, ptr(dB), N, ptr(dC), N, None, 0, 1, 1, None) == 0
    close(dC.cpu().numpy(), z - bias + C0, name="beta")
    S = lib.tcar_gemm_splitk_effective(K, 7)
    slabs = torch.empty(S, M, N, device="cuda")
    out = torch.empty(M, N, device="cuda")
    assert lib.tcar_gemm_f32(0, M, N, K, ptr(dA), K, ptr(dB), N, ptr(slabs), N, None, 0, 0, 7, None) == 0
    assert lib.tcar_splitk_reduce(ptr(slabs), S, M, N, N, ptr(out), None) == 0
    close(out.cpu().numpy(), z - bias, name="splitk")


@pytest.mark.parametrize("entry", ["tcar_gemm_f32_grouped", "tcar_gemm_x3_grouped"])
def test_gemm_grouped_segments_and_atomic_splitk(lib, entry):
    """Grouped launch: a 3-segment K-concatenated problem + a biased/activated one (NN), and atomic split-K
    weight-gradient problems (TN) into a zeroed C — for the fp32-MFMA kernel and its split-bf16 twin."""
    grouped = getattr(lib, entry)
    from tcar_amd._lib import GemmDesc
    from tcar_amd.engine import TcarEngine
    rng = np.random.RandomState(9)
    D = TcarEngine.desc
    M = 300
    xs = [rng.standard_normal((M, k)).astype(np.float32) for k in (512, 256, 64)]
    ws = [rng.standard_normal((k, 192)).astype(np.float32) * 0.1 for k in (512, 256, 64)]
    x2, w2 = rng.standard_normal((70, 128)).astype(np.float32), rng.standard_normal((128, 64)).astype(np.float32) * 0.1
    b2 = rng.standard_normal(64).astype(np.float32)
    dx = [torch.tensor(a).cuda() for a in xs]
    dw = [torch.tensor(a).cuda() for a in ws]
    dx2, dw2, db2 = torch.tensor(x2).cuda(), torch.tensor(w2).cuda(), torch.tensor(b2).cuda()
    c1 = torch.empty(M, 192, device="cuda")
    c2 = torch.empty(70, 64, device="cuda")
    descs = [D(M, 192, [(ptr(dx[i]), xs[i].shape[1], ptr(dw[i]), 192, xs[i].shape[1]) for i in range(3)], ptr(c1), 192),
             D(70, 64, [(ptr(dx2), 128, ptr(dw2), 64, 128)], ptr(c2), 64, bias=ptr(db2), act=2)]
    arr = (GemmDesc * 2)(*descs)
    assert grouped(0, 2, arr, None) == 0
    close(c1.cpu().numpy(), sum(x.astype(np.float64) @ w.astype(np.float64) for x, w in zip(xs, ws)), name="3seg")
    close(c2.cpu().numpy(), np.tanh(x2.astype(np.float64) @ w2 + b2), name="bias-tanh")
    # TN, atomic split-K: dW = x^T dy with K = 5000 rows
    Kr = 5000
    x = rng.standard_normal((Kr, 320)).astype(np.float32)
    dy = rng.standard_normal((Kr, 256)).astype(np.float32)
    xd, dyd = torch.tensor(x).cuda(), torch.tensor(dy).cuda()
    g1 = torch.zeros(320, 256, device="cuda")
    g2 = torch.zeros(64, 256, device="cuda")
    descs = [D(320, 256, [(ptr(xd), 320, ptr(dyd), 256, Kr)], ptr(g1), 256, splitk=5, atomic=1),
             D(64, 256, [(ptr(xd, 128), 320, ptr(dyd), 256, Kr)], ptr(g2), 256, splitk=2, atomic=1)]
    arr = (GemmDesc * 2)(*descs)
    assert grouped(2, 2, arr, None) == 0
    close(g1.cpu().numpy(), x.astype(np.float64).T @ dy, name="atomic dW", atol_scale=5e-5)
    close(g2.cpu().numpy(), x[:, 128:192].astype(np.float64).T @ dy, name="atomic dW view", atol_scale=5e-5)
    # NT (dx = dy W^T) with odd sizes
    dyn = rng.standard_normal((77, 256)).astype(np.float32)
    wn = rng.standard_normal((130, 256)).astype(np.float32)
    dd, wd = torch.tensor(dyn).cuda(), torch.tensor(wn).cuda()
    o = torch.full((77, 132), 3.0, device="cuda")
    arr = (GemmDesc * 1)(D(77, 130, [(ptr(dd), 256, ptr(wd), 256, 256)], ptr(o), 132))
    assert grouped(1, 1, arr, None) == 0
    got = o.cpu().numpy()
    close(got[:, :130], dyn.astype(np.float64) @ wn.astype(np.float64).T, name="NT")
    assert (got[:, 130:] == 3.0).all()


# -------------------------------------------------------------------------------------- standalone score ops
def test_softmax_ce_and_rank_topk(lib):
    rng = np.random.RandomState(2)
    B, N = 9, 1003
    ldn = 1024
    x = (rng.standard_normal((B, ldn)) * 3).astype(np.float32)
    x[3, :N] = 1.5                                   # all-tie row
    x[4, 10:40] = x[4, 5]                            # partial ties
    lab = rng.randint(0, N, B).astype(np.int32)
    lab[4] = 5
    d = torch.tensor(x).cuda()
    dl = torch.tensor(lab).cuda()
    rank = torch.empty(B, dtype=torch.int32, device="cuda")
    topk = torch.empty(B, 20, dtype=torch.int32, device="cuda")
    assert lib.tcar_rank_topk(B, N, ptr(d), ldn, ptr(dl), 20, ptr(rank), ptr(topk), None) == 0
    xv = x[:, :N].astype(np.float64)
    want_rank = (xv > xv[np.arange(B), lab][:, None]).sum(1) + 1
    assert (rank.cpu().numpy() == want_rank).all()
    from oracle.metrics_oracle import topk_list
    for b in range(B):
        assert topk[b].cpu().numpy().tolist() == topk_list(x[b, :N], 20), b
    ce = torch.empty(B, device="cuda")
    assert lib.tcar_softmax_ce(B, N, ptr(d), ldn, ptr(dl), ptr(ce), None) == 0
    lse = np.log(np.exp(xv - xv.max(1, keepdims=True)).sum(1)) + xv.max(1)
    close(ce.cpu().numpy(), lse - xv[np.arange(B), lab], name="ce")
    p = np.exp(xv - lse[:, None])
    p[np.arange(B), lab] -= 1
    got = d.cpu().numpy()
    close(got[:, :N], p, name="dlogits")
    assert (got[:, N:] == 0).all()
    assert np.abs(got[:, :N].sum(1)).max() < 1e-4    # rows of softmax - onehot sum to 0


# --------------------------------------------------------------------------------------------- full model
@pytest.mark.parametrize("scoring", ["f32", "bf16x3", "bf16x3-mixed"])
@pytest.mark.parametrize("N,H,Ht,B,T,K", CASES)
def test_step_matches_oracle(N, H, Ht, B, T, K, scoring):
    """All scoring precisions hold the SAME 1e-3 gate on logits and loss: bf16x3 carries fp32 operands as hi/lo bf16 planes;
    bf16x3-mixed relaxes the gradients only (check_grads)."""
    _need_gpu()
    from oracle.tcar_oracle import TcarOracle
    from tcar_amd.engine import TcarEngine
    params, content, mw, batch = _case(N, H, Ht, B, T, K, seed=N + H + B + T)
    eng = TcarEngine(params, content, mw, max_grad=2.0, scoring=scoring)
    ora = TcarOracle(params, content, mw, max_grad=2.0)
    # forward + eval
    rank, topk, ce, logits = eng.eval_step(batch, keep_logits=True)
    o_logits, o_ce = ora.eval_batch(batch)
    close(logits.cpu().numpy(), o_logits.numpy(), name="logits")
    close(ce.cpu().numpy(), o_ce.numpy(), name="ce")
    lab = torch.as_tensor(batch["label"], dtype=torch.long)
    lg = logits.cpu().double()
    assert (rank.cpu().numpy() == ((lg > lg.gather(1, lab[:, None])).sum(1).numpy() + 1)).all()
    # gradients + clip norms
    loss = eng.loss_and_grads(batch)
    o, g_o, sq_o = ora.loss_and_grads(batch)
    close(loss.cpu().numpy(), o["loss"].detach().numpy(), name="loss")
    g_e, sq_e = eng.export_grads(), eng.export_sqnorms()
    check_grads(g_e, sq_e, {k: v.numpy() for k, v in g_o.items()}, sq_o, scoring)
    # three optimizer steps
    for i in range(3):
        le = eng.train_step(batch)
        lo = ora.train_step(batch)
        # the first loss is the forward pass at the initial variables (1e-3 in every precision); later ones follow Adam steps
        # on gradients that carry bf16 noise in mixed mode (a coordinate may move by lr the other way): 1e-2 there
        close(le.cpu().numpy(), lo.numpy(), name="train loss %d" % i, rtol=1e-2 if (scoring == "bf16x3-mixed" and i) else RTOL)
    # after Adam steps a coordinate whose gradient is at rounding level moves by ~lr with a rounding-determined sign
    # (Adam normalises by sqrt(v)); the split-bf16 mode has ~1e-5 relative gradient noise instead of ~1e-7
    p_e, p_o = eng.export_params(), ora.export()
    for k in p_o:
        if scoring == "f32":
            close(p_e[k], p_o[k], name="param " + k, atol_scale=1e-4)
        else:   # gradients were compared at 1e-3 above; here allow a quarter of the distance Adam can travel (lr * steps);
            # mixed: a coordinate whose gradient is below the bf16 noise can move the full distance the other way
            d = np.abs(p_e[k] - p_o[k]).max()
            travel = 2.0 if scoring == "bf16x3-mixed" else 0.25
            assert d <= 1e-3 * np.abs(p_o[k]).max() + travel * 1e-3 * 3, ("param " + k, d)
            if scoring == "bf16x3-mixed":
                # ... but a coordinate whose gradient carried SIGNAL at the first step (>= 10 % of the variable's largest) has
                # moved the way the oracle's did: the two-plane bound (a quarter of lr * steps) holds there
                g1 = np.abs(g_o[k].numpy())
                big = g1 >= 0.1 * g1.max() if g1.max() > 0 else np.zeros_like(g1, dtype=bool)
                if big.any():
                    db = np.abs(p_e[k] - p_o[k])[big].max()
                    assert db <= 1e-3 * np.abs(p_o[k]).max() + 0.25 * 1e-3 * 3, ("param (signal coordinates) " + k, db)


def test_golden_fixture():
    _need_gpu()
    from tcar_amd.engine import TcarEngine
    z = np.load(os.path.join(GOLD, "oracle_step_small.npz"))
    params = {k[2:]: z[k] for k in z.files if k.startswith("p/")}
    batch = {k[2:]: z[k] for k in z.files if k.startswith("b/")}
    eng = TcarEngine(params, z["content"], z["mwdhm"], max_grad=1.5)
    rank, topk, ce, logits = eng.eval_step(batch, keep_logits=True)
    close(logits.cpu().numpy(), z["logits"], name="logits")
    assert (rank.cpu().numpy() == z["rank"]).all()
    loss = eng.loss_and_grads(batch)
    close(loss.cpu().numpy(), z["loss"], name="loss")
    ge, sq = eng.export_grads(), eng.export_sqnorms()
    for k in ge:
        close(ge[k], z["g/" + k], name="grad " + k, atol_scale=5e-5)
        assert abs(sq[k] - float(z["sqn/" + k])) <= 2e-3 * float(z["sqn/" + k]) + 1e-12
    eng.update()
    p1 = eng.export_params()
    for k in p1:
        close(p1[k], z["p1/" + k], name="p1 " + k, atol_scale=1e-4)
    eng.train_step(batch)
    eng.train_step(batch)
    p3 = eng.export_params()
    for k in p3:
        close(p3[k], z["p3/" + k], name="p3 " + k, atol_scale=1e-4)


@pytest.mark.parametrize("scoring", ["f32", "bf16x3"])
def test_full_size_properties(scoring):
    """Globo-like size (N=46,033, H=250, B=512): properties that need no oracle run."""
    _need_gpu()
    from tcar_amd.engine import TcarEngine
    N, H, Ht, B, T, K = 46033, 250, 64, 512, 3, 20
    params, content, mw, batch = _case(N, H, Ht, B, T, K, seed=99, emb_std=0.05, w_std=0.05)
    eng = TcarEngine(params, content, mw, scoring=scoring)
    rank, topk, ce, logits = eng.eval_step(batch, keep_logits=True)
    lg = logits.double()
    lab = torch.as_tensor(batch["label"], dtype=torch.long, device="cuda")
    # (1) rank / top-k consistency with the materialised scores
    assert (rank.long() == (lg > lg.gather(1, lab[:, None])).sum(1) + 1).all()
    tv = lg.gather(1, topk.long())
    assert (tv[:, :-1] >= tv[:, 1:]).all()                               # sorted descending
    assert (tv[:, -1:] >= lg.topk(21, dim=1).values[:, 20:21]).all()     # nothing larger was missed
    # (2) CE equals logsumexp - label score
    want = torch.logsumexp(lg, 1) - lg.gather(1, lab[:, None]).squeeze(1)
    close(ce.cpu().numpy(), want.cpu().numpy(), name="ce full")
    # (3) data-parallel additivity: gradients of two half batches add up to the full-batch gradient
    eng.loss_and_grads(batch)
    g_full = eng.export_grads()
    acc = None
    for sl in (slice(0, B // 2), slice(B // 2, B)):
        sub = {k: v[sl] for k, v in batch.items()}
        eng.loss_and_grads(sub)
        g = eng.export_grads()
        acc = g if acc is None else {k: acc[k] + g[k] for k in g}
    for k in g_full:
        close(acc[k], g_full[k], name="dp-sum " + k, atol_scale=1e-4)
    # (4) a training step lowers the loss on the same batch
    l0 = float(eng.train_step(batch).sum())
    for _ in range(5):
        l1 = float(eng.train_step(batch).sum())
    assert l1 < l0
    # (5) padding columns of the parameter arena stay exactly zero
    E = eng.E
    assert float(E[:, H:eng.geo.ldh].abs().max()) == 0.0 and float(E[N:].abs().max()) == 0.0


@pytest.mark.parametrize("scoring", ["bf16x3", "bf16x3-mixed"])
@pytest.mark.parametrize("T", [2, 5])
def test_globo_full_size_step_matches_oracle(scoring, T):
    """The BENCHED configuration (BASELINE.json configs[1]: N = 46,033, H = 250, Ht = 64, B = 512, K = 20) against the fp64
    oracle (model_combine.py:52-163) in the benched precision and in bf16x3: full-catalog logits and per-session loss at 1e-3
    (north star), all 23 gradients and their S5 clip norms (bf16x3: 1e-3 element-wise; mixed: 1e-2 norm-wise on EVERY
    variable), then two training steps through the fused deferred-update driver that bench.py times."""
    _need_gpu()
    from oracle.tcar_oracle import TcarOracle
    from tcar_amd.engine import TcarEngine
    N, H, Ht, B, K = 46033, 250, 64, 512, 20
    params, content, mw, batch = _case(N, H, Ht, B, T, K, seed=1000 + T, emb_std=0.05, w_std=0.05)
    eng = TcarEngine(params, content, mw, scoring=scoring)
    ora = TcarOracle(params, content, mw)
    rank, topk, ce, logits = eng.eval_step(batch, keep_logits=True)
    o_logits, o_ce = ora.eval_batch(batch)
    close(logits.cpu().numpy(), o_logits.numpy(), name="logits")
    close(ce.cpu().numpy(), o_ce.numpy(), name="ce")
    # HR@20 / MRR@20 of the batch from the device ranks against the oracle's scores (ties within rounding may move a rank)
    lab = torch.as_tensor(batch["label"], dtype=torch.long)
    want_rank = ((o_logits > o_logits.gather(1, lab[:, None])).sum(1) + 1).numpy()
    r = rank.cpu().numpy()
    for i in np.nonzero(r != want_rank)[0]:      # a rank may move only across scores within fp32 rounding of the label's
        row = o_logits[i].numpy()
        near = int((np.abs(row - row[batch["label"][i]]) <= 2e-5 * np.abs(row).max()).sum())
        assert abs(int(r[i]) - int(want_rank[i])) <= near, (i, int(r[i]), int(want_rank[i]), near)
    assert abs(float((r <= 20).mean()) - float((want_rank <= 20).mean())) <= 0.002
    assert abs(float((1.0 / r * (r <= 20)).mean()) - float((1.0 / want_rank * (want_rank <= 20)).mean())) <= 1e-3
    loss = eng.loss_and_grads(batch)
    o, g_o, sq_o = ora.loss_and_grads(batch)
    close(loss.cpu().numpy(), o["loss"].detach().numpy(), name="loss")
    check_grads(eng.export_grads(), eng.export_sqnorms(), {k: v.numpy() for k, v in g_o.items()}, sq_o, scoring)
    # the fused step of the training loops (deferred update, three streams): per-session losses of two consecutive steps
    for i in range(2):
        le = eng.train_step(batch, defer_update=True)
        lo = ora.train_step(batch)
        close(le.cpu().numpy(), lo.numpy(), name="train loss %d" % i, rtol=1e-2 if (scoring == "bf16x3-mixed" and i) else RTOL)
    p_e, p_o = eng.export_params(), ora.export()
    for k in p_o:      # two Adam steps move a coordinate by at most ~2 lr; well-conditioned ones agree far closer
        d = np.abs(p_e[k] - p_o[k]).max()
        mixed = scoring == "bf16x3-mixed"
        assert d <= 1e-3 * np.abs(p_o[k]).max() + (2.0 if mixed else 0.5) * 1e-3 * 2, ("param " + k, d)
        assert rel_norm(p_e[k], p_o[k]) <= (3e-2 if mixed else 2e-3), ("param " + k, rel_norm(p_e[k], p_o[k]))


@pytest.mark.parametrize("fused_ce", [2, 1])
def test_fused_step_gradients_at_the_benched_size_match_oracle(fused_ce):
    """The gradients the FUSED training step itself leaves (the driver bench.py times: softmax epilogue, one-hot gradient GEMMs,
    order-fixed sums; `loss_and_grads` above takes the op-level path with materialised logits) against the fp64 oracle at the
    benched size — all 23 variables + clip norms at the mixed-precision gate, and tighter where the form promises it: in the anchored
    softmax form (2, default) the one-hot part of the softmax gradient is exact in dX and the plane is rounded once, so the
    session-side time path (dP = dlogits OH is exact in its operands) agrees to 3e-4 norm-wise; the rescaled form (1) likewise."""
    _need_gpu()
    from oracle.tcar_oracle import TcarOracle
    from tcar_amd.engine import TcarEngine
    N, H, Ht, B, K, T = 46033, 250, 64, 512, 20, 2
    params, content, mw, batch = _case(N, H, Ht, B, T, K, seed=1000 + T, emb_std=0.05, w_std=0.05)
    ora = TcarOracle(params, content, mw)
    o, g_o, sq_o = ora.loss_and_grads(batch)
    g_o = {k: v.numpy() for k, v in g_o.items()}
    eng = TcarEngine(params, content, mw, scoring="bf16x3-mixed")
    eng.set_tuning(TCAR_FUSED_CE=fused_ce)
    bt = eng.make_resident(batch)
    form = eng.step_form(bt)
    assert form["onehot_bwd"] and form["ce_anchored"] == (fused_ce == 2), form
    loss = eng.train_step(None, bt=bt, defer_update=True)
    torch.cuda.synchronize()
    close(loss[:B].cpu().numpy(), o["loss"].detach().numpy(), name="loss")
    g_e, sq_e = eng.export_grads(), eng.export_sqnorms()
    check_grads(g_e, sq_e, g_o, sq_o, "bf16x3-mixed")
    for k in ("cont_attention/input_linear_trans/w_3d", "cont_attention/cont_linear_trans/w_3d", "cont_attention/res_linear_trans/w_3d",
              "attout_pt_trans/w1"):
        assert rel_norm(g_e[k], g_o[k]) <= 3e-4, (k, rel_norm(g_e[k], g_o[k]))


def test_dp_engine_single_rank_path_matches_oracle():
    """The data-parallel code path (gather backward emitting rows -> exchange schedule -> scatter kernel) with a
    world of one must reproduce the oracle exactly like the fused single-GPU path."""
    _need_gpu()
    from oracle.tcar_oracle import TcarOracle
    from tcar_amd.dp import DPEngine
    N, H, Ht, B, T, K = 1000, 250, 64, 33, 5, 7
    params, content, mw, batch = _case(N, H, Ht, B, T, K, seed=321)
    eng = DPEngine(params, content, mw, max_grad=2.0)
    ora = TcarOracle(params, content, mw, max_grad=2.0)
    loss = eng.loss_and_grads(batch, cap_rows=(B + 3) * T)          # padded row capacity, as an uneven shard has
    o, g_o, sq_o = ora.loss_and_grads(batch)
    close(loss.cpu().numpy(), o["loss"].detach().numpy(), name="loss")
    g_e, sq_e = eng.export_grads(), eng.export_sqnorms()
    for k in g_o:
        close(g_e[k], g_o[k].numpy(), name="grad " + k, atol_scale=5e-5)
        assert abs(sq_e[k] - sq_o[k]) <= 2e-3 * sq_o[k] + 1e-12, ("sqnorm", k, sq_e[k], sq_o[k])
    for _ in range(2):
        close(eng.train_step(batch).cpu().numpy(), ora.train_step(batch).numpy(), name="train loss")
    p_e, p_o = eng.export_params(), ora.export()
    for k in p_o:
        close(p_e[k], p_o[k], name="param " + k, atol_scale=1e-4)


# ----------------------------------------------------------------------------------------- split-bf16 GEMM
@pytest.mark.parametrize("M,N,K,nsplit,K2", [(300, 1000, 64, 3, 0), (77, 129, 96, 3, 0), (512, 46033, 832, 3, 0), (130, 5000, 832, 1, 0),
                                             (300, 1000, 64, 3, 139), (77, 129, 512, 3, 160), (512, 46033, 512, 3, 139)])


def test_logits_gemm_softmax_epilogue(lib, M, N, K, nsplit, K2):
    """tcar_gemm_bf16_ce + tcar_ce_finish (model_combine.py:138,145 without materialised logits): per-group (max, sum) statistics,
    the label's score, the cross entropy, and the in-place rescaled plane softmax - onehot against fp64 — on every workgroup
    tile of the logits layout (group width 64 and 96), ragged M and N, padding rows / columns zero.  K2 > 0 adds the second K
    segment (A2 in hi / lo planes, B2 exact in bf16 — 0 / 1 entries like the one-hot plane of the publish-time rows)."""
    rng = np.random.RandomState(M + N)
    A = (rng.standard_normal((M, K)) * 0.7).astype(np.float32)
    Bm = (rng.standard_normal((N, K)) * 0.6).astype(np.float32)
    label = rng.randint(0, N, M).astype(np.int32)
    label[0], label[-1] = 0, N - 1
    x = A.astype(np.float64) @ Bm.astype(np.float64).T
    if nsplit == 1:          # hi planes only: the reference rounds the operands the same way
        x = torch.tensor(A).bfloat16().double().numpy() @ torch.tensor(Bm).bfloat16().double().numpy().T
    ah, al, ai, ar = _planes(lib, A)
    bh, bl, bi, br = _planes(lib, Bm)
    seg2 = (K, None, None, None, 0)
    if K2:
        A2 = (rng.standard_normal((M, K2)) * 0.5).astype(np.float32)
        B2 = (rng.uniform(size=(N, K2)) < 5.0 / K2).astype(np.float32)
        x = x + A2.astype(np.float64) @ B2.astype(np.float64).T
        a2h, a2l, a2i, _ = _planes(lib, A2)
        b2h, b2l, b2i, _ = _planes(lib, B2)
        assert a2i == b2i == 160 and float(b2l.float().abs().max()) == 0.0
        seg2 = (K, ptr2(a2h), ptr2(a2l), ptr2(b2h), a2i)
    Np, Mp = (N + 127) // 128 * 128, (M + 127) // 128 * 128
    plane = torch.full((Mp * Np,), float("nan"), dtype=torch.bfloat16, device="cuda")
    nstat = M * ((N + 63) // 64 + 8) * 2
    stats = torch.full((nstat,), float("nan"), device="cuda")
    lab_d = torch.tensor(label).cuda()
    lab_logit = torch.zeros(M, device="cuda")
    rowstat, ce = torch.zeros(2 * M, device="cuda"), torch.zeros(M, device="cuda")
    gw, ng = C.c_int32(0), C.c_int32(0)
    assert lib.tcar_gemm_bf16_ce(M, N, K + (160 if K2 else 0), ptr2(ah), ptr2(al), ai, ar, ptr2(bh), ptr2(bl), bi, br, *seg2, ptr2(plane),
                                 Np, Mp, ptr(stats), nstat, ptr2(lab_d), ptr(lab_logit), nsplit, C.byref(gw), C.byref(ng), None) == 0
    gw, ng = gw.value, ng.value
    assert gw in (64, 96) and ng * gw >= N
    st = stats[:M * ng * 2].view(M, ng, 2).cpu().numpy().astype(np.float64)
    xp = np.full((M, ng * gw), -np.inf)
    xp[:, :N] = x
    xg = xp.reshape(M, ng, gw)
    gmax = xg.max(2)
    tol = 1e-5 if nsplit == 3 else 1e-6
    live = np.isfinite(gmax)
    assert np.allclose(st[..., 0][live], gmax[live], rtol=tol, atol=tol * np.abs(x).max()) and (st[..., 0][~live] == -np.inf).all()
    gsum = np.where(live, np.exp(xg - np.where(live, gmax, 0)[..., None]).sum(2), 0.0)
    assert np.allclose(st[..., 1], gsum, rtol=2e-4, atol=1e-6)
    assert np.allclose(lab_logit.cpu().numpy(), x[np.arange(M), label], rtol=tol, atol=tol * np.abs(x).max())
    idx = torch.tensor(_kb32_index(Mp, Np), device="cuda")
    e = plane[idx].float().cpu().numpy()[:M]
    want_e = np.exp(xp[:, :ng * gw] - np.repeat(np.where(live, gmax, 0), gw, axis=1))[:, :N]
    assert np.abs(e[:, :N] - want_e).max() <= 2.0 ** -8 and (e[:, N:] == 0).all()
    assert lib.tcar_ce_finish(M, N, gw, ng, ptr(stats), ptr(lab_logit), ptr2(lab_d), ptr(rowstat), ptr(ce), ptr2(plane), Np, None) == 0
    m = x.max(1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(x - m).sum(1))
    close(ce.cpu().numpy(), lse - x[np.arange(M), label], name="ce", rtol=1e-4, atol_scale=1e-5)
    d = plane[idx].float().cpu().numpy()
    want = np.exp(x - lse[:, None])
    want[np.arange(M), label] -= 1.0
    # bf16 plane of a value rounded twice (exp to bf16, product to bf16): 2^-7 relative, 2^-9 absolute at the label (p - 1)
    err = np.abs(d[:M, :N] - want)
    assert (err <= 2.0 ** -7 * np.abs(want) + 1e-30 + 2.0 ** -8 * (np.arange(N)[None, :] == label[:, None])).all(), float(err.max())
    assert (d[:M, N:] == 0).all() and (d[M:] == 0).all()                      # padding columns and the k-rows of dE
    rel = np.linalg.norm(d[:M, :N] - want) / np.linalg.norm(want)
    assert rel < 4e-3, rel


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(256, 1000, 64), (128, 129, 96), (512, 46033, 512)])
def test_logits_gemm_anchored_epilogue_and_fold(lib, M, N, K):
    """Anchored form of the softmax epilogue (round 6).  The row reference a[b] (here: the label's score +- 3) rides INSIDE the
    contraction: the second K segment holds minus its eight partial sums in columns 139 .. 146 of A2 (hi / lo) against columns of ones
    in B2 — as the step does with the time-score planes and the one-hot plane — so tcar_gemm_bf16_ce_anchor writes exp(x - a[b])
    without group maxima, statistics (0, group sum) and the label's accumulator x_l - a; tcar_ce_anchor_fold then gives
    ce = lse - x_label against fp64, scale2 = (1 / S, one-hot residual), the label's entry as bf16(e - S), and the per-row scaled
    attout plane — and plane * scale (+ residual) is softmax - onehot to the bf16 bound of ONE rounding, the one-hot part to fp32."""
    rng = np.random.RandomState(M + N)
    A = (rng.standard_normal((M, K)) * 0.7).astype(np.float32)
    Bm = (rng.standard_normal((N, K)) * 0.6).astype(np.float32)
    label = rng.randint(0, N, M).astype(np.int32)
    label[0], label[-1] = 0, N - 1
    A2 = np.zeros((M, 160), np.float32)
    A2[:, :139] = rng.standard_normal((M, 139)) * 0.5
    B2 = np.zeros((N, 160), np.float32)
    B2[:, :139] = rng.uniform(size=(N, 139)) < 5.0 / 139
    x = A.astype(np.float64) @ Bm.astype(np.float64).T + A2.astype(np.float64) @ B2.astype(np.float64).T
    xl = x[np.arange(M), label]
    parts = rng.standard_normal((M, 8)).astype(np.float32)
    parts[:, 0] += (xl + rng.uniform(-3, 3, M)).astype(np.float32) - parts.sum(1)
    A2[:, 139:147] = -parts
    B2[:, 139:147] = 1.0
    ah, al, ai, ar = _planes(lib, A)
    bh, bl, bi, br = _planes(lib, Bm)
    a2h, a2l, a2i, _ = _planes(lib, A2)
    b2h, b2l, b2i, _ = _planes(lib, B2)
    assert a2i == b2i == 160 and float(b2l.float().abs().max()) == 0.0
    # the reference the GEMM subtracts: the partials as their hi + lo planes hold them
    pidx2 = torch.tensor(_kb32_index((M + 127) // 128 * 128, 160), device="cuda")
    anchor = -(a2h[pidx2].double() + a2l[pidx2].double())[:M, 139:147].sum(1).cpu().numpy()
    seg2 = (K, ptr2(a2h), ptr2(a2l), ptr2(b2h), a2i)
    Np, Mp = (N + 127) // 128 * 128, (M + 127) // 128 * 128
    assert Mp == M
    plane = torch.full((Mp * Np,), float("nan"), dtype=torch.bfloat16, device="cuda")
    nstat = M * ((N + 63) // 64 + 8) * 2
    stats = torch.full((nstat,), float("nan"), device="cuda")
    lab_d = torch.tensor(label).cuda()
    lab_logit = torch.zeros(M, device="cuda")
    gw, ng = C.c_int32(0), C.c_int32(0)
    assert lib.tcar_gemm_bf16_ce_anchor(M, N, K + 160, ptr2(ah), ptr2(al), ai, ar, ptr2(bh), ptr2(bl), bi, br, *seg2,
                                        ptr2(plane), Np, Mp, ptr(stats), nstat, ptr2(lab_d), ptr(lab_logit), 3, C.byref(gw), C.byref(ng),
                                        None) == 0
    gw, ng = gw.value, ng.value
    st = stats[:M * ng * 2].view(M, ng, 2).cpu().numpy()
    xp = np.full((M, ng * gw), -np.inf)
    xp[:, :N] = x
    want_e = np.exp(xp - anchor[:, None])
    assert np.allclose(st[..., 1], want_e.reshape(M, ng, gw).sum(2), rtol=3e-4, atol=1e-6)        # .y: the exponentials (the loss)
    assert np.allclose(lab_logit.cpu().numpy(), xl - anchor, rtol=1e-5, atol=1e-5 * np.abs(x).max())
    idx = torch.tensor(_kb32_index(Mp, Np), device="cuda")
    e = plane[idx].float().cpu().numpy()
    # (bf16: 7 explicit mantissa bits — round-to-nearest is within 2^-8 relative; + the split-bf16 logits' own error inside the
    #  exponential, 1e-4 at |x| ~ 40)
    assert (np.abs(e[:, :N] - want_e[:, :N]) <= (2.0 ** -8 + 1e-3) * want_e[:, :N] + 1e-30).all() and (e[:, N:] == 0).all()
    # .x: the sum of the plane's entries AS ROUNDED (the gradient's scale: plane / S_r sums to one)
    ep = np.zeros((M, ng * gw))
    ep[:, :N] = e[:, :N]
    assert np.allclose(st[..., 0], ep.reshape(M, ng, gw).sum(2), rtol=1e-5, atol=1e-30)
    # ---- the fold
    cols = 576
    ap = (rng.standard_normal((M, cols)) * 0.5).astype(np.float32)
    ph, pl, pi, _ = _planes(lib, ap)
    aps = torch.full_like(ph, float("nan"))
    rowstat, ce, rowscale = torch.zeros(2 * M, device="cuda"), torch.zeros(M, device="cuda"), torch.zeros(2 * M, device="cuda")
    assert lib.tcar_ce_anchor_fold(M, N, gw, ng, ptr(stats), ptr(lab_logit), ptr2(lab_d), ptr(rowstat), ptr(ce), ptr(rowscale), ptr2(plane),
                                   Np, ptr2(ph), ptr2(pl), ptr2(aps), cols, pi, None) == 0
    m = x.max(1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(x - m).sum(1))
    close(ce.cpu().numpy(), lse - xl, name="ce", rtol=1e-4, atol_scale=1e-5)
    S, St = st[..., 0].astype(np.float64).sum(1), st[..., 1].astype(np.float64).sum(1)      # rounded / true
    sc2 = rowscale.cpu().numpy().reshape(M, 2).astype(np.float64)
    rs, rd = sc2[:, 0], sc2[:, 1]
    assert np.allclose(rs, 1.0 / S, rtol=1e-5) and np.allclose(rowstat.cpu().numpy().reshape(M, 2), np.stack([0 * S, 1.0 / St], 1), rtol=1e-5)
    d = plane[idx].float().cpu().numpy()
    keep = np.ones((M, N), bool)
    keep[np.arange(M), label] = False
    assert (d[:, :N][keep] == e[:, :N][keep]).all()                              # nothing but the label's entry moved
    el, dl = e[np.arange(M), label].astype(np.float64), d[np.arange(M), label].astype(np.float64)
    # dX side: label entry * (1 / S) + residual = e_l / S - 1 to fp32 — the one-hot part carries no bf16 rounding
    assert np.abs(dl * rs + rd - (el * rs - 1.0)).max() <= 1e-6 and np.abs(rd).max() <= 1.01 * 2.0 ** -8
    # dE side: the row scale 1 / S' = 1 / (e_l - v) makes v / S' = e_l / S' - 1 exact; S' within 2^-8 of S
    s_e = el - dl
    assert np.allclose(s_e, S, rtol=1.01 * 2.0 ** -8)
    p = np.exp(x - lse[:, None])
    want = p.copy()
    want[np.arange(M), label] -= 1.0
    got = d[:, :N] * rs[:, None]
    got[np.arange(M), label] += rd
    err = np.abs(got - want)
    # the row's gradient sums to ZERO to fp32 (the scale is 1 / the sum of the plane's own entries, the one-hot exact): what keeps the
    # label's entry right when p_label -> 1 (its e_l - S is then the small sum of the OTHER entries, not e_l's rounding error)
    assert np.abs(got.sum(1)).max() <= 2e-6, float(np.abs(got.sum(1)).max())
    # ONE rounding per softmax element (+ the split-bf16 logits' own error inside the exponential, 1e-4 at |x| ~ 40; + the rounded
    # sum against the true one: up to 2^-8 where one element dominates)
    bound = (2.0 ** -7 + 1e-3) * p + 1e-6 * (np.arange(N)[None, :] == label[:, None]) + 1e-30
    w = np.unravel_index(np.argmax(err - bound), err.shape)
    assert (err <= bound).all(), (w, int(label[w[0]]), float(got[w]), float(want[w]), float(e[w]), float(d[w]), float(rs[w[0]]), float(S[w[0]]))
    assert np.linalg.norm(got - want) / np.linalg.norm(want) < 3e-3
    rs = 1.0 / s_e                                                              # the scale of the attout plane of dE
    pidx = torch.tensor(_kb32_index(Mp, pi), device="cuda")
    sc = aps[pidx].float().cpu().numpy()[:, :cols]
    want_sc = ap.astype(np.float64) * rs[:, None]
    assert (np.abs(sc - want_sc) <= 1.01 * 2.0 ** -8 * np.abs(want_sc) + 1e-30).all()
    # a logit far above its row's anchor SATURATES at 2^100 instead of overflowing: plane, sums and the fold stay finite
    A2[3, 139] += 200.0                      # row 3: anchor 200 below its label's score
    a2h, a2l, _, _ = _planes(lib, A2)
    plane2 = torch.full_like(plane, float("nan"))
    assert lib.tcar_gemm_bf16_ce_anchor(M, N, K + 160, ptr2(ah), ptr2(al), ai, ar, ptr2(bh), ptr2(bl), bi, br, K, ptr2(a2h), ptr2(a2l), ptr2(b2h),
                                        a2i, ptr2(plane2), Np, Mp, ptr(stats), nstat, ptr2(lab_d), ptr(lab_logit), 3, C.byref(C.c_int32(0)),
                                        C.byref(C.c_int32(0)), None) == 0
    e2 = plane2[idx].float()
    assert bool(torch.isfinite(e2).all()) and float(e2[3].max()) == 2.0 ** 100 and bool(torch.isfinite(stats[:M * ng * 2]).all())
    assert (e2[:3].cpu().numpy() == e[:3]).all()                                 # (the other rows: the same bits as before)
    assert lib.tcar_ce_anchor_fold(M, N, gw, ng, ptr(stats), ptr(lab_logit), ptr2(lab_d), ptr(rowstat), ptr(ce), ptr(rowscale), ptr2(plane2),
                                   Np, ptr2(ph), ptr2(pl), ptr2(aps), cols, pi, None) == 0
    assert bool(torch.isfinite(ce).all()) and bool(torch.isfinite(rowscale).all()) and bool(torch.isfinite(aps.float()[pidx][:, :cols]).all())
    # any B: the scaled attout rows [B, ceil32(B)) — k-rows of dE beyond the batch — are zeroed, rows beyond are left alone
    before = aps[pidx].float().clone()
    assert lib.tcar_ce_anchor_fold(M - 35, N, gw, ng, ptr(stats), ptr(lab_logit), ptr2(lab_d), ptr(rowstat), ptr(ce), ptr(rowscale), ptr2(plane2),
                                   Np, ptr2(ph), ptr2(pl), ptr2(aps), cols, pi, None) == 0
    after = aps[pidx].float()
    assert float(after[M - 35:M - 32, :cols].abs().max()) == 0.0 and torch.equal(after[M - 32:], before[M - 32:])


@pytest.mark.parametrize("N,H,Ht,B", [(3000, 250, 64, 77), (46033, 250, 64, 512), (500, 30, 100, 5), (700, 100, 200, 33)])
def test_time_onehot_plane_and_time_scores(lib, N, H, Ht, B):
    """tcar_time_onehot + tcar_time_scores (model_combine.py:86-92,135,138 — the candidate-side publish-time vectors' part of the
    logits): OH is the exact one-hot plane of the five table rows of every item (+ eight columns of ones, 139 .. 146, that the
    anchored softmax form contracts with minus a session's anchor; P is zero there here), P holds attout_t . clip(row) for every one of
    the 139 rows, and (P OH^T)[b, n] equals sum_k attout_tk[b] . clip(table_k[mwdhm[n, k]]) in fp64 to the split-bf16 bound."""
    from tcar_amd._lib import Dims
    ldh, ldt = (H + 63) // 64 * 64, (Ht + 63) // 64 * 64
    d = Dims(N, H, Ht, ldh, ldt)
    rng = np.random.RandomState(N + B)
    sizes = (13, 32, 8, 25, 61)
    tabs = [np.zeros((n, ldt), np.float32) for n in sizes]
    for t in tabs:
        t[:, :Ht] = rng.standard_normal((t.shape[0], Ht)) * rng.choice([0.05, 0.4], (t.shape[0], 1))    # rows both sides of norm 1
    mw = np.stack([rng.randint(0, n, N) for n in sizes], 1).astype(np.int32)
    ek = 2 * ldh + 5 * ldt
    att = np.tanh(rng.standard_normal((B, ek))).astype(np.float32)
    tabs_d = [torch.tensor(t).cuda() for t in tabs]
    arr = (C.c_void_p * 5)(*[t.data_ptr() for t in tabs_d])
    Np, Bp = (N + 127) // 128 * 128, (B + 127) // 128 * 128
    oh = torch.full((Np * 160,), float("nan"), dtype=torch.bfloat16, device="cuda")
    ph = torch.full((Bp * 160,), float("nan"), dtype=torch.bfloat16, device="cuda")
    pl = torch.full((Bp * 160,), float("nan"), dtype=torch.bfloat16, device="cuda")
    mw_d, att_d = torch.tensor(mw).cuda(), torch.tensor(att).cuda()
    assert lib.tcar_time_onehot(C.byref(d), ptr2(mw_d), ptr2(oh), 160, None) == 0
    assert lib.tcar_time_scores(C.byref(d), C.byref(arr), B, ptr(att_d), ek, ptr2(ph), ptr2(pl), 160, None) == 0
    off = np.concatenate([[0], np.cumsum(sizes)])[:5]
    want_oh = np.zeros((Np, 160), np.float32)
    want_oh[np.arange(N)[:, None], off[None, :] + mw] = 1.0
    want_oh[:N, 139:147] = 1.0           # the anchor columns of the anchored softmax form (P is zero there unless a step anchors)
    got_oh = oh[torch.tensor(_kb32_index(Np, 160), device="cuda")].float().cpu().numpy()
    assert (got_oh == want_oh).all()
    clipped = []
    for t in tabs:
        t64 = t.astype(np.float64)
        nrm = np.sqrt((t64 * t64).sum(1, keepdims=True))
        clipped.append(t64 * np.where(nrm > 1.0, 1.0 / (nrm + 1e-7), 1.0))
    want_p = np.zeros((Bp, 160))
    for k in range(5):
        want_p[:B, off[k]:off[k] + sizes[k]] = att[:, 2 * ldh + k * ldt:2 * ldh + (k + 1) * ldt].astype(np.float64) @ clipped[k].T
    idx = torch.tensor(_kb32_index(Bp, 160), device="cuda")
    got_h, got_l = ph[idx].float().cpu().numpy().astype(np.float64), pl[idx].float().cpu().numpy().astype(np.float64)
    assert (got_h[B:] == 0).all() and (got_l[B:] == 0).all() and (got_h[:, 139:] == 0).all() and (got_l[:, 139:] == 0).all()
    scale = np.abs(want_p).max()
    assert np.abs(got_h + got_l - want_p).max() <= 2.0 ** -16 * scale               # hi + lo planes: 16 mantissa bits
    assert np.abs(got_h - want_p).max() <= 2.0 ** -8 * scale
    # the contraction the logits GEMM runs over the two planes
    scores = (got_h + got_l)[:B] @ want_oh[:N].T.astype(np.float64)
    direct = sum(att[:, 2 * ldh + k * ldt:2 * ldh + (k + 1) * ldt].astype(np.float64) @ clipped[k][mw[:, k]].T for k in range(5))
    assert np.abs(scores - direct).max() <= 1e-5 * np.abs(direct).max()


@pytest.mark.parametrize("B", [5, 77, 512])
def test_attout_finish_scores_kernel(lib, B):
    """tcar_attout_finish_scores (model_combine.py:119,127,132 + the one-hot time scores): attout = tanh(sum of split-K slabs + bias)
    folded in slab order, its hi / lo planes, the packed [item | time] planes, and P / tclip bit-for-bit what tcar_time_scores_clip
    computes from the same attout; rows beyond B stay untouched (attout, planes) or zero (score planes)."""
    from tcar_amd._lib import Dims
    N, H, Ht, ldh, ldt = 1000, 250, 64, 256, 64
    d = Dims(N, H, Ht, ldh, ldt)
    ic, pt, ek = 2 * ldh, 5 * ldt, 2 * ldh + 5 * ldt
    nd_ic, nd_pt = 4, 3
    rng = np.random.RandomState(B)
    slabs = (rng.standard_normal((4, B, ek)) * 0.4).astype(np.float32)
    slabs[3, :, ic:] = np.nan                                   # the time problem has three slabs only: never read
    b_o, b_ot = (rng.standard_normal(ic) * 0.1).astype(np.float32), (rng.standard_normal(pt) * 0.1).astype(np.float32)
    sizes = (13, 32, 8, 25, 61)
    tabs = [(rng.standard_normal((n, ldt)) * rng.choice([0.05, 0.4], (n, 1))).astype(np.float32) for n in sizes]
    tabs_d = [torch.tensor(t).cuda() for t in tabs]
    arr = (C.c_void_p * 5)(*[t.data_ptr() for t in tabs_d])
    Bp = (B + 127) // 128 * 128
    t = lambda x: torch.tensor(x, device="cuda")
    sl, bo, bot = t(slabs), t(b_o), t(b_ot)
    att = torch.full((B + 2, ek), 7.0, device="cuda")
    mk = lambda n: torch.full((n,), 3.0, dtype=torch.bfloat16, device="cuda")
    ah, al, aph, apl = mk(Bp * ek), mk(Bp * ek), mk(Bp * (ldh + pt)), mk(Bp * (ldh + pt))
    ph, pl = mk(Bp * 160), mk(Bp * 160)
    tclip = torch.zeros(160 * ldt + 320, device="cuda")
    assert lib.tcar_attout_finish_scores(C.byref(d), C.byref(arr), B, ptr(sl), nd_ic, nd_pt, B * ek, ptr(bo), ptr(bot), ptr(att), ek,
                                         ptr2(ah), ptr2(al), ek, ptr2(aph), ptr2(apl), ldh + pt, ptr2(ph), ptr2(pl), 160, ptr(tclip),
                                         None) == 0
    pre = slabs[:3].astype(np.float64).sum(0)
    pre[:, :ic] += slabs[3, :, :ic]
    want = np.tanh(pre + np.concatenate([b_o, b_ot]).astype(np.float64))
    got = att.cpu().numpy()
    close(got[:B], want, rtol=1e-5, atol_scale=1e-6, name="attout")
    assert (got[B:] == 7.0).all()
    idx = torch.tensor(_kb32_index(Bp, ek), device="cuda")
    h, l = ah[idx].float().cpu().numpy(), al[idx].float().cpu().numpy()
    assert np.abs(h[:B].astype(np.float64) + l[:B] - got[:B]).max() <= 2.0 ** -16 and (h[B:] == 3.0).all()      # hi + lo of the fp32 value
    want_h = torch.tensor(got[:B]).bfloat16().float().numpy()
    assert (h[:B] == want_h).all()
    pidx = torch.tensor(_kb32_index(Bp, ldh + pt), device="cuda")
    ph_ = aph[pidx].float().cpu().numpy()
    assert (ph_[:B, :ldh] == want_h[:, :ldh]).all() and (ph_[:B, ldh:] == want_h[:, ic:]).all()
    # scores and clipped rows: the same bits as the stand-alone launch on this attout
    ph2, pl2 = mk(Bp * 160), mk(Bp * 160)
    tclip2 = torch.zeros_like(tclip)
    assert lib.tcar_time_scores_clip(C.byref(d), C.byref(arr), B, ptr(att), ek, ptr2(ph2), ptr2(pl2), 160, ptr(tclip2), None) == 0
    assert torch.equal(ph.view(torch.int16), ph2.view(torch.int16)) and torch.equal(pl.view(torch.int16), pl2.view(torch.int16))
    assert torch.equal(tclip, tclip2)
    # without planes / scores (the catalog-sharded step's begin): attout alone, the same bits
    att2 = torch.full((B + 2, ek), 7.0, device="cuda")
    assert lib.tcar_attout_finish_scores(C.byref(d), C.byref(arr), B, ptr(sl), nd_ic, nd_pt, B * ek, ptr(bo), ptr(bot), ptr(att2), ek,
                                         None, None, 0, None, None, 0, None, None, 0, None, None) == 0
    assert torch.equal(att2, att)


@pytest.mark.parametrize("B", [1, 8, 77, 512])
def test_click_query_mlp_in_one_launch(lib, B):
    """tcar_query_mlp (modules.py:138-139): q1 = relu(click_t Wq1 + b1), q = tanh(q1 Wq2 + b2) in fp32 against fp64 — ragged
    batch sizes (the workgroup owns eight sessions), other rows of the outputs untouched, unsupported hidden sizes refused."""
    from tcar_amd._lib import Dims
    rng = np.random.RandomState(B)
    d = Dims(1000, 250, 64, 256, 64)
    click = (rng.standard_normal((B, 128)) * 0.4).astype(np.float32)
    w1, b1 = (rng.standard_normal((128, 256)) * 0.15).astype(np.float32), (rng.standard_normal(256) * 0.1).astype(np.float32)
    w2, b2 = (rng.standard_normal((256, 512)) * 0.1).astype(np.float32), (rng.standard_normal(512) * 0.1).astype(np.float32)
    dv = lambda x: torch.tensor(x).cuda()
    cd, w1d, b1d, w2d, b2d = dv(click), dv(w1), dv(b1), dv(w2), dv(b2)
    q1 = torch.full((B + 3, 256), 7.0, device="cuda")
    q = torch.full((B + 3, 512), 7.0, device="cuda")
    assert lib.tcar_query_mlp(C.byref(d), B, ptr(cd), ptr(w1d), ptr(b1d), ptr(w2d), ptr(b2d), ptr(q1), ptr(q), None) == 0
    want1 = np.maximum(click.astype(np.float64) @ w1.astype(np.float64) + b1, 0.0)
    want2 = np.tanh(want1 @ w2.astype(np.float64) + b2)
    close(q1[:B].cpu().numpy(), want1, name="q1", rtol=1e-5, atol_scale=1e-6)
    close(q[:B].cpu().numpy(), want2, name="q", rtol=1e-5, atol_scale=1e-6)
    assert (q1[B:] == 7.0).all() and (q[B:] == 7.0).all()
    for bad in (Dims(1000, 250, 100, 256, 128), Dims(1000, 300, 64, 320, 64)):
        assert lib.tcar_query_mlp(C.byref(bad), B, ptr(cd), ptr(w1d), ptr(b1d), ptr(w2d), ptr(b2d), ptr(q1), ptr(q), None) != 0


def test_flag_fork_time_out_is_reported():
    """A polling kernel of a flag fork that gives up counts in tcar_ctx_t.sig_dev[32]; engine.check_forks() (export, epoch end,
    bench) must raise on it instead of letting a consumer that ran ahead of its producer go unnoticed — and stay silent
    after ordinary steps."""
    _need_gpu()
    from tcar_amd.engine import TcarEngine
    N, H, Ht, B, T, K = 2000, 250, 64, 32, 2, 4
    params, content, mw, batch = _case(N, H, Ht, B, T, K, seed=3)
    eng = TcarEngine(params, content, mw, scoring="bf16x3-mixed")
    for _ in range(3):
        eng.train_step(batch, defer_update=True)
    eng.flush()
    eng.check_forks()                                   # flag forks ran (default mask), none timed out
    epoch = int(np.frombuffer(eng._fork_host, dtype=np.uint32, count=1)[0])      # the context's own fork counter (host)
    assert eng._sig is not None and epoch > 0
    eng._sig[32] = 2                                    # what two expired polls leave behind
    with pytest.raises(RuntimeError, match="flag-fork"):
        eng.check_forks()
    with pytest.raises(RuntimeError, match="flag-fork"):
        eng.export_params()
    eng._sig[32] = 0
    eng.check_forks()
    # the host-visible mirror (pinned word, system-scope atomic of the polling kernel): tested after EVERY training step and
    # every evaluation step without a synchronisation — no metric leaves an engine whose forks timed out
    eng._sig_err_np[0] = 1
    with pytest.raises(RuntimeError, match="flag-fork"):
        eng.train_step(batch, defer_update=True)
    with pytest.raises(RuntimeError, match="flag-fork"):
        eng.eval_step(batch)
    eng._sig_err_np[0] = 0
    eng.flush()
    # and the DEVICE really writes both words: a polling kernel that gives up (it waits for an epoch nobody publishes)
    assert eng.lib.tcar_flag_poll_expire(eng._sig.data_ptr(), eng._sig_err.data_ptr(),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    assert int(eng._sig[32]) == 1 and int(eng._sig_err_np[0]) == 1
    with pytest.raises(RuntimeError, match="flag-fork"):
        eng.poll_fork_errors()
    eng._sig[32] = 0
    eng._sig_err_np[0] = 0


def test_two_engines_in_flight_at_once_match_their_solo_runs(monkeypatch):
    """Two engines stepped from two host threads AT THE SAME TIME — their kernels overlap on the device — reproduce their solo runs
    bit for bit.  Until round 5 the Globo-size engine differed in 25-36 of 40 steps there (observation 2): hipcc's
    SLP-packed `v_pk_fma_f32 ... op_sel:[0,1,0]` loses its low-half product in lanes 48-63 while another wave of the SIMD issues
    MFMAs (profiles/r05_obs1_erratum.txt), and another engine's scoring GEMMs put exactly such waves beside this engine's small fp32
    kernels.  The library is built without the SLP vectorizer now (_lib.SAFE_FLAGS); this is the product-level regression test of
    that mitigation (the binary-level one: tests/test_host_logic.py)."""
    _need_gpu()
    import threading
    from tcar_amd.engine import TcarEngine
    monkeypatch.setenv("TCAR_NO_PRIO", "1")          # each engine keeps the (priority) stream its thread hands it
    H, Ht, K, steps = 250, 64, 20, 30
    cases = [_case(46033, H, Ht, 512, 2, K, seed=61), _case(9000, H, Ht, 256, 3, K, seed=62)]

    def run(case, stream, barrier=None, out=None, slot=0):
        params, content, mw, batch = case
        with torch.cuda.stream(stream):
            eng = TcarEngine(params, content, mw, scoring="bf16x3-mixed")
            bt = eng.make_resident(batch)
            losses = []
            for _ in range(steps):
                if barrier is not None:
                    barrier.wait()                    # both threads enqueue step k together: the device work overlaps
                losses.append(eng.train_step(None, bt=bt, defer_update=True).clone())
            eng.flush()
            eng.check_forks()
            res = (torch.stack(losses).cpu().numpy(), eng.export_state())
        if out is not None:
            out[slot] = res
        return res

    solo = [run(c, torch.cuda.Stream(priority=-1)) for c in cases]
    both = [None, None]
    barrier = threading.Barrier(2)
    th = [threading.Thread(target=run, args=(cases[i], torch.cuda.Stream(priority=-1), barrier, both, i)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for i in range(2):
        assert both[i] is not None, "engine %d's thread died" % i
        assert (solo[i][0] == both[i][0]).all(), ("losses of engine %d" % i, int((solo[i][0] != both[i][0]).any(1).sum()))
        for k in solo[i][1]:
            assert np.array_equal(solo[i][1][k], both[i][1][k]), (i, k)


def test_flag_forks_fall_back_to_events_when_streams_do_not_overlap(monkeypatch):
    """The engine probes once whether its side streams run beside the main stream (tcar_flag_fork_selftest: true on a plain
    GPU box, and it leaves the flag words as it found them).  When the probe says no — counter-collecting profiler,
    serialised kernels — the context gets no flag words, the step forks with events and computes the same step."""
    _need_gpu()
    from tcar_amd.engine import TcarEngine
    N, H, Ht, B, T, K = 3000, 250, 64, 64, 3, 5
    params, content, mw, batch = _case(N, H, Ht, B, T, K, seed=11)
    a = TcarEngine(params, content, mw, scoring="bf16x3-mixed")
    la = [a.train_step(batch, defer_update=True).cpu().numpy() for _ in range(3)]
    a.flush()
    assert a._sig is not None and a._probe_flag_forks() and int(a._sig[32]) == 0
    monkeypatch.setattr(TcarEngine, "_probe_flag_forks", lambda self: False)
    with pytest.warns(UserWarning, match="flag forks off"):
        b = TcarEngine(params, content, mw, scoring="bf16x3-mixed")
        lb = [b.train_step(batch, defer_update=True).cpu().numpy() for _ in range(3)]
    b.flush()
    assert b._sig is None
    b.check_forks()
    # the same kernels in the same per-stream order, every sum order-fixed: the two schedules must agree BIT FOR BIT — a
    # consumer that read a stale line behind a flag would show up here
    for x, y in zip(la, lb):
        assert (x == y).all()
    pa, pb = a.export_params(), b.export_params()
    for k in pa:
        assert (pa[k] == pb[k]).all(), k


def test_fork_state_does_not_leak_between_engines():
    """The logits -> arena-zero fork is armed in the forward call and used in the backward call.  Its state lives in the
    CONTEXT's own host block (tcar_ctx_t.fork_host; round 3 kept it in thread-local slots of the library): a training forward
    of one engine cannot leave an arm behind that a LATER engine's backward takes for its own (round 3: same context address
    after garbage collection, the aux stream's negative-term forward then ran ahead of attout — seen once as 6 % wrong
    item-gradient rows in the fp32 mode).  Alternate short-lived engines of both kinds and check the fp32
    engine's gradients against a single-stream run of the same engine class."""
    _need_gpu()
    import gc
    from tcar_amd.engine import TcarEngine
    N, H, Ht, B, T, K = 3000, 250, 64, 128, 3, 20
    params, content, mw, batch = _case(N, H, Ht, B, T, K, seed=31)
    other = _case(N, H, Ht, B, T, K, seed=32)[3]         # a different batch in between: a stale attout would show
    os.environ["TCAR_NO_OVERLAP"] = "1"
    try:
        ref = TcarEngine(params, content, mw, scoring="f32")
        ref.loss_and_grads(batch)
        want = ref.export_grads()
    finally:
        del os.environ["TCAR_NO_OVERLAP"]
    del ref
    for rep in range(8):
        a = TcarEngine(params, content, mw, scoring="bf16x3-mixed")
        a.train_step(batch)                      # arms the cross-call fork slot
        del a
        gc.collect()
        b = TcarEngine(params, content, mw, scoring="f32")
        rb, ro = b.make_resident(batch), b.make_resident(other)
        for _ in range(3):
            b.loss_and_grads(None, bt=ro)        # (no host synchronisation between the two calls)
            b.loss_and_grads(None, bt=rb)
            got = b.export_grads()
            for k in want:
                close(got[k], want[k], name="rep %d grad %s" % (rep, k), rtol=1e-4, atol_scale=1e-5)
        del b, rb, ro
        gc.collect()


def test_flag_and_event_forks_agree_bitwise_over_a_long_run():
    """Race hunt at the benched size: 300 deferred steps over batches of different lengths, once with the flag forks (default
    mask 4095) and once with events only (this engine's own switch copy: TCAR_FLAG_FORK = 0); losses of every step and all 23
    variables + Adam moments at the end are bitwise equal — the two schedules run the same kernels in the same per-stream
    order with order-fixed sums, so a consumer that read a stale line behind a flag would show up here."""
    _need_gpu()
    from tcar_amd.engine import TcarEngine
    N, H, Ht, B, K = 46033, 250, 64, 512, 20
    params, content, mw, _ = _case(N, H, Ht, 8, 2, K, seed=21)
    batches = [_case(N, H, Ht, B, T, K, seed=100 + T)[3] for T in (1, 2, 3, 5, 2, 1)]
    runs = []
    for mask in (None, 0):
        eng = TcarEngine(params, content, mw, scoring="bf16x3-mixed")
        if mask is not None:
            eng.set_tuning(TCAR_FLAG_FORK=mask)
        res = [eng.make_resident(b) for b in batches]
        losses = [eng.train_step(None, bt=res[i % len(res)], defer_update=True).clone() for i in range(300)]
        eng.flush()
        eng.check_forks()
        epoch = int(np.frombuffer(eng._fork_host, dtype=np.uint32, count=1)[0])
        assert (epoch > 0) == (mask is None), epoch          # flags really were / were not in use
        runs.append((torch.stack([l[:B] for l in losses]).cpu().numpy(), eng.export_state()))
        del eng, res
        torch.cuda.empty_cache()
    assert (runs[0][0] == runs[1][0]).all()
    for k in runs[0][1]:
        assert np.array_equal(runs[0][1][k], runs[1][1][k]), k


def test_schedule_switches_agree_bitwise_with_the_default_schedule():
    """All TWELVE switches of tcar_tuning_t (round 6) against the default schedule, 60 deferred steps at the benched size over batches of
    different lengths — every loss, all variables, all Adam moments:
      * BITWISE for the switches that change WHERE or HOW a launch runs, not what it sums in which order: event forks instead of flag
        forks (TCAR_FLAG_FORK = 0, and the mask the multi-rank sharded engine takes), the cross-entropy finish as two launches
        (TCAR_CE_FOLD = 0: consulted only by the group-maximum form — test_ce_finish_as_one_launch_... compares it there), the gradient GEMMs' LDS staging (TCAR_BF16_KS = 1 / 3 / 4: 32-deep stages, 64-deep everywhere, the dX ring),
        the dE tile codes that keep the 192-row tile (TCAR_BF16_TILE = 1922 / 1923: double buffer / three-stage ring), the gather's
        throughput form from row 1 (TCAR_GATHER_BIG_ROWS = 1: the same clips and copies);
      * to 2e-4 of the loss scale for those that re-associate fp32 sums or take another arithmetic path: other workgroup tiles
        (TCAR_BF16_TILE = 256, 2562), the weight gradients' K chunk (TCAR_WGRAD_KS), the projections' split-K slabs on / off
        (TCAR_PROJ_SPLIT_ROWS), float atomics instead of the order-fixed sums (TCAR_SORT_SCATTER = 0, TCAR_DET_SMALL = 0), the softmax
        epilogue with group maxima + the rescale pass instead of the anchored form (TCAR_FUSED_CE = 1), materialised fp32 logits (TCAR_FUSED_CE = 0), the materialised candidate-time columns (TCAR_ONEHOT_TIME = 1 / 0);
      * TCAR_MHA_MFMA (off the training step): tests/test_gpu_torch_ops.py runs the attention core in both forms."""
    _need_gpu()
    from tcar_amd.engine import TcarEngine
    N, H, Ht, B, K = 46033, 250, 64, 512, 20
    params, content, mw, _ = _case(N, H, Ht, 8, 2, K, seed=29)
    batches = [_case(N, H, Ht, B, T, K, seed=500 + T)[3] for T in (2, 1, 5, 3)]
    bitwise = [{}, {"TCAR_FLAG_FORK": 0}, {"TCAR_FLAG_FORK": 4095 & ~((1 << 3) | (1 << 4) | (1 << 6))}, {"TCAR_CE_FOLD": 0},
               {"TCAR_BF16_KS": 1}, {"TCAR_BF16_KS": 3}, {"TCAR_BF16_KS": 4}, {"TCAR_BF16_TILE": 1922}, {"TCAR_BF16_TILE": 1923},
               {"TCAR_GATHER_BIG_ROWS": 1}]
    close_only = [{"TCAR_BF16_TILE": 256}, {"TCAR_BF16_TILE": 2562}, {"TCAR_WGRAD_KS": 512}, {"TCAR_PROJ_SPLIT_ROWS": 0},
                  {"TCAR_PROJ_SPLIT_ROWS": 1 << 20}, {"TCAR_SORT_SCATTER": 0}, {"TCAR_DET_SMALL": 0}, {"TCAR_FUSED_CE": 1}, {"TCAR_FUSED_CE": 0},
                  {"TCAR_ONEHOT_TIME": 1}, {"TCAR_ONEHOT_TIME": 0}]
    covered = set()
    for sw in bitwise + close_only:
        covered |= set(sw)
    assert covered | {"TCAR_MHA_MFMA"} == {"TCAR_" + f.upper() for f in _lib.TUNING_FIELDS}, covered
    base = None
    for sw in bitwise + close_only:
        eng = TcarEngine(params, content, mw, scoring="bf16x3-mixed")
        if sw:
            eng.set_tuning(**sw)
        res = [eng.make_resident(b) for b in batches]
        losses = [eng.train_step(None, bt=res[i % len(res)], defer_update=True).clone() for i in range(60)]
        eng.flush()
        eng.check_forks()
        run = (torch.stack([l[:B] for l in losses]).cpu().numpy(), eng.export_state())
        del eng, res
        torch.cuda.empty_cache()
        if base is None:
            base = run
            continue
        if sw in bitwise:
            assert (base[0] == run[0]).all(), sw
            for k in base[1]:
                assert np.array_equal(base[1][k], run[1][k]), (sw, k)
        else:
            assert np.isfinite(run[0]).all(), sw
            # (TCAR_FUSED_CE = 1 / 0 round the softmax gradient's bf16 plane twice / from fp32 logits where the anchored default rounds
            #  once: bf16-level differences in the gradients, amplified by Adam — test_anchored_softmax_form_in_the_step)
            tol = 5e-3 if "TCAR_FUSED_CE" in sw else 2e-4
            assert np.abs(base[0] - run[0]).max() <= tol * np.abs(base[0]).max(), (sw, np.abs(base[0] - run[0]).max())


def test_anchored_softmax_form_in_the_step():
    """Round 6: the fused step at the benched size takes the ANCHORED softmax form (no rescale pass over the [B, N] plane).
      * the form is on for every batch (full ones and a 500-session tail batch) and off under TCAR_FUSED_CE = 1;
      * the anchor the forward pass leaves is the label's score without its time part (|difference| small, S_b >= e^-|difference|);
      * DEFERRED steps (label rows of E updated in the early part of the split update, beside which the forward reads them) and
        IMMEDIATE steps give the same bits — losses, variables, Adam moments: the rest pass never writes a row the forward reads;
      * the anchored form and the rescaled form agree to 2e-4 of the loss scale over 30 steps and in every variable to the Adam bound;
      * a tail batch (B = 500: padding rows in every plane) between full batches."""
    _need_gpu()
    from tcar_amd.engine import TcarEngine
    N, H, Ht, B, K = 46033, 250, 64, 512, 20
    params, content, mw, _ = _case(N, H, Ht, 8, 2, K, seed=37)
    batches = [_case(N, H, Ht, B, T, K, seed=700 + T)[3] for T in (2, 1, 5)]
    tail = _case(N, H, Ht, 500, 3, K, seed=777)[3]

    def run(sw, defer, with_tail=False, steps=30):
        eng = TcarEngine(params, content, mw, scoring="bf16x3-mixed")
        if sw:
            eng.set_tuning(**sw)
        res = [eng.make_resident(b) for b in batches]
        rt = eng.make_resident(tail)
        form = (eng.step_form(res[0])["ce_anchored"], eng.step_form(rt)["ce_anchored"])
        losses = []
        for i in range(steps):
            bt = rt if (with_tail and i % 7 == 3) else res[i % len(res)]
            losses.append(eng.train_step(None, bt=bt, defer_update=defer)[:500].clone())
        eng.flush()
        eng.check_forks()
        extra = None
        if not defer and not with_tail:
            pidx = torch.tensor(_kb32_index(512, 160), device="cuda")
            anc = -(eng._p16h[pidx].double() + eng._p16l[pidx].double())[:B, 139:147].sum(1).cpu().numpy()
            lab = eng._ce_ws[2 * B:3 * B].cpu().numpy() + anc          # (the GEMM leaves the label's accumulator: x_label - anchor)
            extra = (anc, lab, eng._ce_rowscale[:2 * B].view(B, 2)[:, 0].cpu().numpy())
        out = (torch.stack(losses).cpu().numpy(), eng.export_state(), form, extra)
        del eng, res, rt
        torch.cuda.empty_cache()
        return out

    imm = run({}, False)
    assert imm[2] == (True, True), imm[2]
    anc, lab, rs = imm[3]
    assert np.abs(anc - lab).max() < 6.0, float(np.abs(anc - lab).max())       # the time part of the label's score
    assert (rs > 0).all() and (rs <= np.exp(np.abs(anc - lab)) * 1.001).all()     # S_b >= exp(x_label - anchor)
    dfr = run({}, True)
    assert (imm[0] == dfr[0]).all()
    for k in imm[1]:
        assert np.array_equal(imm[1][k], dfr[1][k]), k
    old = run({"TCAR_FUSED_CE": 1}, True)
    assert old[2] == (False, False)
    # (the forward pass of step 0 is the same arithmetic up to the reference of the exponentials; from then on the two forms'
    #  gradients differ by bf16 roundings — one per plane element against two —, which Adam amplifies like any rounding noise)
    assert np.abs(old[0][0] - dfr[0][0]).max() <= 2e-6 * np.abs(dfr[0]).max(), np.abs(old[0][0] - dfr[0][0]).max()
    assert np.abs(old[0] - dfr[0]).max() <= 5e-3 * np.abs(dfr[0]).max(), np.abs(old[0] - dfr[0]).max()
    for k in dfr[1]:        # variables: inside the Adam bound (a weight moves at most ~lr per step; the two forms differ by roundings)
        if k.startswith("var/"):
            assert np.abs(dfr[1][k] - old[1][k]).max() <= 2 * 30 * 1e-3, k
    mix_a, mix_b = run({}, True, with_tail=True), run({"TCAR_FUSED_CE": 1}, True, with_tail=True)
    assert np.isfinite(mix_a[0]).all()
    assert np.abs(mix_a[0] - mix_b[0]).max() <= 5e-3 * np.abs(mix_b[0]).max()


def test_ce_finish_as_one_launch_agrees_bitwise_with_the_two_launches():
    """Round 5: tcar_ce_finish as ONE launch whose workgroups fold their own rows' (max, sum) pairs (TCAR_CE_FOLD = w > 0, default
    1024) against the combine launch + rescale launch (0), at three grid sizes — the same lane-strided sums and shuffle trees, so the
    plane, the losses, every variable and every Adam moment after 40 deferred steps agree BIT FOR BIT.  (The group-maximum form,
    TCAR_FUSED_CE = 1: the anchored form of round 6 has no pass over the plane to fold into.)"""
    _need_gpu()
    from tcar_amd.engine import TcarEngine
    N, H, Ht, B, K = 46033, 250, 64, 512, 20
    params, content, mw, _ = _case(N, H, Ht, 8, 2, K, seed=31)
    batches = [_case(N, H, Ht, B, T, K, seed=600 + T)[3] for T in (2, 1, 5, 3)]

    def run(sw):
        eng = TcarEngine(params, content, mw, scoring="bf16x3-mixed")
        eng.set_tuning(TCAR_FUSED_CE=1, **sw)
        res = [eng.make_resident(b) for b in batches]
        losses = [eng.train_step(None, bt=res[i % len(res)], defer_update=True).clone() for i in range(40)]
        eng.flush()
        eng.check_forks()
        out = (torch.stack([l[:B] for l in losses]).cpu().numpy(), eng.export_state())
        del eng, res
        torch.cuda.empty_cache()
        return out

    base = run({})
    for sw in ({"TCAR_CE_FOLD": 0}, {"TCAR_CE_FOLD": 256}, {"TCAR_CE_FOLD": 4096}):
        got = run(sw)
        assert (base[0] == got[0]).all(), sw
        for k in base[1]:
            assert np.array_equal(base[1][k], got[1][k]), (sw, k)


def test_two_engines_stepped_alternately_from_two_host_threads_match_their_solo_runs(monkeypatch):
    """Re-entrancy of the boundary on the HOST (no global mutable state, per-device handles passed in).  Two
    engines of different shapes, each with its own context, fork words and streams, are stepped ALTERNATELY from two Python
    threads — A's step k, then B's step k, then A's step k + 1 ... (a baton of two semaphores; the thread that holds the baton
    drains the device before it hands it on) — so every fork_arm / launch / fork_go of one engine happens on another host thread
    than the other engine's and between two of its own steps, and each engine ends BIT FOR BIT where it ends when it runs alone.
    With the fork slots in per-thread state (round 3) a context that changes threads, or two contexts on one thread, could take
    each other's flags.
    (Two engines whose DEVICE work overlaps: test_two_engines_in_flight_at_once_match_their_solo_runs — the divergence round 4
    reported there was the packed-FMA erratum of DESIGN.md §7, fixed in round 5.)"""
    _need_gpu()
    import threading
    from tcar_amd.engine import TcarEngine
    monkeypatch.setenv("TCAR_NO_PRIO", "1")          # each engine keeps the (priority) stream its thread hands it
    H, Ht, K, steps = 250, 64, 20, 30
    cases = [_case(46033, H, Ht, 512, 2, K, seed=61), _case(9000, H, Ht, 256, 3, K, seed=62)]

    def run(case, stream, mine=None, other=None, out=None, slot=0):
        params, content, mw, batch = case
        with torch.cuda.stream(stream):
            eng = TcarEngine(params, content, mw, scoring="bf16x3-mixed")
            bt = eng.make_resident(batch)
            losses = []
            for _ in range(steps):
                if mine is not None:
                    assert mine.acquire(timeout=30) and not errs, "the other engine's thread failed"
                losses.append(eng.train_step(None, bt=bt, defer_update=True).clone())
                if other is not None:
                    torch.cuda.synchronize()          # the other engine's step starts on an idle device
                    other.release()
            eng.flush()
            eng.check_forks()
            assert int(np.frombuffer(eng._fork_host, dtype=np.uint32, count=1)[0]) > 0       # flag forks in use
            res = (torch.stack(losses).cpu().numpy(), eng.export_state())
        if out is not None:
            out[slot] = res
        return res

    both, errs = [None, None], []
    solo = [run(c, torch.cuda.Stream(priority=-1)) for c in cases]
    torch.cuda.synchronize()
    baton = [threading.Semaphore(1), threading.Semaphore(0)]

    def worker(i):
        try:
            run(cases[i], torch.cuda.Stream(priority=-1), baton[i], baton[1 - i], both, i)
        except BaseException as e:      # noqa: BLE001
            errs.append(e)
            baton[1 - i].release()

    th = [threading.Thread(target=worker, args=(i,), daemon=True) for i in range(2)]      # daemon: a failure never keeps the process alive
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=240)
    assert not errs, errs
    assert not any(t.is_alive() for t in th), "a stepping thread did not finish"
    for i in range(2):
        assert (solo[i][0] == both[i][0]).all(), "losses of engine %d differ" % i
        for k in solo[i][1]:
            assert np.array_equal(solo[i][1][k], both[i][1][k]), (i, k)


def test_split_bf16_planes_kb32_layout(lib):
    rng = np.random.RandomState(1)
    rows, cols = 137, 820
    x = (rng.standard_normal((rows, cols)) * np.exp(rng.uniform(-8, 8, (rows, cols)))).astype(np.float32)
    xd = torch.tensor(x).cuda()
    inner, rp = 832, 256
    hi = torch.full((rp * inner,), float("nan"), dtype=torch.bfloat16, device="cuda")
    lo = torch.full((rp * inner,), float("nan"), dtype=torch.bfloat16, device="cuda")
    phi = torch.full((rp * 576,), float("nan"), dtype=torch.bfloat16, device="cuda")
    plo = torch.full((rp * 576,), float("nan"), dtype=torch.bfloat16, device="cuda")
    assert lib.tcar_split_bf16(ptr(xd), cols, rows, cols, ptr2(hi), ptr2(lo), inner, ptr2(phi), ptr2(plo), 576, 256, 512,
                               None) == 0
    full = torch.zeros(rp, inner, device="cuda")
    full[:rows, :cols] = xd
    want_hi = full.bfloat16()
    want_lo = (full - want_hi.float()).bfloat16()
    idx = torch.tensor(_kb32_index(rp, inner), device="cuda")
    assert torch.equal(hi[idx], want_hi) and torch.equal(lo[idx], want_lo)          # incl. zero-filled padding
    pidx = torch.tensor(_kb32_index(rp, 576), device="cuda")
    packed = torch.cat([want_hi[:, :256], want_hi[:, 512:832]], 1)
    got = phi[pidx]
    assert torch.equal(got[:rows, :256 + 308], packed[:rows, :256 + 308])
    rec = hi[idx].double() + lo[idx].double()
    assert ((rec - full.double()).abs() <= 2.0 ** -16 * full.double().abs() + 1e-40).all()


@pytest.mark.parametrize("nsplit", [3, 1])
@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("M,N,K", [(512, 300, 832), (130, 129, 64), (64, 832, 2080), (257, 576, 512), (5, 7, 32),
                                   (600, 260, 96)])


def test_gemm_bf16_layouts(lib, layout, nsplit, M, N, K):
    """All three operand layouts (swizzled b128 fragments and ds_read_b64_tr_b16 transposed fragments, staged by
    direct-to-LDS DMA) against fp64; asymmetric random operands (a swapped row/col map cannot pass)."""
    rng = np.random.RandomState(M + 3 * N + 7 * K + layout)
    A = rng.standard_normal((M, K) if layout != 2 else (K, M)).astype(np.float32)
    Bm = (rng.standard_normal((K, N) if layout != 1 else (N, K)) * 0.5 + 0.25).astype(np.float32)
    Al = A if layout != 2 else A.T
    Bl = Bm if layout != 1 else Bm.T
    want = Al.astype(np.float64) @ Bl.astype(np.float64)
    ah, al, ai, ar = _planes(lib, A)
    bh, bl, bi, br = _planes(lib, Bm)
    ldc = N + 4
    dC = torch.full((M, ldc), 7.0, device="cuda")
    rc = lib.tcar_gemm_bf16(layout, M, N, K, ptr2(ah), ptr2(al), ai, ar, ptr2(bh), ptr2(bl), bi, br, ptr(dC), ldc,
                            None, 0, 0, nsplit, 1, None)
    assert rc == 0
    got = dC.cpu().numpy()
    close(got[:, :N], want, rtol=1e-3 if nsplit == 3 else 2e-2, atol_scale=2e-5 if nsplit == 3 else 6e-3, name="bf16 gemm")
    assert (got[:, N:] == 7.0).all()
    if nsplit == 1:     # hi planes only (64-deep LDS stages): exactly the product of the bf16-rounded operands, fp32 accumulation
        rb = lambda x: torch.tensor(x).bfloat16().double().numpy()
        close(got[:, :N], rb(Al) @ rb(Bl), rtol=1e-4, atol_scale=2e-6, name="bf16 gemm, hi planes")


def test_gemm_bf16_dual_output_and_splitk(lib):
    rng = np.random.RandomState(4)
    # TN with two destinations (dE: item block | time block)
    Kb, M, N = 96, 700, 576
    dl = (rng.standard_normal((Kb, M)) * 0.1).astype(np.float32)
    at = rng.standard_normal((Kb, N)).astype(np.float32)
    want = dl.astype(np.float64).T @ at.astype(np.float64)
    ah, al, ai, ar = _planes(lib, dl)
    bh, bl, bi, br = _planes(lib, at)
    c1 = torch.zeros(M, 256, device="cuda")
    c2 = torch.zeros(M, 320, device="cuda")
    assert lib.tcar_gemm_bf16(2, M, N, Kb, ptr2(ah), ptr2(al), ai, ar, ptr2(bh), ptr2(bl), bi, br, ptr(c1), 256, ptr(c2), 320,
                              256, 3, 1, None) == 0
    close(c1.cpu().numpy(), want[:, :256], atol_scale=2e-5, name="dual C1")
    close(c2.cpu().numpy(), want[:, 256:], atol_scale=2e-5, name="dual C2")
    # NN with split-K slabs (dX: contraction over the catalog)
    M, N, K = 100, 832, 6400
    a = (rng.standard_normal((M, K)) * 0.05).astype(np.float32)
    b = rng.standard_normal((K, N)).astype(np.float32)
    ah, al, ai, ar = _planes(lib, a)
    bh, bl, bi, br = _planes(lib, b)
    S = lib.tcar_gemm_splitk_effective(K, 9)
    slabs = torch.empty(S, M, N, device="cuda")
    out = torch.empty(M, N, device="cuda")
    assert lib.tcar_gemm_bf16(0, M, N, K, ptr2(ah), ptr2(al), ai, ar, ptr2(bh), ptr2(bl), bi, br, ptr(slabs), N, None, 0, 0,
                              3, 9, None) == 0
    assert lib.tcar_splitk_reduce(ptr(slabs), S, M, N, N, ptr(out), None) == 0
    close(out.cpu().numpy(), a.astype(np.float64) @ b.astype(np.float64), atol_scale=2e-5, name="splitk bf16")


def test_plain_bf16_scoring_is_close_and_trains():
    """scoring='bf16' (hi planes only) is the speed mode: logits within ~1e-2 of the oracle norm-wise, same top ranks
    up to near-ties, loss decreases."""
    _need_gpu()
    from oracle.tcar_oracle import TcarOracle
    from tcar_amd.engine import TcarEngine
    N, H, Ht, B, T, K = 1000, 250, 64, 64, 4, 20
    params, content, mw, batch = _case(N, H, Ht, B, T, K, seed=77)
    eng = TcarEngine(params, content, mw, scoring="bf16")
    ora = TcarOracle(params, content, mw)
    rank, topk, ce, logits = eng.eval_step(batch, keep_logits=True)
    o_logits, o_ce = ora.eval_batch(batch)
    rel = float((logits.cpu().double() - o_logits).norm() / o_logits.norm())
    assert rel < 1e-2, rel
    close(ce.cpu().numpy(), o_ce.numpy(), rtol=2e-2, atol_scale=1e-2, name="ce bf16")
    l0 = float(eng.train_step(batch).sum())
    for _ in range(5):
        l1 = float(eng.train_step(batch).sum())
    assert l1 < l0


def test_mixed_precision_backward_mode():
    """scoring='bf16x3-mixed': logits / loss hold the fp32-class gate (forward is bf16x3); the scoring gradients are
    plain bf16 (norm-wise 1e-2), the loss still decreases."""
    _need_gpu()
    from oracle.tcar_oracle import TcarOracle
    from tcar_amd.engine import TcarEngine
    N, H, Ht, B, T, K = 1000, 250, 64, 64, 4, 20
    params, content, mw, batch = _case(N, H, Ht, B, T, K, seed=78)
    eng = TcarEngine(params, content, mw, scoring="bf16x3-mixed")
    ora = TcarOracle(params, content, mw)
    rank, topk, ce, logits = eng.eval_step(batch, keep_logits=True)
    o_logits, o_ce = ora.eval_batch(batch)
    close(logits.cpu().numpy(), o_logits.numpy(), name="logits mixed")
    loss = eng.loss_and_grads(batch)
    o, g_o, sq_o = ora.loss_and_grads(batch)
    close(loss.cpu().numpy(), o["loss"].detach().numpy(), name="loss mixed")
    check_grads(eng.export_grads(), eng.export_sqnorms(), {k: v.numpy() for k, v in g_o.items()}, sq_o, "bf16x3-mixed")
    l0 = float(eng.train_step(batch).sum())
    for _ in range(5):
        l1 = float(eng.train_step(batch).sum())
    assert l1 < l0


@pytest.mark.parametrize("N", [8200, 20001, 49200])
def test_softmax_ce_kernel_variants(lib, N):
    """row-resident kernels (<= 16,384 / <= 49,152 columns) and the streaming kernel beyond: fp32 and bf16-plane outputs"""
    rng = np.random.RandomState(N)
    B, ldn = 3, (N + 127) // 128 * 128
    x = (rng.standard_normal((B, ldn)) * 4).astype(np.float32)
    lab = np.array([0, N - 1, N // 2], np.int32)
    xv = x[:, :N].astype(np.float64)
    lse = np.log(np.exp(xv - xv.max(1, keepdims=True)).sum(1)) + xv.max(1)
    p = np.exp(xv - lse[:, None])
    p[np.arange(B), lab] -= 1
    d, dl = torch.tensor(x).cuda(), torch.tensor(lab).cuda()
    ce = torch.empty(B, device="cuda")
    hi = torch.full((128 * ldn,), 7.0, dtype=torch.bfloat16, device="cuda")
    lo = torch.full((128 * ldn,), 7.0, dtype=torch.bfloat16, device="cuda")
    assert lib.tcar_softmax_ce_bf16(B, N, ptr(d), ldn, ptr(dl), ptr(ce), ptr(hi), ptr(lo), None) == 0
    close(ce.cpu().numpy(), lse - xv[np.arange(B), lab], name="ce planes")
    assert (d.cpu().numpy() == x).all()                       # logits untouched in plane mode
    idx = _kb32_index(128, ldn)
    g = (hi.float() + lo.float()).cpu().numpy()[idx]
    close(g[:B, :N], p, name="dlogits planes", rtol=2e-5)
    assert (g[B:] == 0).all() and (g[:B, N:] == 0).all()      # padding rows / columns are zero
    assert lib.tcar_softmax_ce(B, N, ptr(d), ldn, ptr(dl), ptr(ce), None) == 0
    got = d.cpu().numpy()
    close(got[:, :N], p, name="dlogits fp32")
    assert (got[:, N:] == 0).all()


def test_negative_term_split_and_fused_reduce(lib):
    """tcar_neg_fwd + tcar_neg_scatter + tcar_splitk_reduce_dact reproduce tcar_neg_term + tcar_splitk_reduce +
    tcar_dact_colsum (the unfused sequence), including a saturated session (S8) whose gradient is exactly 0."""
    from tcar_amd._lib import Dims
    rng = np.random.RandomState(5)
    N, H, Ht, B, K, S = 300, 250, 64, 37, 7, 5
    ldh, ldt = 256, 64
    ic, pt = 2 * ldh, 5 * ldt
    ek = ic + pt
    dims = Dims(n_items=N, H=H, Ht=Ht, ldh=ldh, ldt=ldt)
    E = (rng.standard_normal((N, ek)) * 0.3).astype(np.float32)
    att = np.tanh(rng.standard_normal((B, ek))).astype(np.float32)
    att[3, :ic] = np.sign(E[5, :ic]) * 0.99                  # session 3: huge positive logit -> saturation
    neg = rng.randint(0, N, (B, K)).astype(np.int32)
    neg[3] = 5
    slabs = rng.standard_normal((S, B, ek)).astype(np.float32)
    ce = rng.rand(B).astype(np.float32)
    w = 0.01
    t = lambda a: torch.tensor(a).cuda()
    dE, datt, dneg, dslab, dce = t(E), t(att), t(neg), t(slabs), t(ce)
    # unfused sequence
    ref_datt = torch.empty(B, ek, device="cuda")
    assert lib.tcar_splitk_reduce(ptr(dslab), S, B, ek, ek, ptr(ref_datt), None) == 0
    ref_fb, ref_loss = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    ref_gi = torch.zeros(N, ldh, device="cuda")
    assert lib.tcar_neg_term(C.byref(dims), B, K, ptr(dE), ptr(dneg), ptr(datt), w, ptr(ref_fb), ptr(ref_datt), ptr(ref_gi),
                             ptr(dce), ptr(ref_loss), None) == 0
    ref_b0, ref_b1 = torch.zeros(ic, device="cuda"), torch.zeros(pt, device="cuda")
    assert lib.tcar_dact_colsum(B, ic, ek, ptr(datt), ptr(ref_datt), ptr(ref_b0), 2, None) == 0
    assert lib.tcar_dact_colsum(B, pt, ek, ptr(datt, ic), ptr(ref_datt, ic), ptr(ref_b1), 2, None) == 0
    # split + fused
    fb, coef, part = torch.empty(B, device="cuda"), torch.empty(B, device="cuda"), torch.empty(B, ic, device="cuda")
    assert lib.tcar_neg_fwd(C.byref(dims), B, K, ptr(dE), ptr(dneg), ptr(datt), w, ptr(fb), ptr(coef), ptr(part), None) == 0
    gi, loss = torch.zeros(N, ldh, device="cuda"), torch.empty(B, device="cuda")
    assert lib.tcar_neg_scatter(C.byref(dims), B, K, ptr(dneg), ptr(datt), ptr(coef), ptr(gi), ptr(fb), ptr(dce), w,
                                ptr(loss), None) == 0
    out = torch.empty(B, ek, device="cuda")
    b0, b1 = torch.zeros(ic, device="cuda"), torch.zeros(pt, device="cuda")
    assert lib.tcar_splitk_reduce_dact(ptr(dslab), S, B, ek, ek, ptr(part), ic, ic, ptr(datt), ek, 2, ptr(out), ptr(b0), ic,
                                       ptr(b1), None) == 0
    close(fb.cpu().numpy(), ref_fb.cpu().numpy(), name="neg_fb")
    close(loss.cpu().numpy(), ref_loss.cpu().numpy(), name="loss")
    close(out.cpu().numpy(), ref_datt.cpu().numpy(), name="dattout", rtol=1e-5)
    close(gi.cpu().numpy(), ref_gi.cpu().numpy(), name="g_item", rtol=1e-5)
    close(b0.cpu().numpy(), ref_b0.cpu().numpy(), name="bias O", rtol=1e-4)
    close(b1.cpu().numpy(), ref_b1.cpu().numpy(), name="bias OT", rtol=1e-4)
    assert float(coef[3]) == 0.0 and abs(float(fb[3]) - 55.262) < 1e-2          # S8
    # against numpy for the fused reduce itself
    want = (slabs.astype(np.float64).sum(0))
    want[:, :ic] += part.cpu().numpy()
    want *= 1 - att.astype(np.float64) ** 2
    close(out.cpu().numpy(), want, name="dattout numpy", rtol=1e-5)


@pytest.mark.parametrize("scoring", ["f32", "bf16x3"])
def test_step_without_negatives(scoring):
    """a feed without the sampled negatives (model_combine.py:142-143 contribute nothing): loss = CE, the item gradient
    has no negative rows, and a step following a step WITH negatives does not reuse their stale forward outputs"""
    _need_gpu()
    from oracle.tcar_oracle import TcarOracle
    from tcar_amd.engine import TcarEngine
    N, H, Ht, B, T, K = 400, 250, 64, 33, 3, 6
    params, content, mw, batch = _case(N, H, Ht, B, T, K, seed=91)
    eng = TcarEngine(params, content, mw, scoring=scoring)
    ora = TcarOracle(params, content, mw)
    eng.loss_and_grads(batch)                              # with negatives first (fills the negative-term buffers)
    plain = {k: v for k, v in batch.items() if k != "neg"}
    loss = eng.loss_and_grads(plain)
    o, g_o, sq_o = ora.loss_and_grads(plain)
    close(loss.cpu().numpy(), o["loss"].detach().numpy(), name="loss")
    # label_neg fed as [B, 0]: the negative term is the constant 0.01 * ln 2 per session (model_combine.py:142-147)
    close(loss.cpu().numpy(), o["ce"].detach().numpy() + 0.01 * np.log(2.0), name="loss == ce + 0.01 ln 2")
    g_e, sq_e = eng.export_grads(), eng.export_sqnorms()
    for k in g_o:
        close(g_e[k], g_o[k].numpy(), name="grad " + k, atol_scale=5e-5)
        assert abs(sq_e[k] - sq_o[k]) <= 2e-3 * sq_o[k] + 1e-12, ("sqnorm", k, sq_e[k], sq_o[k])
    le, lo = eng.train_step(plain), ora.train_step(plain)
    close(le.cpu().numpy(), lo.numpy(), name="train loss")


def test_catalog_beyond_int32_flat_indices():
    """N = 4.3 M items at B = 512: B * Npad > 2^31, so any 32-bit flat index into the [B, N] score matrix, the bf16
    planes or E would wrap.  Size-independent properties on the highest rows / columns (no oracle run at this size)."""
    _need_gpu()
    from tcar_amd.engine import TcarEngine
    N, H, Ht, B, T, K = 4_300_000, 250, 64, 512, 2, 4
    if torch.cuda.get_device_properties(0).total_memory < 150e9:
        pytest.skip("needs ~70 GB of device memory")
    rng = np.random.RandomState(7)
    from tcar_amd.host.model import initial_variables
    np.random.seed(7)
    params = initial_variables(N, H, Ht, 0.05, 0.05, weight_seed=7)
    content = (rng.standard_normal((N + 1, H)).astype(np.float32) * 0.5)
    content[0] = 0
    mw = np.stack([rng.randint(1, 13, N), rng.randint(1, 32, N), rng.randint(1, 8, N), rng.randint(1, 25, N),
                   rng.randint(1, 61, N)], -1).astype(np.int32)
    b = {"seq": rng.randint(1, N + 1, (B, T)), "label": rng.randint(0, N, B), "pm": rng.randint(1, 13, (B, T)),
         "pd": rng.randint(1, 32, (B, T)), "pw": rng.randint(1, 8, (B, T)), "ph": rng.randint(1, 25, (B, T)),
         "pmi": rng.randint(1, 61, (B, T)), "cw": rng.randint(0, 7, B), "ch": rng.randint(0, 24, B),
         "gap": rng.randint(0, 11, (B, T)), "neg": rng.randint(0, N, (B, K))}
    b = {k: v.astype(np.int32) for k, v in b.items()}
    b["label"][-1] = N - 1                    # the very last score of the last row: flat index B * Npad - pad
    b["seq"][-1, :] = N                       # highest item row on the session side
    b["neg"][-1, :] = N - 1
    eng = TcarEngine(params, content, mw, scoring="bf16x3")
    rank, topk, ce, logits = eng.eval_step(b, keep_logits=True)
    lab = torch.as_tensor(b["label"], dtype=torch.long, device="cuda")
    for r in (0, B // 2, B - 1):                                       # row-wise, to keep the fp64 copies small
        lg = logits[r].double()
        assert int(rank[r]) == int((lg > lg[lab[r]]).sum()) + 1, r
        assert abs(float(ce[r]) - float(torch.logsumexp(lg, 0) - lg[lab[r]])) < 1e-3, r
        tv = lg[topk[r].long()]
        assert (tv[:-1] >= tv[1:]).all() and float(tv[-1]) >= float(lg.topk(21).values[20])
    # last row against a direct fp64 dot product of its operands (attout . E^T): catches a wrapped row offset
    att = eng.attout[B - 1].double()
    ek = eng.geo.ek
    hi, lo = eng.e16h.view(-1), eng.e16l.view(-1)
    assert hi.numel() > 2 ** 31                                          # the planes themselves exceed 2^31 elements
    k = np.arange(ek)
    for n in (0, N // 2, N - 1):
        r = n & 127                                                      # csrc/tcar_bf16_layout.h, one row
        off = ((n >> 7) * (ek // 32) + (k >> 5)).astype(np.int64) * 4096 + r * 32 + ((((k & 31) >> 3) ^ ((r >> 2) & 3)) << 3 | (k & 7))
        o = torch.as_tensor(off, device="cuda")
        row = hi[o].double() + lo[o].double()                            # E row n as the GEMM sees it (item|content|time)
        assert float((row[:512] - eng.E[n, :512].double()).abs().max()) < 1e-4
        want = float((row * att).sum())
        assert abs(float(logits[B - 1, n]) - want) <= 1e-3 * abs(want) + 1e-4, (n, float(logits[B - 1, n]), want)
    l0 = float(eng.train_step(b).sum())
    for _ in range(3):
        l1 = float(eng.train_step(b).sum())
    assert np.isfinite(l1) and l1 < l0
    assert float(eng.E[N:].abs().max()) == 0.0                           # padding rows untouched


@pytest.mark.parametrize("M,N,K", [(300, 40000, 96), (512, 38417, 64)])
def test_gemm_bf16_large_n_tiles(lib, M, N, K):
    """shapes whose workgroup count selects the 256 x 384 (8 waves, 4 x 3 MFMA tiles per wave) and 256 x 256 tiles of the
    logits GEMM, ragged in both M and N"""
    rng = np.random.RandomState(M + N + K)
    A = rng.standard_normal((M, K)).astype(np.float32)
    Bm = (rng.standard_normal((N, K)) * 0.5 + 0.25).astype(np.float32)
    want = A.astype(np.float64) @ Bm.astype(np.float64).T
    ah, al, ai, ar = _planes(lib, A)
    bh, bl, bi, br = _planes(lib, Bm)
    ldc = (N + 127) // 128 * 128
    dC = torch.full((M, ldc), 7.0, device="cuda")
    for env in ("384", "256"):
        tune = _lib.tuning(TCAR_BF16_TILE=int(env))          # a caller-owned copy of the switches: the library keeps none
        dC.fill_(7.0)
        assert lib.tcar_gemm_bf16_tuned(C.byref(tune), 1, M, N, K, ptr2(ah), ptr2(al), ai, ar, ptr2(bh), ptr2(bl), bi, br, ptr(dC),
                                        ldc, None, 0, 0, 3, 1, None) == 0
        got = dC.cpu().numpy()
        close(got[:, :N], want, rtol=1e-3, atol_scale=2e-5, name="bf16 gemm tile " + env)
        assert (got[:, N:] == 7.0).all()


@pytest.mark.parametrize("tile", ["193", "192", "256"])
def test_gemm_bf16_de_tiles(lib, tile):
    """the dE layout (both operands read transposed) on its three workgroup tiles: 192 x 192 (12 waves of 1 x 3 MFMA
    tiles), 256 x 192 and 256 x 256, with the dual (item | time) destination and ragged M"""
    rng = np.random.RandomState(11)
    M, N, K = 1000, 576, 96
    A = rng.standard_normal((K, M)).astype(np.float32)
    Bm = (rng.standard_normal((K, N)) * 0.5 + 0.25).astype(np.float32)
    want = A.astype(np.float64).T @ Bm.astype(np.float64)
    ah, al, ai, ar = _planes(lib, A)
    bh, bl, bi, br = _planes(lib, Bm)
    c1 = torch.full((M, 260), 7.0, device="cuda")
    c2 = torch.full((M, 324), 7.0, device="cuda")
    tune = _lib.tuning(TCAR_BF16_TILE=int(tile))
    assert lib.tcar_gemm_bf16_tuned(C.byref(tune), 2, M, N, K, ptr2(ah), ptr2(al), ai, ar, ptr2(bh), ptr2(bl), bi, br, ptr(c1), 260,
                                    ptr(c2), 324, 256, 3, 1, None) == 0
    g1, g2 = c1.cpu().numpy(), c2.cpu().numpy()
    close(g1[:, :256], want[:, :256], rtol=1e-3, atol_scale=2e-5, name="dE item block")
    close(g2[:, :320], want[:, 256:], rtol=1e-3, atol_scale=2e-5, name="dE time block")
    assert (g1[:, 256:] == 7.0).all() and (g2[:, 320:] == 7.0).all()


def test_cand_time_bwd_permuted_layout_equals_plain():
    """The candidate-time backward reads d_et either as [N, pt] through the inverted index or in list order (the layout
    the dE GEMM writes through tcar_gemm_bf16_perm): same table gradients and norm pieces, bit for bit."""
    _need_gpu()
    from tcar_amd.engine import TcarEngine
    N, H, Ht, B, T, K = 3000, 250, 64, 8, 2, 2
    params, content, mw, batch = _case(N, H, Ht, B, T, K, seed=5)
    eng = TcarEngine(params, content, mw, scoring="bf16x3")
    g = eng.geo
    rng = np.random.RandomState(3)
    d_et = rng.standard_normal((N, g.pt)).astype(np.float32)
    perm = eng.et_perm.cpu().numpy().reshape(5, N)
    listed = np.zeros((5 * N, g.ldt), np.float32)
    for k in range(5):
        listed[perm[k]] = d_et[:, k * g.ldt:(k + 1) * g.ldt]
    outs = []
    for permuted, src in ((0, d_et), (1, listed)):
        eng.Gx.zero_()
        eng.sqn_pieces.zero_() if hasattr(eng, "sqn_pieces") else None
        eng.d_et.view(-1).copy_(torch.tensor(src.reshape(-1)).cuda())
        gr = eng._grads()
        assert eng.lib.tcar_cand_time_bwd_indexed(C.byref(eng.dims), C.byref(eng._time_ptrs()), eng._p(eng.inv_n),
                                                  eng._p(eng.inv_off), eng._p(eng.d_et), permuted, eng._p(eng.ct_ws),
                                                  C.byref(gr), eng._stream()) == 0
        outs.append(eng.Gx.clone().cpu().numpy())
    assert np.abs(outs[0]).max() > 0
    assert (outs[0] == outs[1]).all()


@pytest.mark.parametrize("N", [7, 1003, 20001, 49200])
def test_eval_rows_rank_topk_ce(lib, N):
    """row-resident rank / top-20 / CE kernel (N <= 49,152) and the streaming fallback: strict-greater rank
    (util.py:13-17), top-k in the order of np.argsort(x)[::-1] incl. ties (model_combine.py:301), CE (:145)"""
    from oracle.metrics_oracle import topk_list
    rng = np.random.RandomState(N)
    B, k = 5, 20
    ldn = (N + 127) // 128 * 128
    x = (rng.standard_normal((B, ldn)) * 2).astype(np.float32)
    x[1, :N] = -0.75                                      # all-tie row: top-k is the highest indices
    x[2, : N // 2] = x[2, 0]                              # half the row tied at one value
    x[3, N - 1] = 50.0                                    # the winner sits in the last column
    x[:, N:] = 1e9                                        # padding columns must never be picked
    lab = np.array([0, N - 1, N // 3, N - 1, min(5, N - 1)], np.int32)
    d, dl = torch.tensor(x).cuda(), torch.tensor(lab).cuda()
    rank = torch.empty(B, dtype=torch.int32, device="cuda")
    topk = torch.full((B, k), -7, dtype=torch.int32, device="cuda")
    ce = torch.empty(B, device="cuda")
    fused = ldn <= 49152
    rc = lib.tcar_eval_rows(B, N, ptr(d), ldn, ptr(dl), k, ptr(rank), ptr(topk), ptr(ce) if fused else None, None)
    assert rc == 0
    xv = x[:, :N].astype(np.float64)
    assert (rank.cpu().numpy() == (xv > xv[np.arange(B), lab][:, None]).sum(1) + 1).all()
    tk = topk.cpu().numpy()
    for b in range(B):
        want = topk_list(x[b, :N], k)
        want = want + [-1] * (k - len(want))
        assert tk[b].tolist() == want, (b, tk[b].tolist(), want)
    assert (d.cpu().numpy() == x).all()                   # the scores are left untouched
    if fused:
        lse = np.log(np.exp(xv - xv.max(1, keepdims=True)).sum(1)) + xv.max(1)
        close(ce.cpu().numpy(), lse - xv[np.arange(B), lab], name="ce")
    else:
        assert lib.tcar_eval_rows(B, N, ptr(d), ldn, ptr(dl), k, ptr(rank), ptr(topk), ptr(ce), None) != 0


def test_python_sequenced_op_level_path_matches_the_cpp_driver():
    """engine.forward / backward / update call the op-level C-ABI entry points one by one from Python (fp32 scoring; the
    order INTEGRATION.md documents); the C++ step driver must produce the same losses, gradients and updated variables."""
    _need_gpu()
    from tcar_amd.engine import TcarEngine
    N, H, Ht, B, T, K = 700, 250, 64, 41, 3, 5
    params, content, mw, batch = _case(N, H, Ht, B, T, K, seed=17)
    a = TcarEngine(params, content, mw, max_grad=2.0, scoring="f32")
    b = TcarEngine(params, content, mw, max_grad=2.0, scoring="f32")
    b.native = False
    la, lb = a.loss_and_grads(batch), b.loss_and_grads(batch)
    close(la.cpu().numpy(), lb.cpu().numpy(), name="loss", rtol=1e-5)
    ga, gb = a.export_grads(), b.export_grads()
    for k in ga:
        close(ga[k], gb[k], name="grad " + k, rtol=1e-4, atol_scale=1e-5)
    for _ in range(2):
        close(a.train_step(batch).cpu().numpy(), b.train_step(batch).cpu().numpy(), name="train loss", rtol=1e-4)
    pa, pb = a.export_params(), b.export_params()
    for k in pa:
        assert np.abs(pa[k] - pb[k]).max() <= 1e-4 * np.abs(pa[k]).max() + 0.25 * 1e-3 * 2, k


@pytest.mark.parametrize("scoring", ["f32", "bf16x3"])
def test_deferred_update_matches_the_immediate_one(scoring):
    """train_step(defer_update=True): the Adam update of a step is applied at the start of the next one — arena + the item
    rows that step gathers first, the rest on the aux stream — or by flush() / any other entry point.  Same arithmetic
    per element as tcar_train_step (the kernel-level test below is bitwise); two engine runs differ only by the float
    atomics inside a step.  Repeated item ids (the bitmap) and an interleaved evaluation (auto-flush) are in the sequence."""
    _need_gpu()
    from tcar_amd.engine import TcarEngine
    N, H, Ht, B, T, K = 900, 250, 64, 48, 3, 4
    params, content, mw, b0 = _case(N, H, Ht, B, T, K, seed=21)
    _, _, _, b1 = _case(N, H, Ht, B, 2, K, seed=22)
    _, _, _, b2 = _case(N, H, Ht, 7, 5, K, seed=23)
    b1["seq"][:, :] = b1["seq"][0, 0]                     # one item repeated in every session: one row, many ids
    a = TcarEngine(params, content, mw, max_grad=2.0, scoring=scoring)
    d = TcarEngine(params, content, mw, max_grad=2.0, scoring=scoring)
    seq = [b0, b1, b2, b0, b2]
    for i, bt in enumerate(seq):
        la = a.train_step(bt)
        ld = d.train_step(bt, defer_update=True)
        close(ld.cpu().numpy(), la.cpu().numpy(), name="loss step %d" % i, rtol=2e-4)
        if i == 2:
            ra, rd = a.eval_step(b0), d.eval_step(b0)                     # flushes the pending update first
            close(rd[2].cpu().numpy(), ra[2].cpu().numpy(), name="eval ce", rtol=2e-4)
    assert d._pending_lr is not None
    pa, pd = a.export_params(), d.export_params()                         # export flushes
    assert d._pending_lr is None and int(d.adam_bitmap.abs().sum()) == 0
    for k in pa:
        assert np.abs(pa[k] - pd[k]).max() <= 1e-3 * np.abs(pa[k]).max() + 0.25 * 1e-3 * len(seq), k


def test_split_adam_kernels_equal_the_single_launch_bitwise(lib):
    """tcar_clip_adam_early (arena + listed item rows, each exactly once although ids repeat) followed by
    tcar_clip_adam_rest (every other row; clears the bitmap) == tcar_clip_adam_all, bit for bit, incl. the bf16 planes."""
    from tcar_amd._lib import Segments
    rng = np.random.RandomState(9)
    N, ldh, ek, arena_n = 777, 256, 832, 4096
    Npad = (N + 127) // 128 * 128
    t = lambda a: torch.tensor(a).cuda()
    E0 = rng.standard_normal((Npad, ek)).astype(np.float32)
    W0, G = rng.standard_normal(arena_n).astype(np.float32), rng.standard_normal(arena_n + 32).astype(np.float32) * 0.1
    Gi = (rng.standard_normal((N, ldh)) * 0.1).astype(np.float32)
    M0, V0 = rng.standard_normal(arena_n).astype(np.float32) * 0.01, rng.rand(arena_n).astype(np.float32) * 1e-3
    Mi0, Vi0 = (rng.standard_normal((N, ldh)) * 0.01).astype(np.float32), (rng.rand(N, ldh) * 1e-3).astype(np.float32)
    segs = Segments()
    segs.nseg = 2
    segs.off[0], segs.len[0], segs.slot[0] = 0, 1000, 1
    segs.off[1], segs.len[1], segs.slot[1] = 1024, 3072, 2
    sqn = t(np.array([2.0, 3.0, 50.0] + [0.0] * 29, np.float32))
    use = t(np.ones(32, np.int32))
    ids = t(np.array([5, 5, 5, 1, N, 300, 300, 64, 65], np.int32))      # 1-based, with repeats and both ends
    args = (2.0, 1e-3, 0.9, 0.999, 1e-8)
    out = []
    for split in (False, True):
        W, M, V, E, Mi, Vi = t(W0), t(M0), t(V0), t(E0), t(Mi0), t(Vi0)
        dG, dGi = t(G), t(Gi)
        eh = torch.zeros(Npad * ek, dtype=torch.bfloat16, device="cuda")
        el = torch.zeros_like(eh)
        bm = torch.zeros(((N + 31) // 32 + 15) // 16 * 16, dtype=torch.int32, device="cuda")      # whole 64-byte units (tcar_hip.h)
        pieces = C.c_void_p(dG.data_ptr() + 4 * arena_n)
        if split:
            assert lib.tcar_clip_adam_early(ptr(W), ptr(dG), ptr(M), ptr(V), C.byref(segs), ptr(E), ek, ptr(dGi), ptr(Mi), ptr(Vi),
                                            N, ldh, 0, ptr(sqn), pieces, ptr(use), *args, ptr2(eh), ptr2(el), ek, ptr(ids),
                                            ids.numel(), ptr(bm), None) == 0
            assert int((bm != 0).sum()) > 0
            assert lib.tcar_clip_adam_rest(ptr(E), ek, ptr(dGi), ptr(Mi), ptr(Vi), N, ldh, 0, ptr(sqn), pieces, ptr(use), *args,
                                           ptr2(eh), ptr2(el), ek, ptr(bm), None) == 0
            assert int(bm.abs().sum()) == 0
        else:
            assert lib.tcar_clip_adam_all(ptr(W), ptr(dG), ptr(M), ptr(V), C.byref(segs), ptr(E), ek, ptr(dGi), ptr(Mi), ptr(Vi), N,
                                          ldh, 0, ptr(sqn), pieces, ptr(use), *args, ptr2(eh), ptr2(el), ek, None) == 0
        out.append([x.cpu() for x in (W, M, V, E, Mi, Vi, eh.view(torch.int16), el.view(torch.int16))])
    assert not torch.equal(out[0][3], torch.tensor(E0))                   # something was updated
    for x, y in zip(*out):
        assert torch.equal(x, y)


@pytest.mark.parametrize("B,T,H,Ht", [(37, 3, 250, 64), (5, 1, 250, 64), (300, 40, 250, 64), (64, 7, 300, 64), (33, 2, 48, 16)])
def test_gather_forward_throughput_form_equals_latency_form(lib, B, T, H, Ht):
    """tcar_gather_clip_fwd has a latency form (in-step launches) and a throughput form (>= 16 k rows: small tables clipped
    once into LDS, 4 consecutive rows per wave, non-temporal stores).  Same arithmetic, so the outputs are bit-identical —
    incl. dwell bucket 11 (zero row), row counts that are no multiple of 4 and T = 1."""
    from tcar_amd._lib import Batch, Dims, Tables
    rng = np.random.RandomState(B * 100 + T)
    N = 5000
    ldh = (H + 63) // 64 * 64
    ldt = 64 if Ht <= 64 else 128
    ic, pt, ct, ek = 2 * ldh, 5 * ldt, 2 * ldt, 2 * ldh + 5 * ldt
    dev = "cuda"
    E = torch.tensor((rng.standard_normal((N, ek)) * 0.08).astype(np.float32), device=dev)
    small = [torch.tensor((rng.standard_normal((v, ldt)) * 0.3).astype(np.float32), device=dev) for v in (13, 32, 8, 25, 61, 11)]
    pos = torch.tensor((rng.standard_normal((40, ldh)) * 0.1).astype(np.float32), device=dev)
    ti = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.int32), device=dev)
    seq = ti(rng.randint(1, N + 1, (B, T)))
    pub = [ti(rng.randint(1, v, (B, T))) for v in (13, 32, 8, 25, 61)]
    gap_np = rng.randint(0, 12, (B, T))
    gap_np.flat[0] = 11                                  # out of range for the 11-row table (DESIGN S7)
    gap, cw, ch, label = ti(gap_np), ti(rng.randint(0, 7, B)), ti(rng.randint(0, 24, B)), ti(rng.randint(0, N, B))
    d = Dims(N, H, Ht, ldh, ldt)
    tab = Tables()
    tab.E, tab.pos, tab.dur = E.data_ptr(), pos.data_ptr(), small[5].data_ptr()
    for k in range(5):
        tab.time[k] = small[k].data_ptr()
    bt = Batch()
    bt.B, bt.T, bt.K = B, T, 0
    bt.seq, bt.cw, bt.ch, bt.gap, bt.label = seq.data_ptr(), cw.data_ptr(), ch.data_ptr(), gap.data_ptr(), label.data_ptr()
    for k in range(5):
        bt.pub[k] = pub[k].data_ptr()
    outs = []
    for big in (1 << 30, 1):
        x_icp, x_pt = torch.full((B * T, ic), 7.0, device=dev), torch.full((B * T, pt), 7.0, device=dev)
        x_act, click = torch.full((B * T, ldt), 7.0, device=dev), torch.full((B, ct), 7.0, device=dev)
        tune = _lib.tuning(TCAR_GATHER_BIG_ROWS=big)
        assert lib.tcar_gather_clip_fwd_tuned(C.byref(tune), C.byref(d), C.byref(tab), C.byref(bt), ptr(x_icp), ptr(x_pt),
                                              ptr(x_act), ptr(click), None) == 0
        torch.cuda.synchronize()
        outs.append([t.cpu().numpy() for t in (x_icp, x_pt, x_act, click)])
    for name, a, b in zip(("x_icp", "x_pt", "x_act", "click_t"), outs[0], outs[1]):
        bad = np.argwhere(a != b)
        assert bad.size == 0, (name, len(bad), bad[:8].tolist(), [(float(a[tuple(i)]), float(b[tuple(i)])) for i in bad[:4]])
    assert not (outs[1][0] == 7.0).all() and float(np.abs(outs[1][2][0]).max()) == 0.0      # the bucket-11 row is zero


@pytest.mark.parametrize("B,T,K,N,ldh", [(512, 2, 20, 3000, 256), (64, 40, 7, 50, 256), (300, 5, 0, 100000, 256), (1, 1, 3, 10, 256),
                                         (2048, 40, 2, 500, 256), (512, 32, 33, 2, 256), (128, 3, 4, 1_000_000, 512),
                                         (4096, 4, 1, 70000, 320), (1024, 40, 20, 70000, 256), (1024, 20, 0, 5000, 256)])


def test_sorted_segmented_item_scatter(lib, B, T, K, N, ldh):
    """tcar_segsum_*: the item-row gradients of the gathers (mode 0) and of the negatives (mode 1) added into the dense
    gradient by sort + segmented sum — head-heavy ids (runs of hundreds: multi-chunk runs), against np.add.at in fp64, the
    folds of the norms, and bit-for-bit repeatability.  Lists of up to 16384 sources are sorted in ONE workgroup's LDS, longer
    ones by the multi-workgroup form of the same stable radix sort (count / offsets / scatter per 4-bit pass; odd and even pass
    counts: the ping-pong must end in the sorted buffers) — (2048, 40, 2, 500): session list of 81,920, its head article has a run
    of thousands (summed by a whole workgroup); (1024, 40, 20, 70000): both lists long, five passes; (1024, 20, 0, 5000): four
    passes.  Further: a 2-item catalog with both lists at / over the LDS-sort limit (16,384 session sources exactly, 16,896 negatives:
    one 1-bit pass, runs of thousands), a 1 M-item catalog (20 key bits: five passes) with 512-column rows (two column
    chunks per wave), and a row width that is not a multiple of 256."""
    from tcar_amd._lib import Batch, Dims
    rng = np.random.RandomState(B + T + K)
    ek = 2 * ldh + 320
    d = Dims(N, ldh - 6, 64, ldh, 64)
    zipf = np.minimum(rng.zipf(1.3, size=(B, T)), N).astype(np.int32)                 # ids 1..N, head heavy ...
    far = rng.rand(B, T) < 0.4                                                         # ... and a tail that uses every key bit
    zipf[far] = rng.randint(1, N + 1, size=int(far.sum()))
    seq = torch.tensor(zipf, device="cuda")
    neg_np = (np.minimum(rng.zipf(1.5, size=(B, max(K, 1))), N) - 1).astype(np.int32)
    farn = rng.rand(B, max(K, 1)) < 0.4
    neg_np[farn] = rng.randint(0, N, size=int(farn.sum()))
    neg = torch.tensor(neg_np, device="cuda")
    rows_np = rng.standard_normal((B * T, ldh)).astype(np.float32)
    coef_np = rng.standard_normal(B).astype(np.float32)
    coef_np[::7] = 0.0
    att_np = np.tanh(rng.standard_normal((B, ek))).astype(np.float32)
    g0 = rng.standard_normal((N, ldh)).astype(np.float32)
    bt = Batch()
    bt.B, bt.T, bt.K = B, T, K
    bt.seq, bt.neg = seq.data_ptr(), (neg.data_ptr() if K else None)
    nbytes = lib.tcar_segsum_ws_bytes(C.byref(d), B * (T + K))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    coef, att = torch.tensor(coef_np, device="cuda"), torch.tensor(att_np, device="cuda")
    ce, fb = torch.rand(B, device="cuda"), torch.rand(B, device="cuda")
    want = g0.astype(np.float64)
    if K:
        for k in range(K):
            np.add.at(want, neg_np[:, k], coef_np[:, None].astype(np.float64) * att_np[:, :ldh])
    np.add.at(want, zipf.reshape(-1) - 1, rows_np.astype(np.float64))
    outs = []
    norms_np = (rows_np.astype(np.float64) ** 2).sum(1).astype(np.float32)
    for _ in range(3):
        g = torch.tensor(g0, device="cuda")
        sq = torch.zeros(4, device="cuda")
        ws.fill_(0xEE)                                                                 # nothing may depend on old contents
        assert lib.tcar_segsum_index(C.byref(d), C.byref(bt), ptr(ws), nbytes, None) == 0
        rows = torch.tensor(rows_np, device="cuda")
        assert lib.tcar_segsum_rows_buffer(C.byref(d), C.byref(bt), ptr(ws))           # the in-workspace buffers the step driver uses
        nb = lib.tcar_segsum_norms_buffer(C.byref(d), C.byref(bt), ptr(ws))
        assert ws.data_ptr() <= nb < ws.data_ptr() + nbytes
        off = nb - ws.data_ptr()
        ws[off:off + 4 * B * T].view(torch.float32).copy_(torch.tensor(norms_np, device="cuda"))   # what the gather backward leaves
        loss = torch.zeros(B, device="cuda")
        if K:
            assert lib.tcar_segsum_apply(C.byref(d), C.byref(bt), ptr(ws), nbytes, 1, None, ptr(coef), ptr(att), ek, ptr(g), None,
                                         None, ptr(ce), ptr(fb), 0.25, ptr(loss), None) == 0
        assert lib.tcar_sqnorm_det(ptr(g), N * ldh, ptr(ws), nbytes, None) == 0        # ||g||^2 BEFORE the session rows (S5)
        torch.cuda.synchronize()
        g_mid = g.cpu().numpy().astype(np.float64)
        assert lib.tcar_segsum_apply(C.byref(d), C.byref(bt), ptr(ws), nbytes, 0, ptr(rows), None, None, 0, ptr(g), ptr(sq, 1),
                                     ptr(sq, 2), None, None, 0.0, None, None) == 0
        torch.cuda.synchronize()
        if K:
            np.testing.assert_allclose(loss.cpu().numpy(), (ce + 0.25 * fb).cpu().numpy(), rtol=1e-6)
        outs.append((g.cpu().numpy(), sq.cpu().numpy()))
    assert abs(outs[0][1][1] - norms_np.astype(np.float64).sum()) <= 1e-5 * norms_np.astype(np.float64).sum()
    assert abs(outs[0][1][2] - (g_mid ** 2).sum()) <= 1e-5 * (g_mid ** 2).sum()
    close(outs[0][0], want, rtol=1e-4, atol_scale=1e-6, name="segmented scatter")
    for o in outs[1:]:
        assert np.array_equal(o[0], outs[0][0]) and np.array_equal(o[1], outs[0][1])        # bit for bit


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,k,N,ncat", [(64, 1, 20, 500, 7), (200, 7, 20, 46033, 40), (5, 40, 20, 30, 3), (33, 3, 20, 12, 2),
                                          (257, 2, 20, 1000, 1), (16, 5, 64, 3000, 500)])


def test_eval_diversity_kernel_equals_the_reference_loops(lib, B, T, k, N, ncat):
    """tcar_eval_diversity (ILD / unexp pair counts + the coverage map, model_combine.py:174-194,301-313) against the oracle's
    literal double loops (oracle/metrics_oracle.py: getILD / getUnexp restated line by line) on random top-k lists: few
    categories (many equal pairs), one category (all zero), T = 1, a catalog SHORTER than k (the list then has N entries:
    topk pads with -1), k = 64.  The counts are integers and the host divides int by int in double precision like Python:
    the metrics must agree EXACTLY, not to a tolerance."""
    _need_gpu()
    from oracle import metrics_oracle
    from tcar_amd.host import metrics as host_metrics
    r = np.random.RandomState(B * 7 + T)
    cat = r.randint(0, ncat, size=N).astype(np.int32)
    reverse_item = {i: "art%d" % i for i in range(N)}
    category_id = {"art%d" % i: int(cat[i]) for i in range(N)}
    n_list = min(k, N)
    topk = np.full((B, k), -1, dtype=np.int32)
    for b in range(B):
        topk[b, :n_list] = r.permutation(N)[:n_list]
    seq = r.randint(1, N + 1, size=(B, T)).astype(np.int32)
    dev = "cuda"
    d_topk, d_seq, d_cat = (torch.tensor(x, device=dev) for x in (topk, seq, cat))
    out = torch.full((3, B), -7, dtype=torch.int32, device=dev)
    seen = torch.zeros(N, dtype=torch.uint8, device=dev)
    assert lib.tcar_eval_diversity(B, T, k, N, ptr(d_topk), ptr(d_seq), ptr(d_cat), ptr(out[0]), ptr(out[1]), ptr(out[2]),
                                   C.c_void_p(seen.data_ptr()), None) == 0
    torch.cuda.synchronize()
    ild_c, un_c, n_rec = (x.cpu().numpy() for x in out)
    assert (n_rec == n_list).all()
    ild, un = host_metrics.diversity_from_counts(ild_c, un_c, n_rec, T)
    for b in range(B):
        rec = topk[b, :n_list].tolist()
        assert ild[b] == metrics_oracle.ild(rec, reverse_item, category_id), b
        assert un[b] == metrics_oracle.unexp(seq[b].tolist(), rec, reverse_item, category_id), b
    want_seen = np.zeros(N, dtype=np.uint8)
    want_seen[np.unique(topk[topk >= 0])] = 1
    assert (seen.cpu().numpy() == want_seen).all()
    # bad arguments are refused before any launch
    assert lib.tcar_eval_diversity(B, T, 65, N, ptr(d_topk), ptr(d_seq), ptr(d_cat), ptr(out[0]), ptr(out[1]), None, None, None) == -1
    assert lib.tcar_eval_diversity(B, 0, k, N, ptr(d_topk), ptr(d_seq), ptr(d_cat), ptr(out[0]), ptr(out[1]), None, None, None) == -1


def _bf(x):
    """fp32 -> the value of its bf16 hi plane (round to nearest even), as fp64"""
    return torch.tensor(np.asarray(x, dtype=np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


# (tile: the dE launcher's code — 0 / 256 / 128 / 64 = row tiles of the double-buffered form; 1923 / 1283 = the three-stage LDS ring
#  of round 6 on 192- / 128-row tiles, 1922 / 2562 = the double-buffered 192- / 256-row tiles under their A/B codes)
@pytest.mark.parametrize("N,B,tile", [(3000, 100, 0), (46033, 512, 0), (46033, 512, 256), (46033, 512, 128), (5754, 600, 64), (700, 33, 0),
                                      (46033, 512, 1923), (3000, 100, 1923), (5754, 600, 1283), (46033, 512, 2562), (700, 33, 1922)])


def test_onehot_gradient_gemms_and_candidate_time_backward(lib, N, B, tile):
    """The one-hot form of the two scoring GRADIENT GEMMs (round 4) at op level, through the C-ABI, against fp64 numpy on the
    bf16-rounded operands AND against the materialised form it replaces:
      tcar_gemm_bf16_dx_onehot + tcar_reduce_dact_onehot  ==  dlogits [E_ic | E_time] through tanh'  (E_time = OH T_clip)
      tcar_gemm_bf16_de_qz + tcar_cand_time_bwd_onehot    ==  tcar_gemm_bf16_perm + tcar_cand_time_bwd_indexed
    i.e. the IndexedSlices gradient of the five time tables' candidate-side lookups through the max_norm clip and its S5 norm
    pieces (model_combine.py:86-92,135-138,156), table rows with norm > 1 and < 1, ragged N and B."""
    from tcar_amd._lib import Dims, Grads
    rng = np.random.RandomState(N + B)
    ldh, ldt, ic, pt = 256, 64, 512, 320
    ek = ic + pt
    d = Dims(N, 250, 64, ldh, ldt)
    Bp, Npad = (B + 127) // 128 * 128, (N + 127) // 128 * 128
    vocab, rowoff = [13, 32, 8, 25, 61], [0, 13, 45, 53, 78]
    tabs = [(rng.standard_normal((v, ldt)) * (0.2 if k % 2 else 0.08)).astype(np.float32) for k, v in enumerate(vocab)]
    for t in tabs:
        t[0] = 0.0                                         # zero-pad rows exist (modules.py:33-34) and are looked up
    mw = np.stack([rng.randint(0, v, N) for v in vocab], 1).astype(np.int32)
    dl = (rng.standard_normal((B, N)) * 0.01).astype(np.float32)
    att = np.tanh(rng.standard_normal((B, ek))).astype(np.float32)
    E = (rng.standard_normal((N, ek)) * 0.3).astype(np.float32)
    raw = np.concatenate(tabs, 0).astype(np.float64)
    nrm = np.sqrt((raw ** 2).sum(1))
    sc = np.where(nrm > 1, 1.0 / np.maximum(nrm, 1e-30), 1.0)
    tclip_np = raw * sc[:, None]
    assert (nrm > 1).any() and (nrm < 1).any()
    rows = np.stack([rowoff[k] + mw[:, k] for k in range(5)], 1)              # [N, 5] table row of every candidate
    E[:, ic:] = tclip_np[rows].reshape(N, pt).astype(np.float32)               # candidate_publish_t (model_combine.py:86-92)
    dev = "cuda"
    T = lambda x, dt=None: torch.tensor(np.ascontiguousarray(x), device=dev) if dt is None else torch.tensor(np.ascontiguousarray(x), device=dev, dtype=dt)
    d_tabs = [T(t) for t in tabs]
    tt = (C.c_void_p * 5)(*[t.data_ptr() for t in d_tabs])
    d_mw, d_att = T(mw), T(att)
    # planes: dlogits [B rows, N inner], E [N rows, ek inner], packed attout [B rows, ldh + pt], one-hot [N rows, 160], scores
    dl_p = np.zeros((B, Npad), np.float32)                   # the engine's planes are [*, Npad]: catalog padded to 128 rows / columns
    dl_p[:, :N] = dl
    E_p = np.zeros((Npad, ek), np.float32)
    E_p[:N] = E
    dlh, _, dl_in, _ = _planes(lib, dl_p)
    eh, _, e_in, _ = _planes(lib, E_p)
    aph, _, ap_in, _ = _planes(lib, np.concatenate([att[:, :ldh], att[:, ic:]], 1))
    oh = torch.zeros(Npad * 160, dtype=torch.bfloat16, device=dev)
    assert lib.tcar_time_onehot(C.byref(d), ptr(d_mw), ptr2(oh), 160, None) == 0
    ph, pl = torch.zeros(Bp * 160, dtype=torch.bfloat16, device=dev), torch.zeros(Bp * 160, dtype=torch.bfloat16, device=dev)
    tclip = torch.zeros(160 * ldt + 320, device=dev)
    assert lib.tcar_time_scores_clip(C.byref(d), C.byref(tt), B, ptr(d_att), ek, ptr2(ph), ptr2(pl), 160, ptr(tclip), None) == 0
    tc = tclip.cpu().numpy()
    close(tc[:139 * ldt].reshape(139, ldt), tclip_np, rtol=1e-6, atol_scale=1e-7, name="clipped rows")
    close(tc[160 * ldt:160 * ldt + 139], sc, rtol=1e-6, name="clip scales")
    assert (tc[160 * ldt + 160:160 * ldt + 160 + 139] == (nrm > 1)).all()
    dlb, Eb, attb = _bf(dl), _bf(E), _bf(att)
    # ---- dX: slabs of dlogits [E_ic | OH], then the reduce + expansion + tanh'
    splitk = 7
    S = lib.tcar_gemm_splitk_effective(Npad, splitk)
    slabs = torch.full((S, B, ic + 160), 7.0, device=dev)
    assert lib.tcar_gemm_bf16_dx_onehot(B, ic, Npad, ptr2(dlh), dl_in, B, ptr2(eh), e_in, Npad, ptr2(oh), 160, ptr(slabs), ic + 160,
                                        splitk, None) == 0
    OH = np.zeros((N, 160))
    OH[np.arange(N)[:, None], rows] = 1.0
    want_dp = dlb @ OH
    got = slabs.sum(0).cpu().numpy()
    close(got[:, :ic], dlb @ Eb[:, :ic], rtol=1e-3, atol_scale=1e-5, name="dX item|content columns")
    close(got[:, ic:ic + 139], want_dp[:, :139], rtol=1e-3, atol_scale=1e-5, name="dP = dlogits OH")
    # the other tile shapes of this GEMM through the caller's switch copy: 256 x 384 (round 6, long contractions: its second column
    # tile takes columns 384..511 from the E plane and 512..671 from the one-hot plane), 512 x 128, and the three-stage ring of
    # 32-deep stages on the default tile (TCAR_BF16_KS = 4) — the same sums up to the order of the k blocks
    for sw in (dict(TCAR_BF16_TILE=384), dict(TCAR_BF16_TILE=512), dict(TCAR_BF16_KS=4), dict(TCAR_BF16_TILE=384, TCAR_BF16_KS=1)):
        tune = _lib.tuning(**sw)
        slabs_v = torch.full((S, B, ic + 160), 7.0, device=dev)
        assert lib.tcar_gemm_bf16_dx_onehot_tuned(C.byref(tune), B, ic, Npad, ptr2(dlh), dl_in, B, ptr2(eh), e_in, Npad, ptr2(oh), 160,
                                                  ptr(slabs_v), ic + 160, splitk, None) == 0
        got_v = slabs_v.sum(0).cpu().numpy()
        close(got_v[:, :ic], dlb @ Eb[:, :ic], rtol=1e-3, atol_scale=1e-5, name="dX item|content columns %r" % sw)
        close(got_v[:, ic:ic + 139], want_dp[:, :139], rtol=1e-3, atol_scale=1e-5, name="dP = dlogits OH %r" % sw)
        if sw == dict(TCAR_BF16_KS=4):      # same tile, same k order inside a slab: the ring changes WHEN a stage lands, not what is summed
            assert torch.equal(slabs_v, slabs)
    negpart = (rng.standard_normal((B, ic)) * 0.01).astype(np.float32)
    dattout, dP = torch.full((B, ek), 7.0, device=dev), torch.full((B, 160), 7.0, device=dev)
    assert lib.tcar_reduce_dact_onehot(ptr(slabs), S, B, ic, ic + 160, ptr(T(negpart)), ic, ptr(d_att), ek, ptr(tclip), ptr(dattout),
                                       ek, ptr(dP), None, None, None) == 0
    dact = 1.0 - att.astype(np.float64) ** 2
    want_t = np.concatenate([want_dp[:, rowoff[k]:rowoff[k] + vocab[k]] @ tclip_np[rowoff[k]:rowoff[k] + vocab[k]] for k in range(5)], 1)
    want_dx = np.concatenate([dlb @ Eb[:, :ic] + negpart, want_t], 1) * dact
    close(dattout.cpu().numpy(), want_dx, rtol=1e-3, atol_scale=1e-5, name="d attout (one-hot form)")
    close(dP.cpu().numpy()[:, :139], want_dp[:, :139], rtol=1e-3, atol_scale=1e-5, name="dP buffer")
    # (the materialised form reads the time planes of E in bf16: the same columns to bf16 rounding of T_clip)
    close(dattout.cpu().numpy()[:, ic:], (dlb @ Eb[:, ic:]) * dact[:, ic:], rtol=2e-2, atol_scale=5e-3, name="vs dlogits E_time (bf16 planes)")
    # ---- dE: item block + (q, z) pairs, then the table gradients; against fp64 and against the materialised launch pair
    order = np.argsort((rows.T.reshape(-1)), kind="stable")                   # inverted index: (k, n) pairs sorted by table row
    inv_off = np.zeros(140, dtype=np.int32)
    inv_off[1:] = np.cumsum(np.bincount(rows.T.reshape(-1), minlength=139))
    et_perm = np.empty(5 * N, dtype=np.int32)
    et_perm[order] = np.arange(5 * N, dtype=np.int32)
    d_perm, d_off, d_invn = T(et_perm), T(inv_off), T((order % N).astype(np.int32))
    Gi = torch.full((N, ldh), 7.0, device=dev)
    qz = torch.full((5 * N, 2), 7.0, device=dev)
    K = (B + 31) & ~31
    assert lib.tcar_gemm_bf16_de_qz(N, K, ptr2(dlh), dl_in, Bp, ptr2(aph), ap_in, Bp, ldh, ptr(Gi), ldh, ptr(d_mw), ptr(d_perm), ptr(tclip),
                                    ptr(qz), tile, None) == 0
    gy = (dlb.T @ attb[:, ic:]).reshape(N, 5, ldt)                            # [N, k, 64] time block of dE (never stored)
    close(Gi.cpu().numpy(), dlb.T @ attb[:, :ldh], rtol=1e-3, atol_scale=1e-5, name="dE item block")
    want_q, want_z = (gy ** 2).sum(2), (gy * tclip_np[rows]).sum(2)          # [N, 5]
    got_qz = qz.cpu().numpy()[et_perm.reshape(5, N)]                           # [5, N, 2]
    close(got_qz[..., 0].T, want_q, rtol=1e-3, atol_scale=1e-5, name="q = ||gy||^2")
    close(got_qz[..., 1].T, want_z, rtol=1e-3, atol_scale=1e-5, name="z = x . gy")
    NSLOT = _lib.NSLOT

    def grads():
        gsm, sqn = torch.zeros(150 * ldt, device=dev), torch.zeros(NSLOT, device=dev)
        gr = Grads()
        gr.g_pos, gr.g_dur, gr.sqn = gsm.data_ptr(), gsm.data_ptr() + 4 * 139 * ldt, sqn.data_ptr()
        for k in range(5):
            gr.g_time[k] = gsm.data_ptr() + 4 * rowoff[k] * ldt
            gr.slot_time[k] = 2 + k
        return gsm, sqn, gr

    ws = torch.zeros(int(lib.tcar_cand_time_ws_floats(C.byref(d))), device=dev)
    gsm, sqn, gr = grads()
    assert lib.tcar_cand_time_bwd_onehot(C.byref(d), B, ptr(d_off), ptr(qz), ptr(dP), ptr(d_att), ek, ptr(tclip), ptr(ws), C.byref(gr),
                                         None) == 0
    # fp64 restatement: per (n, k) slice gx = J(row)^T gy (S1); table gradient = sum of the slices, norm piece = sum ||gx||^2 (S5)
    want_g, want_n = np.zeros((139, ldt)), np.zeros(5)
    S_exact = want_dp[:, :139].T @ np.concatenate([att[:, ic:].astype(np.float64)], 1)     # [139, 320]: row r uses block k(r)
    for k in range(5):
        for v in range(vocab[k]):
            r = rowoff[k] + v
            sel = rows[:, k] == r
            Ssum = S_exact[r, k * ldt:(k + 1) * ldt]
            x = tclip_np[r]
            if nrm[r] > 1:
                want_g[r] = sc[r] * (Ssum - x * (x @ Ssum))
                want_n[k] += sc[r] ** 2 * (want_q[sel, k].sum() - (want_z[sel, k] ** 2).sum())
            else:
                want_g[r] = Ssum
                want_n[k] += want_q[sel, k].sum()
    got_g = gsm.cpu().numpy()[:139 * ldt].reshape(139, ldt)
    close(got_g, want_g, rtol=2e-3, atol_scale=2e-5, name="time-table gradients (one-hot form)")
    close(sqn.cpu().numpy()[2:7], want_n, rtol=2e-3, name="S5 norm pieces (one-hot form)")
    # the materialised pair: dE with its [N, 5 ldt] block in list order + the indexed backward
    det = torch.zeros(5 * N * ldt, device=dev)
    Gi2 = torch.zeros(N, ldh, device=dev)
    assert lib.tcar_gemm_bf16_perm(2, N, ldh + pt, K, ptr2(dlh), None, dl_in, Bp, ptr2(aph), None, ap_in, Bp, ptr(Gi2), ldh, ptr(det), pt,
                                   ldh, ptr(d_perm), ldt, 1, 1, None) == 0
    gsm2, sqn2, gr2 = grads()
    assert lib.tcar_cand_time_bwd_indexed(C.byref(d), C.byref(tt), ptr(d_invn), ptr(d_off), ptr(det), 1, ptr(ws), C.byref(gr2), None) == 0
    close(Gi.cpu().numpy(), Gi2.cpu().numpy(), rtol=1e-5, atol_scale=1e-6, name="item block: both forms")
    # (the list SUM uses fp32 attout in the one-hot form, the bf16 plane in the materialised one: bf16-level agreement)
    close(got_g, gsm2.cpu().numpy()[:139 * ldt].reshape(139, ldt), rtol=2e-2, atol_scale=5e-3, name="table gradients: both forms")
    close(sqn.cpu().numpy()[2:7], sqn2.cpu().numpy()[2:7], rtol=1e-3, name="norm pieces: both forms")


@pytest.mark.parametrize("B", [1, 7, 512, 1030])
def test_query_mlp_backward_kernel(lib, B):
    """tcar_query_mlp_bwd: dq1 = (dq Wq2^T) * relu'(q1), dclick = dq1 Wq1^T (modules.py:138-139 backward) in one launch against
    fp64, ragged B (sessions per workgroup = 4), relu' exactly zero where q1 == 0."""
    from tcar_amd._lib import Dims
    rng = np.random.RandomState(B)
    d = Dims(1000, 250, 64, 256, 64)
    dq = (rng.standard_normal((B, 512)) * 0.3).astype(np.float32)
    q1 = np.maximum(rng.standard_normal((B, 256)), 0).astype(np.float32)           # post-relu: about half the entries are 0
    w1 = (rng.standard_normal((128, 256)) * 0.1).astype(np.float32)
    w2 = (rng.standard_normal((256, 512)) * 0.1).astype(np.float32)
    t = lambda x: torch.tensor(x, device="cuda")
    ddq, dq1_, dw1, dw2 = t(dq), t(q1), t(w1), t(w2)
    o1, o2 = torch.full((B + 3, 256), 7.0, device="cuda"), torch.full((B + 3, 128), 7.0, device="cuda")
    assert lib.tcar_query_mlp_bwd(C.byref(d), B, ptr(ddq), ptr(dq1_), ptr(dw1), ptr(dw2), ptr(o1), ptr(o2), None) == 0
    want1 = (dq.astype(np.float64) @ w2.astype(np.float64).T) * (q1 > 0)
    want2 = want1 @ w1.astype(np.float64).T
    close(o1[:B].cpu().numpy(), want1, rtol=1e-5, atol_scale=1e-6, name="dq1")
    close(o2[:B].cpu().numpy(), want2, rtol=1e-5, atol_scale=1e-6, name="dclick")
    assert (o1[B:] == 7.0).all() and (o2[B:] == 7.0).all()
    again1, again2 = torch.empty_like(o1), torch.empty_like(o2)
    assert lib.tcar_query_mlp_bwd(C.byref(d), B, ptr(ddq), ptr(dq1_), ptr(dw1), ptr(dw2), ptr(again1), ptr(again2), None) == 0
    assert torch.equal(again1[:B], o1[:B]) and torch.equal(again2[:B], o2[:B])        # fixed summation order
    # layer-1 half alone (dq = NULL: dq1 is an input — the default step's form on the aux stream): the same dclick bits
    o3 = torch.full((B + 3, 128), 7.0, device="cuda")
    assert lib.tcar_query_mlp_bwd(C.byref(d), B, None, None, ptr(dw1), None, ptr(o1), ptr(o3), None) == 0
    assert torch.equal(o3[:B], o2[:B]) and (o3[B:] == 7.0).all()
    bad = Dims(1000, 300, 64, 320, 64)
    assert lib.tcar_query_mlp_bwd(C.byref(bad), B, ptr(ddq), ptr(dq1_), ptr(dw1), ptr(dw2), ptr(o1), ptr(o2), None) == -1
