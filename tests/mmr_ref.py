"""The numpy model of the MMR walk (include/tcar_mmr.h) that the host and the GPU tests share.

walk_f32 follows the rule in fp32, operation for operation: the pool, 1 / sqrt with correctly rounded sqrt and division, the dot in the
kernel's chain order, sim = dot * (r_i * r_j), v = s - fl(mu * m), the pick under (v, id descending, slot ascending).  ONE difference:
the kernel fuses each multiply-add of a dot and numpy rounds the product first, so the two agree bit for bit where every product and
partial sum of a dot is exact — the exact-arithmetic cases of tests/test_gpu_mmr_walk.py — and within TOL_SIM elsewhere.
walk_f64 is the same rule in fp64 (cosines straight from the definition) and also reports how decisive every session's walk was.
tau_greedy replays a list somebody else produced and measures, in fp64, how far each of its picks was from the best one."""
import numpy as np

MAX_POOL = 256


def pool_of(cand, score, order, N, max_pool=MAX_POOL):
    """the pool of one session: the first max_pool eligible slots of `order` (a slot in [0, C), id in [0, N), score not NaN, not -inf)"""
    C = len(cand)
    out = []
    for s in order:
        if len(out) == max_pool:
            break
        if 0 <= s < C and 0 <= cand[s] < N and not np.isnan(score[s]) and score[s] != -np.inf:
            out.append(int(s))
    return out


def dots_f32(X, y):
    """fp32 dots of the rows of X [P, H] with y [H] in the kernel's order: the columns 8 i + 4 h + q form chain q of half h (i ascending),
    per half (c0 + c1) + (c2 + c3), then half 0 + half 1"""
    P, H = X.shape
    Hp = (H + 7) // 8 * 8
    Xp, yp = np.zeros((P, Hp), np.float32), np.zeros(Hp, np.float32)
    Xp[:, :H], yp[:H] = X, y
    prod = (Xp * yp).reshape(P, Hp // 8, 2, 4)
    acc = np.zeros((P, 2, 4), np.float32)
    for i in range(Hp // 8):
        acc = acc + prod[:, i]
    h = (acc[:, :, 0] + acc[:, :, 1]) + (acc[:, :, 2] + acc[:, :, 3])
    return h[:, 0] + h[:, 1]


def _best(v, ids, slots, taken):
    """the index of the pick: v descending (+0.0 == -0.0), id descending, slot ascending, among the entries not taken"""
    best = None
    for j in range(len(v)):
        if taken[j]:
            continue
        key = (float(v[j]) + 0.0, int(ids[j]), -int(slots[j]))
        if best is None or key > best[0]:
            best = (key, j)
    return best[1]


def _walk(cand, score, order, content, mu, k, fill, f32):
    cand, score, order = np.asarray(cand), np.asarray(score, dtype=np.float32), np.asarray(order)
    content = np.asarray(content, dtype=np.float32)
    B, N = cand.shape[0], content.shape[0]
    real = np.float32 if f32 else np.float64
    topk = np.full((B, k), -1, np.int32)
    out_score, msim = np.full((B, k), fill, np.float32), np.full((B, k), fill, real)
    gaps = np.full(B, np.inf)
    mu_r = real(mu)
    for b in range(B):
        slots = pool_of(cand[b], score[b], order[b], N)
        if not slots:
            continue
        ids, s = cand[b][slots].astype(np.int64), score[b][slots].astype(real)
        X = content[ids]
        if f32:
            ss = np.array([dots_f32(X[j:j + 1], X[j])[0] for j in range(len(slots))], np.float32)
            with np.errstate(divide="ignore"):
                r = np.where(ss > 0, np.float32(1) / np.sqrt(ss, dtype=np.float32), np.float32(0)).astype(np.float32)
        else:
            X = X.astype(np.float64)
            ss = (X * X).sum(1)
            r = np.where(ss > 0, 1.0 / np.sqrt(np.where(ss > 0, ss, 1.0)), 0.0)
        m = np.zeros(len(slots), real)
        taken = np.zeros(len(slots), bool)
        for t in range(min(k, len(slots))):
            v = (s - (mu_r * m).astype(real)).astype(real)
            j = _best(v, ids, slots, taken)
            if not f32:
                rest = [float(v[i]) for i in range(len(slots)) if not taken[i] and i != j]
                if rest:
                    gaps[b] = min(gaps[b], float(v[j]) - max(rest))
            taken[j] = True
            topk[b, t], out_score[b, t], msim[b, t] = ids[j], score[b][slots[j]], m[j]
            d = dots_f32(X, X[j]) if f32 else X @ X[j]
            sim = (d * (r * r[j])).astype(real)
            m = np.fmax(m, sim)
    return topk, out_score, msim, gaps


def walk_f32(cand, score, order, content, mu, k, fill=0.0):
    """cand [B, C] int, score [B, C] f32, order [B, C] int (tcar_cand_rank's), content [N, H] f32 -> (topk [B, k] int32, out_score [B, k]
    f32, msim [B, k] f32); what lies behind a session's last pick holds -1 / fill / fill"""
    return _walk(cand, score, order, content, mu, k, fill, True)[:3]


def walk_f64(cand, score, order, content, mu, k, fill=0.0):
    """the same rule in fp64 -> (topk, out_score, msim f64, gap [B]): gap[b] is the smallest difference, over the steps of session b,
    between the best and the second-best value among the slots not yet taken (inf where a step had no second)"""
    return _walk(cand, score, order, content, mu, k, fill, False)


def tau_greedy(cand, score, order, content, mu, topk):
    """Replay the lists `topk` [B, k] (item ids, -1 behind the last; of the free slots of a repeated id the best one is meant) in fp64: for every
    pick, the best value among the slots that were left minus the value of the pick (0 for the greedy choice), and the fp64 m of the
    pick.  -> (shortfall [B, k], msim [B, k], count [B]: picks per session); entries behind the last pick are 0.  Raises
    AssertionError where a pick is not a pool slot that is still free, or the list ends before min(k, pool)."""
    cand, score, order, topk = np.asarray(cand), np.asarray(score, dtype=np.float32), np.asarray(order), np.asarray(topk)
    content = np.asarray(content, dtype=np.float64)
    B, k = topk.shape
    short, msim, count = np.zeros((B, k)), np.zeros((B, k)), np.zeros(B, np.int64)
    for b in range(B):
        slots = pool_of(cand[b], score[b], order[b], content.shape[0])
        ids, s = cand[b][slots].astype(np.int64), score[b][slots].astype(np.float64)
        X = content[ids]
        ss = (X * X).sum(1)
        r = np.where(ss > 0, 1.0 / np.sqrt(np.where(ss > 0, ss, 1.0)), 0.0)
        m, free = np.zeros(len(slots)), np.ones(len(slots), bool)
        want = min(k, len(slots))
        assert (topk[b, want:] == -1).all() and (topk[b, :want] >= 0).all(), (b, topk[b], want)
        count[b] = want
        for t in range(want):
            hit = np.where((ids == topk[b, t]) & free)[0]
            assert len(hit) >= 1, ("session %d, pick %d: item %d is not a free pool slot" % (b, t, topk[b, t]))
            v = s - mu * m
            j = int(max(hit, key=lambda i: (v[i] + 0.0, -slots[i])))        # of the free twins of one id: the one the rule takes first
            short[b, t], msim[b, t] = v[free].max() - v[j], m[j]
            free[j] = False
            m = np.fmax(m, (X @ X[j]) * (r * r[j]))
    return short, msim, count


def brute_walk(cand, score, content, mu, k):
    """The rule written as plainly as possible, in fp64, for tiny cases without NaN: no `order` — the pool is ALL eligible slots sorted
    by (score, id descending, slot ascending), cut to MAX_POOL.  -> topk [B, k]"""
    cand, score, content = np.asarray(cand), np.asarray(score, dtype=np.float64), np.asarray(content, dtype=np.float64)
    B, C = cand.shape
    out = np.full((B, k), -1, np.int32)
    for b in range(B):
        elig = [c for c in range(C) if 0 <= cand[b, c] < len(content) and score[b, c] != -np.inf]
        elig.sort(key=lambda c: (-(score[b, c] + 0.0), -cand[b, c], c))
        pool, listed = elig[:MAX_POOL], []

        def cos(i, j):
            x, y = content[cand[b, i]], content[cand[b, j]]
            nx, ny = np.sqrt(x @ x), np.sqrt(y @ y)
            return (x @ y) / (nx * ny) if nx > 0 and ny > 0 else 0.0
        for t in range(min(k, len(pool))):
            best = None
            for c in pool:
                if c in listed:
                    continue
                m = max([0.0] + [cos(c, p) for p in listed])
                key = (score[b, c] - mu * m + 0.0, cand[b, c], -c)
                if best is None or key > best[0]:
                    best = (key, c)
            listed.append(best[1])
            out[b, t] = cand[b, best[1]]
    return out
