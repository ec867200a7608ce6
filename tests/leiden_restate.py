"""Sequential NumPy / plain-Python restatement of the Leiden contract of include/icnv.h (icnv_leiden_dev, DESIGN K11): the
yardstick the GPU is held to bit for bit.

  - graph: edge {i, j} (i != j, weight 1) iff j is in row i or i in row j; loop at i iff i is in row i; strength
    s_i = #neighbours + 2 loop_i; neighbour lists ascending, loops never take part in a move.
  - node weights: 1 (CPM) or s_i (modularity); r = gamma (CPM) or gamma / sum(s) (modularity); every weight an exact integer.
  - diff = e_vC - ((w_v * W_C) * r) in doubles, in that order (Python floats are IEEE doubles, one rounding per operation).
  - streams: NumPy's Generator(Philox(key=[seed, token], counter=[0, phase, (it << 32) | l, c])): phase 1 the level's
    visiting order, phase 2 / 3 the refinement order and draws of move cluster c.
  - exp_lib: the library's exp, separately rounded operations in a fixed order (icnv leiden_internal.h)."""
import math
from collections import deque

import numpy as np

CPM, MODULARITY = 1, 2
MAX_LEVELS = 512            # LEIDEN_MAX_LEVELS of leiden_internal.h
EXP_LIB_MAX = 709.0         # exp_lib(x) = +inf above this
INV_LN2 = 1.4426950408889634
LN2_HI = 6.93147180369123816490e-01
LN2_LO = 1.90821492927058770002e-10
EXP_COEF = [1.0 / math.factorial(j) for j in range(12)]   # Horner from the top: 1/11!, ..., 1/2!, 1, 1


class CapExceeded(RuntimeError):
    pass


def move_cap(n):
    """Queue pops allowed in one move phase of n nodes (LEIDEN_MOVE_CAP)."""
    return 256 * n + 1024


def exp_lib(x):
    """The library's exp for x >= 0: k = floor(x / ln2 + 1/2), t = (x - k ln2_hi) - k ln2_lo, p = Horner of the Taylor
    polynomial of degree 11 (separately rounded mul and add), ldexp(p, k).  x > 709 (or NaN): +inf."""
    x = float(x)
    if not (x <= EXP_LIB_MAX):
        return math.inf
    k = math.floor(x * INV_LN2 + 0.5)
    kd = float(k)
    t = (x - kd * LN2_HI) - kd * LN2_LO
    p = EXP_COEF[11]
    for j in range(10, -1, -1):
        p = p * t + EXP_COEF[j]
    return math.ldexp(p, k)


def generator(seed, token, phase, it, level, c):
    bg = np.random.Philox(key=np.array([seed, token], dtype=np.uint64),
                          counter=np.array([0, phase, (it << 32) | level, c], dtype=np.uint64))
    return np.random.Generator(bg)


def snn_graph(nn_idx):
    """(row_off int64 (n+1), col int32, strength int64) of the graph of one problem's (n, k) 0-based nn_idx block."""
    nn = np.asarray(nn_idx, dtype=np.int64)
    n, k = nn.shape
    i = np.repeat(np.arange(n, dtype=np.int64), k)
    j = nn.ravel()
    loop = np.zeros(n, dtype=np.int64)
    loop[i[i == j]] = 1
    m = i != j
    a = np.concatenate([i[m], j[m]])
    b = np.concatenate([j[m], i[m]])
    key = np.unique(a * n + b)
    rows, cols = key // n, key % n
    off = np.zeros(n + 1, dtype=np.int64)
    np.add.at(off, rows + 1, 1)
    off = np.cumsum(off)
    strength = np.diff(off) + 2 * loop
    return off, cols.astype(np.int32), strength


def _renumber(memb):
    """Renumber by first appearance in node order -> (new membership, count)."""
    ids = {}
    out = np.empty(len(memb), dtype=np.int64)
    for v, c in enumerate(memb):
        out[v] = ids.setdefault(int(c), len(ids))
    return out, len(ids)


def _move(off, col, ew, w, memb, r, order, stats):
    N = len(w)
    W = [0] * N
    cnt = [0] * N
    for v in range(N):
        W[memb[v]] += w[v]
        cnt[memb[v]] += 1
    stack = [c for c in range(N) if cnt[c] == 0]
    queue = deque(int(v) for v in order)
    stable = [False] * N
    pops, cap = 0, move_cap(N)
    while queue:
        pops += 1
        if pops > cap:
            raise CapExceeded("move phase")
        v = queue.popleft()
        c0, wv = memb[v], w[v]
        W[c0] -= wv
        cnt[c0] -= 1
        if cnt[c0] == 0:
            stack.append(c0)
        e, seen = {}, []
        for t in range(off[v], off[v + 1]):
            C = memb[col[t]]
            if C not in e:
                e[C] = 0
                seen.append(C)
            e[C] += ew[t]
        best = c0
        bd = float(e.get(c0, 0)) - ((float(wv) * float(W[c0])) * r)
        for C in [stack[-1]] + seen:
            d = float(e.get(C, 0)) - ((float(wv) * float(W[C])) * r)
            if d > bd:
                best, bd = C, d
        if cnt[best] == 0:
            assert stack[-1] == best
            stack.pop()
        memb[v] = best
        W[best] += wv
        cnt[best] += 1
        stable[v] = True
        if best != c0:
            for t in range(off[v], off[v + 1]):
                u = col[t]
                if stable[u] and memb[u] != best:
                    queue.append(u)
                    stable[u] = False
    stats["move_visits"] += pops
    return _renumber(memb)


def _refine(off, col, ew, w, memb, K, r, beta, seed, token, it, level, stats):
    N = len(w)
    rm = list(range(N))
    Wr = list(w)
    nonsingle = [False] * N
    ext = [0] * N
    for v in range(N):
        for t in range(off[v], off[v + 1]):
            if memb[col[t]] == memb[v]:
                ext[v] += ew[t]
    S = [[] for _ in range(K)]
    for v in range(N):
        S[memb[v]].append(v)
    for c in range(K):
        Sc = S[c]
        T = sum(w[v] for v in Sc)
        perm = generator(seed, token, 2, it, level, c).permutation(len(Sc))
        rng = generator(seed, token, 3, it, level, c)
        for i in perm:
            v = Sc[int(i)]
            if nonsingle[v]:
                continue
            wv = w[v]
            if not (float(ext[v]) >= ((float(wv) * float(T - wv)) * r)):
                continue
            stats["refine_visits"] += 1
            Wr[v] = 0
            ext[v] = 0
            e, cands = {v: 0}, [v]
            for t in range(off[v], off[v + 1]):
                u = col[t]
                if memb[u] != c:
                    continue
                D = rm[u]
                if D not in e:
                    e[D] = 0
                    cands.append(D)
                e[D] += ew[t]
            total, cum, best, bd, last = 0.0, [], v, 0.0, 0
            for j, D in enumerate(cands):
                if float(ext[D]) >= ((float(Wr[D]) * float(T - Wr[D])) * r):
                    d = float(e[D]) - ((float(wv) * float(Wr[D])) * r)
                    if d > bd:
                        best, bd = D, d
                    if d >= 0:
                        total = total + exp_lib(d / beta)
                        last = j
                cum.append(total)
            if total < math.inf:
                t_draw = float(rng.random()) * total
                stats["draws"] += 1
                chosen = cands[last]
                for j, D in enumerate(cands):
                    if cum[j] > t_draw:
                        chosen = D
                        break
            else:
                chosen = best
            Wr[chosen] += wv
            for t in range(off[v], off[v + 1]):
                u = col[t]
                if memb[u] != c:
                    continue
                if rm[u] == chosen:
                    ext[chosen] -= ew[t]
                else:
                    ext[chosen] += ew[t]
            rm[v] = chosen
            if chosen != v:
                nonsingle[chosen] = True
    num, R = {}, 0
    for c in range(K):
        for v in S[c]:
            if rm[v] not in num:
                num[rm[v]] = R
                R += 1
    return np.array([num[rm[v]] for v in range(N)], dtype=np.int64), R


def _aggregate(off, col, ew, w, amap, n2):
    w2 = [0] * n2
    for v in range(len(w)):
        w2[amap[v]] += w[v]
    rows = [dict() for _ in range(n2)]
    for v in range(len(w)):
        a = amap[v]
        for t in range(off[v], off[v + 1]):
            b = amap[col[t]]
            if a != b:
                rows[a][b] = rows[a].get(b, 0) + ew[t]
    off2, col2, ew2 = [0], [], []
    for a in range(n2):
        for b in sorted(rows[a]):
            col2.append(b)
            ew2.append(rows[a][b])
        off2.append(len(col2))
    return off2, col2, ew2, w2


def leiden(nn_idx, objective, gamma, beta=0.01, n_iterations=2, seed=0, token=0, stats=None):
    """One problem: (1-based membership int32 (n,), number of clusters)."""
    if stats is None:
        stats = {"levels": 0, "move_visits": 0, "refine_visits": 0, "draws": 0}
    off0, col0, s = snn_graph(nn_idx)
    n = len(s)
    w0 = [1] * n if objective == CPM else [int(x) for x in s]
    r = float(gamma) if objective == CPM else float(gamma) / float(int(s.sum()))
    off0, col0 = [int(x) for x in off0], [int(x) for x in col0]
    memb_orig = list(range(n))
    for it in range(n_iterations):
        off, col, ew, w = off0, col0, [1] * len(col0), w0
        memb = list(memb_orig)
        agg_of = np.arange(n)
        level = 0
        while True:
            if level >= MAX_LEVELS:
                raise CapExceeded("levels")
            stats["levels"] += 1
            N = len(w)
            order = generator(seed, token, 1, it, level, 0).permutation(N)
            mv, K = _move(off, col, ew, w, memb, r, order, stats)
            if K == N:
                final = mv
                break
            rm, R = _refine(off, col, ew, w, mv, K, r, beta, seed, token, it, level, stats)
            if R == N:
                amap, n2 = mv, K
                nxt = list(range(K))
            else:
                amap, n2 = rm, R
                nxt = [0] * R
                for v in range(N):
                    nxt[rm[v]] = int(mv[v])
            off, col, ew, w = _aggregate(off, col, ew, w, [int(a) for a in amap], n2)
            agg_of = np.asarray(amap)[agg_of]
            memb = nxt
            level += 1
        memb_orig, _ = _renumber(np.asarray(final)[agg_of])
        memb_orig = [int(x) for x in memb_orig]
    out = np.asarray(memb_orig, dtype=np.int32) + 1
    return out, int(out.max()) if n else 0


def leiden_batch(nn_idx, sizes, objective, gamma, beta=0.01, n_iterations=2, seed=0, tokens=None):
    """Problems stacked as device.leiden takes them: nn_idx (sum n_p, k), gamma one value or one per problem."""
    nn_idx = np.asarray(nn_idx)
    sizes = [int(x) for x in sizes]
    gam = np.broadcast_to(np.asarray(gamma, dtype=np.float64), (len(sizes),))
    tokens = [0] * len(sizes) if tokens is None else list(tokens)
    memb, ncl, r0 = [], [], 0
    for p, n in enumerate(sizes):
        m, K = leiden(nn_idx[r0:r0 + n], objective, float(gam[p]), beta, n_iterations, seed, int(tokens[p]))
        memb.append(m)
        ncl.append(K)
        r0 += n
    return (np.concatenate(memb) if memb else np.zeros(0, dtype=np.int32)), np.asarray(ncl, dtype=np.int32)
