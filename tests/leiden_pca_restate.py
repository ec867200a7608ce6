"""Sequential NumPy / plain-Python restatement of the PCA route of the Leiden subclustering (include/icnv.h, K18;
.leiden_seurat_preprocess_routine, R/inferCNV_tumor_subclusters.R:699-723): the yardstick the GPU is held to.

  stage 1  mean / variance: K15's exact moments (hspike_restate.group_gene_tables); trend: the library's host fit
           (infercnv_amd.loess_fit, itself under test in test_leiden_pca_host.py) of log10(var) on log10(mean) over the
           genes with var > 0; sd_e = sqrt(10^fit); v_std = (sum over the cells in order of min(sqrt(n), (x - mean) / sd_e)^2)
           / (n - 1), one rounding per operation; 0 for a gene outside the fit; features = head(order(-v_std), 2000).
  stage 2  z = min(10, (x - mean) / sqrt(var)), 0 for a constant gene; Z is (F, n).
  stage 3  npcs = min(10, F - 1, n - 1); top eigenvectors of Z Z^T by numpy.linalg.eigh, largest-magnitude entry positive;
           E[c, j] = the sequential sum over f of Z[f, c] V[f, j].
  stage 4  exact kNN of E's rows (K8: d2 = sequential sum of rounded squares of rounded differences, ties by position);
           s_ij = |N(i) n N(j)|, kept iff 16 s >= 2 k, weight = (2 s 2^24 + d) // (2 d) with d = 2 k - s; a loop at every node.
  stage 5  leiden_restate's move / refine / aggregate on the weighted graph: level-0 edge weights w, strength = row sum +
           2 * 2^24 per loop, node weight 1 (CPM, gamma * 2^24) or the strength (modularity, gamma / sum strength)."""
import math

import numpy as np

import leiden_restate as lr
from infercnv_amd.loess_fit import loess_fit, window_points

ONE = 1 << 24
NFEATURES = 2000
NPCS = 10


class Fallback(Exception):
    """The reference's FindVariableFeatures would warn: the problem goes the simple route."""


def moments(expr, genes, cells):
    """K15's mean and variance (n - 1) of expr[genes, cells] per gene."""
    from hspike_restate import group_gene_tables
    sub = np.asarray(expr, dtype=np.float64)[np.asarray(genes)]
    m, v, _ = group_gene_tables(sub, [np.asarray(cells, dtype=np.int64)])
    return m[0], v[0]


def trend_sd(mean, var):
    pos = var > 0
    if np.any(mean[pos] <= 0):
        raise ValueError("mean <= 0")
    m = int(np.count_nonzero(pos))
    if window_points(m) < 4:
        raise Fallback("q < 4")
    fit, ok = loess_fit(np.log10(mean[pos]), np.log10(var[pos]))
    if not ok:
        raise Fallback("degenerate window")
    sd = np.zeros(mean.size)
    sd[pos] = np.sqrt(np.power(10.0, fit))
    return sd


def v_std(X, mean, sd_e):
    """X: (genes, n) the problem's block.  The sequential sum down the cells, vectorised over the genes."""
    n = X.shape[1]
    vmax = math.sqrt(float(n))
    acc = np.zeros(X.shape[0])
    fit = sd_e != 0
    for c in range(n):
        d = (X[fit, c] - mean[fit]) / sd_e[fit]
        d = np.where(d > vmax, vmax, d)
        acc[fit] = acc[fit] + d * d
    acc[fit] = acc[fit] / float(n - 1)
    return acc


def features(v):
    return np.argsort(-np.asarray(v), kind="stable")[:min(NFEATURES, len(v))]


def scale(X, mean, var):
    sd = np.sqrt(var)
    Z = np.zeros(X.shape)
    ok = sd != 0
    Z[ok] = (X[ok] - mean[ok, None]) / sd[ok, None]
    return np.where(Z > 10.0, 10.0, Z)


def eigvecs(M, npcs):
    lam, vec = np.linalg.eigh(M)
    V = np.ascontiguousarray(vec[:, ::-1][:, :npcs])
    for j in range(npcs):
        if V[int(np.argmax(np.abs(V[:, j]))), j] < 0:
            V[:, j] = -V[:, j]
    return lam[::-1][:npcs].copy(), V


def project(Z, V):
    E = np.zeros((Z.shape[1], V.shape[1]))
    for f in range(Z.shape[0]):
        E = E + Z[f][:, None] * V[f][None, :]
    return E


def knn(E, k):
    """K8 on the rows of E: d2 summed over the components in order, (d2, position) ascending, self included."""
    n = E.shape[0]
    out = np.empty((n, k), dtype=np.int32)
    for i in range(n):
        d2 = np.zeros(n)
        for j in range(E.shape[1]):
            t = E[:, j] - E[i, j]
            d2 = d2 + t * t
        out[i] = np.lexsort((np.arange(n), d2))[:k]
    return out


def snn_weight(s, k):
    d = 2 * k - s
    return (2 * s * ONE + d) // (2 * d)


def snn_keep(s, k):
    return 16 * s >= 2 * k


def snn(nn_idx):
    """(off, col, shared, weight, loop) of one (n, k) block: plain sets, row by row."""
    nn = np.asarray(nn_idx)
    n, k = nn.shape
    sets = [set(int(x) for x in row) for row in nn]
    if any(len(s) != k for s in sets):
        raise ValueError("snn: an nn_idx row repeats an entry")   # the library's ICNV_ERR_ARG
    rev = [[] for _ in range(n)]
    for i in range(n):
        for m in sets[i]:
            rev[m].append(i)
    off, col, shared, weight = [0], [], [], []
    for i in range(n):
        cnt = {}
        for m in sets[i]:
            for j in rev[m]:
                cnt[j] = cnt.get(j, 0) + 1
        for j in sorted(cnt):
            if j != i and snn_keep(cnt[j], k):
                col.append(j)
                shared.append(cnt[j])
                weight.append(snn_weight(cnt[j], k))
        off.append(len(col))
    return (np.asarray(off, dtype=np.int64), np.asarray(col, dtype=np.int32), np.asarray(shared, dtype=np.int32),
            np.asarray(weight, dtype=np.int64), np.ones(n, dtype=np.int32))


def leiden_graph(off, col, weight, loop, objective, gamma, beta=0.01, n_iterations=2, seed=0, token=0, loop_weight=ONE, stats=None):
    """leiden_restate.leiden with level-0 edge weights: (1-based membership, number of clusters).  gamma is in units of the
    weights for CPM."""
    if stats is None:
        stats = {"levels": 0, "move_visits": 0, "refine_visits": 0, "draws": 0}
    off0, col0, ew0 = [int(x) for x in off], [int(x) for x in col], [int(x) for x in weight]
    n = len(off0) - 1
    s = [sum(ew0[off0[i]:off0[i + 1]]) + 2 * loop_weight * int(loop[i]) for i in range(n)]
    w0 = [1] * n if objective == lr.CPM else s
    r = float(gamma) if objective == lr.CPM else float(gamma) / float(sum(s))
    memb_orig = list(range(n))
    for it in range(n_iterations):
        o, c, ew, w = off0, col0, ew0, w0
        memb = list(memb_orig)
        agg_of = np.arange(n)
        level = 0
        while True:
            if level >= lr.MAX_LEVELS:
                raise lr.CapExceeded("levels")
            stats["levels"] += 1
            N = len(w)
            order = lr.generator(seed, token, 1, it, level, 0).permutation(N)
            mv, K = lr._move(o, c, ew, w, memb, r, order, stats)
            if K == N:
                final = mv
                break
            rm, R = lr._refine(o, c, ew, w, mv, K, r, beta, seed, token, it, level, stats)
            if R == N:
                amap, n2 = mv, K
                nxt = list(range(K))
            else:
                amap, n2 = rm, R
                nxt = [0] * R
                for v in range(N):
                    nxt[rm[v]] = int(mv[v])
            o, c, ew, w = lr._aggregate(o, c, ew, w, [int(a) for a in amap], n2)
            agg_of = np.asarray(amap)[agg_of]
            memb = nxt
            level += 1
        memb_orig, _ = lr._renumber(np.asarray(final)[agg_of])
        memb_orig = [int(x) for x in memb_orig]
    out = np.asarray(memb_orig, dtype=np.int32) + 1
    return out, int(out.max()) if n else 0


def stages(expr, genes, cells, k):
    """Stages 1-4 of one problem, everything on the host: a dict of the intermediates.  Raises Fallback."""
    expr = np.asarray(expr, dtype=np.float64)
    genes, cells = np.asarray(genes), np.asarray(cells)
    X = expr[np.ix_(genes, cells)]
    mean, var = moments(expr, genes, cells)
    sd_e = trend_sd(mean, var)
    vs = v_std(X, mean, sd_e)
    feat = features(vs)
    npcs = min(NPCS, feat.size - 1, cells.size - 1)
    if npcs < 1:
        raise Fallback("npcs < 1")
    Z = scale(X[feat], mean[feat], var[feat])
    M = Z @ Z.T
    lam, V = eigvecs(M, npcs)
    E = project(Z, V)
    nn = knn(E, k)
    off, col, shared, weight, loop = snn(nn)
    return dict(mean=mean, var=var, sd_e=sd_e, v_std=vs, features=feat, Z=Z, M=M, eigenvalues=lam, V=V, E=E, nn_idx=nn, row_off=off,
                col=col, shared=shared, weight=weight, loop=loop, npcs=npcs)


def routine(expr, genes, cells, k, gamma, objective, beta=0.01, n_iterations=2, seed=0, token=0):
    """The whole route for one problem: a 1-based membership (the simple route's on a fallback)."""
    try:
        st = stages(expr, genes, cells, k)
    except Fallback:
        X = np.asarray(expr, dtype=np.float64)[np.ix_(np.asarray(genes), np.asarray(cells))].T
        return lr.leiden(knn(X, k), objective, gamma, beta, n_iterations, seed, token)[0]
    g = gamma * ONE if objective == lr.CPM else gamma
    return leiden_graph(st["row_off"], st["col"], st["weight"], st["loop"], objective, g, beta, n_iterations, seed, token)[0]
