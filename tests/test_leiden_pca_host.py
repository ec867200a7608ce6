"""CPU tests of the PCA route of the Leiden subclustering (DESIGN K18): the host trend fit, the integer SNN rules of the
restatement, the argument validation of the new entry points (no GPU needed), the driver's hooks and the precondition of
the end-to-end GPU test (the restatement alone recovers the planted clones)."""
import ctypes as ct
import logging
import os

import numpy as np
import pytest

import leiden_pca_restate as pr
import leiden_restate as lr
from infercnv_amd import GeneOrder, InfercnvObject, _lib
from infercnv_amd import tumor_subclusters as ts
from infercnv_amd.loess_fit import loess_fit, window_points


def planted_clones(n=200, G=60, n_clones=4, per=5, seed=0, shift=0.6, noise=0.05):
    """Values around 1 (the scale of the matrix at run() step 15); clone c is `shift` up in its own `per` genes.
    Returns (genes x cells matrix, clone of every cell)."""
    rng = np.random.default_rng(seed)
    lab = np.arange(n) % n_clones
    X = 1.0 + rng.normal(0, noise, size=(G, n))
    for c in range(n_clones):
        X[c * per:(c + 1) * per][:, lab == c] += shift
    return X, lab


def planted_obj(**kw):
    X, lab = planted_clones(**kw)
    G, n = X.shape
    obj = InfercnvObject(expr_data=X, gene_order=GeneOrder(chr=np.repeat(["chr1", "chr2", "chr3"], G // 3)),
                         observation_grouped_cell_indices={"tumor": np.arange(n)})
    return obj, lab


# ---------------------------------------------------------------------------------------------------- loess_fit
def test_loess_fit_reproduces_a_quadratic_at_every_point():
    rng = np.random.default_rng(0)
    for m in (14, 37, 300):
        x = rng.uniform(-2.0, 3.0, size=m)
        y = 1.5 - 0.75 * x + 0.25 * x * x
        fit, ok = loess_fit(x, y)
        assert ok
        # Cramer's rule on u in [-1, 1] with q >= 4 points: relative errors of a few hundred ulps at the most
        assert np.max(np.abs(fit - y)) <= 1e-10 * np.max(np.abs(y))


def test_loess_fit_is_local():
    """A kink far to the right changes the fit only where a window reaches it."""
    m = 200
    x = np.linspace(0.0, 1.0, m)
    y = 2.0 * x
    y2 = y.copy()
    y2[x > 0.9] += 5.0 * (x[x > 0.9] - 0.9)
    a, ok_a = loess_fit(x, y)
    b, ok_b = loess_fit(x, y2)
    assert ok_a and ok_b
    q = window_points(m)
    first_changed = int(np.flatnonzero(x > 0.9)[0])
    untouched = np.arange(m) < first_changed - q           # no window of q consecutive points reaches the kink
    assert np.array_equal(a[untouched], b[untouched])
    assert np.max(np.abs(a[~untouched] - b[~untouched])) > 0.01
    assert np.max(np.abs(b[x > 0.95] - y[x > 0.95])) > 0.05   # a global quadratic would have spread this over every point


def test_loess_fit_order_and_degenerate_windows():
    rng = np.random.default_rng(1)
    x = rng.uniform(0, 1, 50)
    y = np.sin(3 * x)
    perm = rng.permutation(50)
    a, _ = loess_fit(x, y)
    b, _ = loess_fit(x[perm], y[perm])
    assert np.array_equal(a[perm], b)                       # distinct x: the input order does not matter
    assert window_points(13) == 3 and window_points(14) == 4 and window_points(10) == 3   # floor(0.3 m + 1e-5)
    fit, ok = loess_fit(np.repeat([1.0, 2.0], 10), np.arange(20.0))   # windows of one distinct x
    assert not ok


def test_trend_sd_fallbacks_and_errors():
    rng = np.random.default_rng(2)
    mean = rng.uniform(0.5, 2.0, 9)
    var = rng.uniform(0.01, 0.02, 9)
    sd, why = ts.vst_trend_sd(mean, var)                    # 9 genes: q = 2 < 4
    assert sd is None and "span" in why
    mean = rng.uniform(0.5, 2.0, 40)
    var = rng.uniform(0.01, 0.02, 40)
    var[3] = 0.0
    sd, why = ts.vst_trend_sd(mean, var)
    assert why is None and sd[3] == 0.0 and np.all(sd[np.arange(40) != 3] > 0)
    mean[5] = -0.1
    with pytest.raises(ValueError, match="mean <= 0"):
        ts.vst_trend_sd(mean, var)


# ---------------------------------------------------------------------------------------------------- integer SNN rules
def test_snn_weights_are_the_rounded_fixed_point_jaccard_index():
    from fractions import Fraction
    for k in range(1, 129):
        for s in range(1, k + 1):
            exact = Fraction(s * (1 << 24), 2 * k - s)
            want = int(exact + Fraction(1, 2))              # round half up: floor(x + 1/2)
            assert pr.snn_weight(s, k) == want
            assert abs(Fraction(pr.snn_weight(s, k), 1 << 24) - Fraction(s, 2 * k - s)) <= Fraction(1, 1 << 25)
    assert pr.snn_weight(20, 20) == 1 << 24


def test_snn_prune_rule_is_the_double_comparison():
    for k in range(1, 129):
        for s in range(0, k + 1):
            pruned = (s / (2 * k - s)) < (1 / 15)           # Seurat's ComputeSNN in doubles
            assert pr.snn_keep(s, k) == (not pruned), (s, k)
    assert pr.snn_keep(1, 8) and not pr.snn_keep(1, 9)      # equality at k = 8 is kept


def test_restated_snn_on_a_small_block():
    nn = np.array([[0, 1], [1, 0], [2, 1], [3, 2]], dtype=np.int32)
    off, col, shared, weight, loop = pr.snn(nn)
    dense = np.zeros((4, 4), dtype=np.int64)
    A = np.zeros((4, 4), dtype=np.int64)
    A[np.repeat(np.arange(4), 2), nn.ravel()] = 1
    S = A @ A.T
    for i in range(4):
        for t in range(off[i], off[i + 1]):
            dense[i, col[t]] = shared[t]
    np.fill_diagonal(S, 0)
    assert np.array_equal(dense, S) and np.array_equal(dense, dense.T)      # k = 2: every shared count is kept
    assert np.array_equal(loop, np.ones(4))
    assert weight[0] == pr.snn_weight(2, 2) == 1 << 24                        # rows 0 and 1 share both neighbours


def test_weighted_restatement_with_unit_weights_is_the_knn_restatement():
    """leiden_graph on the kNN graph with every weight 1 and the kNN graph's loops reproduces leiden_restate.leiden."""
    rng = np.random.default_rng(3)
    X = rng.normal(size=(60, 3))
    X[:30] += 4.0
    nn = pr.knn(X, 5)
    off, col, strength = lr.snn_graph(nn)
    loop = np.array([int(i in nn[i]) for i in range(60)])
    for obj, gam in ((lr.CPM, 0.05), (lr.MODULARITY, 1.0)):
        want, K = lr.leiden(nn, obj, gam, 0.01, 2, seed=5, token=9)
        got, Kg = pr.leiden_graph(off, col, np.ones(col.size, dtype=np.int64), loop, obj, gam, 0.01, 2, seed=5, token=9, loop_weight=1)
        assert K == Kg and np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------------- edge-shape inputs
# The inputs of tests/test_gpu_leiden_pca_edges.py and what makes them edge cases, shown here on the restatement alone.
RULER9 = (0, 1, 5, 12, 25, 27, 35, 41, 44)      # Golomb rulers: every difference of two marks occurs once
RULER8 = (0, 1, 4, 9, 15, 22, 32, 34)


def shift_block(n, shifts):
    """The kNN block nn[i] = (i + d) mod n for d in shifts."""
    return ((np.arange(n)[:, None] + np.asarray(shifts)[None, :]) % n).astype(np.int32)


def shared_counts(nn):
    """|N(i) n N(j)| of every pair as a dense matrix, the diagonal zeroed."""
    n, k = nn.shape
    A = np.zeros((n, n), dtype=np.int64)
    A[np.repeat(np.arange(n), k), nn.ravel()] = 1
    assert np.all(A.sum(axis=1) == k)           # no row repeats an entry
    S = A @ A.T
    np.fill_diagonal(S, 0)
    return S


def gram_int_input(F, n, seed):
    """(K, Z): K int64 (F, n) with entries in -16 .. 16, a random sign and magnitude each; Z = K / 8 in [-2, 2]."""
    K = np.random.default_rng([seed, F, n]).integers(-16, 17, size=(F, n))
    return K, K / 8.0


GRAM_F = (1, 16, 63, 64, 65, 128, 129)
GRAM_N = (2, 7, 30, 32, 33, 64, 4097)           # ldz = 2, 8, 30, 32, 34, 64, 4098


def vstd_clip_case():
    """(X (5 genes, 4 cells), mean, sd) at n = 4, sqrt(n) = 2: gene 0 has a cell at d = 2 exactly, gene 1 one ulp above it,
    gene 2 a cell at d = -1000, gene 3 is outside the fit (sd = 0), gene 4 has a cell at d = 30."""
    rng = np.random.default_rng(41)
    mean, sd = np.full(5, 1.0), np.full(5, 0.5)
    X = 1.0 + 0.5 * rng.uniform(-1.0, 1.0, size=(5, 4))
    X[0, 1] = 2.0
    mean[1] = 0.0
    X[1] -= 1.0
    X[1, 2] = 1.0 + 2.0 ** -52
    X[2, 0] = 1.0 - 500.0
    sd[3] = 0.0
    X[4, 3] = 16.0
    return X, mean, sd


def plant_scale_clips(X, mean, var, genes, cells):
    """In the block X[genes, cells] (>= 2 cells): gene 0 gets z = 10 exactly and z one ulp above 10, gene 1 (if listed)
    z = 198 and z = -2002, gene 2 (if listed) a zero variance.  mean and var are per listed gene."""
    g, c = np.asarray(genes), np.asarray(cells)
    mean[0], var[0] = 1.0, 0.25
    X[g[0], c[0]], X[g[0], c[1]] = 6.0, 6.0 + 2.0 ** -50
    if g.size > 1:
        mean[1], var[1] = 1.0, 0.25
        X[g[1], c[0]], X[g[1], c[1]] = 100.0, -1000.0
    if g.size > 2:
        var[2] = 0.0


def test_ruler_blocks_share_at_most_one_neighbour():
    for n in (100, 89):
        nn = shift_block(n, RULER9)
        S = shared_counts(nn)
        assert S.max() == 1 and 16 * 1 < 2 * 9                     # two rows share at most one node: every entry is pruned
        off, col, shared, weight, loop = pr.snn(nn)
        assert col.size == 0 and not off.any() and off.size == n + 1 and np.array_equal(loop, np.ones(n))
    nn = shift_block(100, RULER8)
    S = shared_counts(nn)
    off, col, shared, weight, loop = pr.snn(nn)
    assert S.max() == 1 and 16 * 1 == 2 * 8                          # the prune rule binds with equality: kept
    assert np.array_equal(np.diff(off), np.full(100, 56)) and np.all(shared == 1)
    assert np.all(weight == pr.snn_weight(1, 8))


def test_complete_and_k128_blocks():
    nn = shift_block(5, range(5))                                    # n = k = 5: rows are the rotations of 0 .. 4
    off, col, shared, weight, loop = pr.snn(nn)
    assert np.array_equal(np.diff(off), np.full(5, 4)) and np.all(shared == 5) and np.all(weight == 1 << 24)
    for i in range(5):
        assert np.array_equal(col[off[i]:off[i + 1]], np.setdiff1d(np.arange(5), [i]))
    off, col, shared, weight, loop = pr.snn(shift_block(128, range(128)))
    assert col.size == 16256 and np.all(shared == 128) and np.all(weight == 1 << 24)
    off, col, shared, weight, loop = pr.snn(shift_block(129, range(128)))
    assert col.size == 16512 and np.all(shared == 127) and np.all(weight == pr.snn_weight(127, 128))


def test_restated_snn_refuses_a_repeated_entry():
    """N(i) is a set (include/icnv.h): the library refuses a row that repeats an entry, and so does the restatement."""
    nn = np.array([[0, 1], [1, 1], [2, 1], [3, 2]], dtype=np.int32)
    with pytest.raises(ValueError, match="repeats an entry"):
        pr.snn(nn)


def test_integer_gram_inputs_are_exact_in_float64():
    worst = 0
    for F in GRAM_F:
        for n in GRAM_N:
            K, Z = gram_int_input(F, n, 7)
            assert np.array_equal(Z * 8.0, K) and np.abs(Z).max() <= 2.0
            P = K @ K.T
            assert P.dtype == np.int64 and np.array_equal(Z @ Z.T, P / 64.0) and np.array_equal((P / 64.0) * 64.0, P)
            worst = max(worst, int((np.abs(K) @ np.abs(K).T).max()))   # 64 |any partial sum, in any order|
            if n >= 7:                                                 # rows differ: a shifted tile gives another product
                assert len({r.tobytes() for r in K}) == F
            if F >= 16:                                                # columns differ: so does a shifted stage or segment
                assert len({c.tobytes() for c in K.T}) == n
    assert 0 < worst < 2 ** 53                   # so 64 |M| < 2^53 as well: every sum of the products z_a z_b is exact


def test_planted_clips_bind_and_are_met_with_equality():
    X, mean, sd = vstd_clip_case()
    n = X.shape[1]
    vmax = np.sqrt(float(n))
    d = (X[sd != 0] - mean[sd != 0, None]) / sd[sd != 0, None]
    assert n == 4 and vmax == 2.0
    assert d[0, 1] == vmax                                          # met with equality
    assert d[1, 2] == np.nextafter(2.0, 3.0) > vmax and d[3, 3] == 30.0 > vmax    # it binds (sd[3] = 0: row 3 of d is gene 4)
    assert d[2, 0] == -1000.0                                       # a large negative d is not clipped
    v = pr.v_std(X, mean, sd)
    X2 = X.copy()
    X2[1, 2], X2[4, 3] = 1.0, 2.0                                   # d = 2 in place of the planted values
    assert np.array_equal(v, pr.v_std(X2, mean, sd)) and v[3] == 0.0 and v[2] > 1000.0 ** 2 / 3 and v[4] < 30.0 ** 2 / 3
    rng = np.random.default_rng(43)
    X = rng.normal(size=(3, 2))
    mean, var = rng.normal(size=3), rng.uniform(0.5, 2.0, size=3)
    plant_scale_clips(X, mean, var, np.arange(3), np.arange(2))
    assert np.sqrt(0.25) == 0.5
    raw = (X[:2] - mean[:2, None]) / np.sqrt(var[:2, None])
    assert raw[0, 0] == 10.0 and raw[0, 1] == np.nextafter(10.0, 11.0) and raw[1, 0] == 198.0 and raw[1, 1] == -2002.0
    Z = pr.scale(X, mean, var)
    assert Z[0, 0] == 10.0 and Z[0, 1] == 10.0 and Z[1, 0] == 10.0 and Z[1, 1] == -2002.0 and not Z[2].any()


# ---------------------------------------------------------------------------------------------------- C ABI without a GPU
NAMES = ("icnv_lpca_vstd_dev", "icnv_lpca_scale_dev", "icnv_lpca_gram_dev", "icnv_lpca_project_dev", "icnv_snn_begin_dev",
         "icnv_snn_fill_dev", "icnv_snn_end", "icnv_leiden_graph_dev")


def test_entry_points_are_declared_bound_and_exported():
    L = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "icnv.h")).read()
    for name in NAMES:
        assert name in _lib.PROTOTYPES and hasattr(L, name) and name + "(" in header


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(_lib._ip)


def test_argument_validation_needs_no_gpu():
    import torch
    L = _lib.load()
    buf = np.zeros(64)
    p = ct.c_void_p(buf.ctypes.data)      # never dereferenced: every call below fails before any device work
    g, gp = _i32([0, 1, 2])
    go, gop = _i32([0, 3])
    c, cp = _i32([0, 1, 2, 3])
    co, cop = _i32([0, 4])

    def vstd(G=3, C=4, ld=3, gp=gp, gop=gop, cp=cp, cop=cop, P=1, fn=L.icnv_lpca_vstd_dev):
        return fn(p, G, C, ld, gp, gop, cp, cop, P, p, p, p, None)

    for fn in (L.icnv_lpca_vstd_dev, L.icnv_lpca_scale_dev):
        assert vstd(G=0, fn=fn) == _lib.ERR_ARG
        assert vstd(ld=2, fn=fn) == _lib.ERR_ARG
        assert vstd(P=0, fn=fn) == _lib.ERR_ARG
        assert vstd(G=2, ld=2, fn=fn) == _lib.ERR_ARG                       # gene index 2 out of range
        assert vstd(C=3, fn=fn) == _lib.ERR_ARG                             # cell index 3 out of range
        assert vstd(gop=_i32([0, 0])[1], fn=fn) == _lib.ERR_ARG             # a problem without genes
        assert vstd(cop=_i32([1, 4])[1], fn=fn) == _lib.ERR_ARG
        assert fn(None, 3, 4, 3, gp, gop, cp, cop, 1, p, p, p, None) == _lib.ERR_ARG
    assert vstd(cop=_i32([0, 1])[1]) == _lib.ERR_ARG                        # one cell: no n - 1
    assert b"fewer than 2 cells" in L.icnv_last_error()

    nf, nfp = _i32([3])
    nc, ncp = _i32([4])
    assert L.icnv_lpca_gram_dev(p, nfp, ncp, 0, p, None) == _lib.ERR_ARG
    assert L.icnv_lpca_gram_dev(p, _i32([0])[1], ncp, 1, p, None) == _lib.ERR_ARG
    assert L.icnv_lpca_gram_dev(None, nfp, ncp, 1, p, None) == _lib.ERR_ARG
    assert L.icnv_lpca_project_dev(p, p, nfp, ncp, _i32([0])[1], 1, p, 10, None) == _lib.ERR_ARG
    assert L.icnv_lpca_project_dev(p, p, nfp, ncp, _i32([11])[1], 1, p, 10, None) == _lib.ERR_ARG     # npcs > e_ld
    assert L.icnv_lpca_project_dev(p, p, nfp, ncp, _i32([2])[1], 1, p, 65, None) == _lib.ERR_ARG

    h, nnz = ct.c_void_p(0), ct.c_int64(-1)
    off, offp = _i32([0, 4])

    def begin(k=2, offp=offp, P=1, nn=p):
        rc = L.icnv_snn_begin_dev(nn, k, offp, P, ct.byref(h), ct.byref(nnz), None)
        assert h.value is None and nnz.value == -1
        return rc

    assert begin(k=0) == _lib.ERR_ARG
    assert begin(k=5) == _lib.ERR_ARG
    assert begin(offp=_i32([1, 4])[1]) == _lib.ERR_ARG
    assert begin(offp=_i32([0, 4, 2])[1], P=2) == _lib.ERR_ARG
    assert begin(nn=None) == _lib.ERR_ARG
    assert begin(k=129, offp=_i32([0, 200])[1]) == _lib.ERR_UNSUPPORTED
    assert L.icnv_snn_fill_dev(None, p, p, p, p, p, None) == _lib.ERR_ARG
    L.icnv_snn_end(None)

    res = np.array([0.1])
    memb = np.full(4, -3, dtype=np.int32)
    ncl = np.full(1, -4, dtype=np.int32)

    def graph(loop_weight=1 << 24, offp=offp, P=1, obj=1, res=res, beta=0.01, iters=2, row=p):
        rc = L.icnv_leiden_graph_dev(row, p, p, p, loop_weight, offp, P, obj, res.ctypes.data_as(_lib._dp), beta, iters, 0, None,
                                     memb.ctypes.data_as(ct.c_void_p), ncl.ctypes.data_as(_lib._ip), None)
        assert (memb == -3).all() and (ncl == -4).all()       # untouched on error
        return rc

    assert graph(row=None) == _lib.ERR_ARG
    assert graph(loop_weight=0) == _lib.ERR_ARG
    assert graph(P=0) == _lib.ERR_ARG
    assert graph(offp=_i32([1, 4])[1]) == _lib.ERR_ARG
    assert graph(offp=_i32([0, 0])[1]) == _lib.ERR_ARG
    assert graph(obj=3) == _lib.ERR_ARG
    assert graph(res=np.array([-1.0])) == _lib.ERR_ARG
    assert graph(beta=0.0) == _lib.ERR_ARG
    assert graph(iters=0) == _lib.ERR_ARG
    if not torch.cuda.is_available():       # valid arguments reach the device: a HIP error, not a crash or a silent success
        assert vstd() == _lib.ERR_HIP
        assert L.icnv_lpca_gram_dev(p, nfp, ncp, 1, p, None) == _lib.ERR_HIP
        assert begin() == _lib.ERR_HIP
        assert graph() == _lib.ERR_HIP


# ---------------------------------------------------------------------------------------------------- driver
def test_driver_sends_the_default_route_through_the_graph_hook(monkeypatch, caplog):
    """define_signif_tumor_subclusters(obj) with R's defaults (leiden_method = "PCA") no longer raises: the PCA batch goes to
    leiden_graph_fn with CPM's gamma in units of 2^24, a problem that falls back to leiden_fn, one log line each."""
    import torch
    obj = InfercnvObject(expr_data=np.ones((30, 65)), gene_order=GeneOrder(chr=np.repeat(["chr1", "chr2", "chr3"], 10)),
                         observation_grouped_cell_indices={"a": np.arange(30), "b": np.arange(30, 65)})
    seen = {}

    def fake_stages(x, genes, cells, k_nn):
        seen["stages"] = ([g.tolist() for g in genes], [c.tolist() for c in cells], k_nn)
        return {"fallback": [(0, "span is too small")], "active": [1], "n_cells": [35], "row_off": "R", "col": "C", "weight": "W",
                "loop": "L"}

    def graph_fn(row_off, col, weight, loop, sizes, objective, gammas, tokens):
        seen["graph"] = (row_off, col, weight, loop, list(sizes), objective, list(gammas), list(tokens))
        return np.array([1] * 20 + [2] * 15, dtype=np.int32)

    def simple_fn(nn_idx, sizes, objective, gammas, tokens):
        seen["simple"] = (list(sizes), objective, list(gammas), list(tokens))
        return np.array([2] * 10 + [1] * 20, dtype=np.int32)

    monkeypatch.setattr(ts, "_to_device", lambda o: None)
    monkeypatch.setattr(ts, "pca_stages", fake_stages)
    monkeypatch.setattr(ts.device, "knn", lambda x, problems, k: (torch.zeros((30, k), dtype=torch.int32), None))
    monkeypatch.setattr(ts.device, "hclust_cells", lambda x, problems, m: [
        (torch.zeros((c.size - 1, 2), dtype=torch.int32), torch.zeros(c.size - 1, dtype=torch.float64),
         torch.arange(1, c.size + 1, dtype=torch.int32)) for _, c in problems])
    with caplog.at_level(logging.INFO, logger="infercnv_amd"):
        out, per_chr = ts.define_signif_tumor_subclusters(obj, leiden_fn=simple_fn, leiden_graph_fn=graph_fn)
    assert per_chr is None
    assert seen["stages"] == ([list(range(30))] * 2, [list(range(30)), list(range(30, 65))], 20)
    assert seen["graph"][:6] == ("R", "C", "W", "L", [35], "CPM")
    assert seen["graph"][6] == [ts.auto_leiden_resolution(35) * (1 << 24)] and seen["graph"][7] == [ts.fnv1a64("b")]
    assert seen["simple"] == ([30], "CPM", [ts.auto_leiden_resolution(30)], [ts.fnv1a64("a")])
    subs = out.tumor_subclusters["subclusters"]
    assert list(subs["a"]) == ["a_s1", "a_s2"] and subs["a"]["a_s1"].tolist() == list(range(10, 30))
    assert list(subs["b"]) == ["b_s1", "b_s2"] and subs["b"]["b_s2"].tolist() == list(range(50, 65))
    lines = [r.getMessage() for r in caplog.records if "Falling back to simple Leiden clustering" in r.getMessage()]
    assert len(lines) == 1 and lines[0].startswith("Got a warning:\n\tspan is too small")


def test_modularity_resolution_is_not_scaled():
    assert ts._graph_resolution("modularity", 1.0) == 1.0 and ts._graph_resolution("CPM", 0.5) == 0.5 * (1 << 24)


# ---------------------------------------------------------------------------------------------------- item 8's precondition
def test_restatement_alone_recovers_the_planted_clones():
    """The inputs of test_gpu_leiden_pca.py::test_default_call_recovers_planted_clones: with leiden_resolution = "auto"
    ((11.98 / 200)^(1 / 1.165) = 0.0893), k_nn = 20, CPM, beta 0.01, 2 iterations, seed 0 and the group's token, the
    restatement puts every clone into a subcluster of its own."""
    obj, lab = planted_obj()
    G, n = obj.expr_data.shape
    memb = pr.routine(obj.expr_data, np.arange(G), np.arange(n), 20, ts.auto_leiden_resolution(n), lr.CPM, 0.01, 2, seed=0,
                      token=ts.fnv1a64("tumor"))
    assert memb.max() == 4
    for c in range(1, 5):
        assert np.unique(lab[memb == c]).size == 1 and np.count_nonzero(memb == c) == 50
