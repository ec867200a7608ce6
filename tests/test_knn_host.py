"""CPU tests of the exact kNN's host side (DESIGN K8): the reference-based gene filter of define_signif_tumor_subclusters
(R/inferCNV_tumor_subclusters.R:45-71) against a restatement, the SNN adjacency of .leiden_simple_snn (:728-734), the C
ABI's argument validation (no GPU needed: every check runs before any device work) and the export of the entry points."""
import ctypes as ct
import math

import numpy as np
import pytest

from infercnv_amd import GeneOrder, InfercnvObject, _lib, tumor_subclusters as ts


def restated_outliers(x, refs):
    """z = (ref - mean(ref)) / sd(ref); which(rowMeans(|z|) >= 0.8) -- correctly rounded sums (math.fsum)"""
    ref = x[:, refs]
    v = ref.ravel()
    m = math.fsum(v) / v.size
    sd = math.sqrt(math.fsum((t - m) ** 2 for t in v) / (v.size - 1))
    z = np.abs((ref - m) / sd)
    return np.array([g for g in range(z.shape[0]) if math.fsum(z[g]) / z.shape[1] >= 0.8], dtype=np.int64)


def make_obj(x, refs, chrs=None):
    G, C = x.shape
    chrs = np.repeat("chr1", G) if chrs is None else chrs
    obs = np.setdiff1d(np.arange(C), refs)
    return InfercnvObject(expr_data=x, gene_order=GeneOrder(chr=chrs),
                          reference_grouped_cell_indices={"normal": np.asarray(refs)} if len(refs) else {},
                          observation_grouped_cell_indices={"tumor": obs})


def test_zscore_outliers_match_restatement_including_genes_near_the_threshold():
    rng = np.random.default_rng(0)
    G, C = 200, 40
    refs = np.arange(12)
    x = rng.normal(0.0, 1.0, size=(G, C))
    pattern = np.where(np.arange(12) % 2 == 0, 1.0, -1.0)           # mean |.| = 1
    targets = {5: 0.8 + 1e-9, 6: 0.8 - 1e-9, 7: 0.8 + 1e-7, 8: 0.8 - 1e-7}
    for _ in range(60):                                              # the global mean / sd move with the rows: iterate
        ref = x[:, refs]
        m, s = ref.mean(), ref.std(ddof=1)
        for g, a in targets.items():
            x[g, refs] = m + s * a * pattern
    obj = make_obj(x, refs)
    got = ts.zscore_outlier_genes(obj)
    want = restated_outliers(x, refs)
    np.testing.assert_array_equal(got, want)
    assert 5 in got and 7 in got and 6 not in got and 8 not in got
    np.testing.assert_array_equal(ts.zscore_kept_genes(obj), np.setdiff1d(np.arange(G), want))


def test_zscore_filter_switches():
    rng = np.random.default_rng(1)
    x = rng.normal(size=(30, 10))
    assert ts.zscore_outlier_genes(make_obj(x, [])) is None                     # no reference cells
    assert ts.zscore_outlier_genes(make_obj(x, [0, 1, 2]), z_score_filter=0) is None
    np.testing.assert_array_equal(ts.zscore_kept_genes(make_obj(x, [0, 1, 2]), z_score_filter=0), np.arange(30))
    # the filter applies and finds nothing: R's expr.data[-integer(0), ] keeps no row
    flat = np.ones((30, 10))
    flat[:, :4] += np.tile([0.1, -0.1, 0.1, -0.1], (30, 1)) * 0.5           # every gene's mean |z| is the same, below 0.8 ...
    obj = make_obj(flat, [0, 1, 2, 3])
    out = ts.zscore_outlier_genes(obj)
    if out.size == 0:
        assert ts.zscore_kept_genes(obj).size == 0
    else:                                                                      # ... or above it: then every gene goes
        assert out.size == 30


def test_snn_adjacency_is_the_unsymmetrised_knn_graph():
    nn = np.array([[0, 2, 1], [1, 0, 3], [2, 3, 1], [3, 1, 2]])
    A = ts.snn_adjacency(nn)
    assert A.shape == (4, 4) and A.nnz == 12
    dense = np.zeros((4, 4))
    for i in range(4):
        dense[i, nn[i]] = 1.0
    np.testing.assert_array_equal(A.toarray(), dense)
    assert not np.array_equal(dense, dense.T)                                 # igraph's mode = "undirected" symmetrises in R


def _host_call(L, genes, goff, cells, coff, k, G=10, C=8):
    x = np.zeros(G * C)
    n = coff[-1]
    oi = np.zeros(max(n * max(k, 1), 1), dtype=np.int32)
    od = np.zeros(max(n * max(k, 1), 1))
    g, gp = _lib.i32(genes)
    go, gop = _lib.i32(goff)
    c, cp = _lib.i32(cells)
    co, cop = _lib.i32(coff)
    return L.icnv_knn(x.ctypes.data_as(ct.c_void_p), G, C, gp, gop, cp, cop, len(goff) - 1, k, oi.ctypes.data_as(ct.c_void_p),
                      od.ctypes.data_as(ct.c_void_p))


def test_knn_argument_validation_needs_no_gpu():
    L = _lib.load()
    g, c = list(range(10)), list(range(8))
    assert _host_call(L, g, [0, 10], c, [0, 8], 0) == _lib.ERR_ARG
    assert b"k must be" in L.icnv_last_error()
    assert _host_call(L, g, [0, 10], c, [0, 8], 9) == _lib.ERR_ARG
    assert _host_call(L, g[:9] + [10], [0, 10], c, [0, 8], 2) == _lib.ERR_ARG
    assert b"gene index" in L.icnv_last_error()
    assert _host_call(L, g, [0, 10], c[:7] + [8], [0, 8], 2) == _lib.ERR_ARG
    assert b"cell index" in L.icnv_last_error()
    assert _host_call(L, g + g, [0, 10, 20], c[:2] + c, [0, 2, 10], 3) == _lib.ERR_ARG
    assert _host_call(L, g, [0, 10], c, [0, 8], 2, G=10, C=8) != _lib.ERR_UNSUPPORTED
    assert _host_call(L, g, [0, 10], list(range(200)), [0, 200], 129, C=200) == _lib.ERR_UNSUPPORTED
    assert b"128" in L.icnv_last_error()


def test_knn_entry_points_are_declared_bound_and_exported():
    L = _lib.load()
    for name in ("icnv_knn", "icnv_knn_dev", "icnv_knn_stats", "icnv_knn_stats_reset"):
        assert name in _lib.PROTOTYPES and hasattr(L, name)
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "icnv.h")).read()
    for name in ("icnv_knn(", "icnv_knn_dev(", "icnv_knn_stats(", "icnv_knn_stats_reset("):
        assert name in header
