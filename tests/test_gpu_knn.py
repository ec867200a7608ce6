"""Exact kNN on the GPU (icnv_knn_dev, DESIGN K8): RANN::nn2(t(expr_data), k) of .leiden_simple_snn
(R/inferCNV_tumor_subclusters.R:726) against an oracle that restates the contract in numpy:

  d2_ij = the sequential fp64 sum over the problem's genes in list order of (x[g,i] - x[g,j])^2 -- np.cumsum along the
          genes (a running sum; ndarray.sum() is pairwise and does NOT match), no FMA anywhere in numpy's elementwise ops;
  rank  = np.lexsort((j, d2)); nn_dist = np.sqrt(d2).

Every case requires nn_idx equal and nn_dist bit-equal to the oracle.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infercnv_amd import device
    torch.cuda.set_device(0)
    device.init(0)
    return device


def to_dev(x):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64).T)).cuda()


def oracle_rows(x, genes, cells, k, rows=None):
    """(nn_idx, nn_dist) of the query positions `rows` (default: all) of one problem."""
    X = np.asarray(x, dtype=np.float64)[np.asarray(genes)][:, np.asarray(cells)]     # G_p x n
    n = X.shape[1]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    idx = np.empty((rows.size, k), dtype=np.int32)
    dist = np.empty((rows.size, k), dtype=np.float64)
    j = np.arange(n)
    for t, i in enumerate(rows):
        diff = X[:, i:i + 1] - X
        d2 = np.cumsum(diff * diff, axis=0)[-1]
        order = np.lexsort((j, d2))[:k]
        idx[t] = order
        dist[t] = np.sqrt(d2[order])
    return idx, dist


def run(dev, x, problems, k):
    idx, dist = dev.knn(to_dev(x), problems, k)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), dist.cpu().numpy()


def assert_exact(dev, x, problems, k):
    got_i, got_d = run(dev, x, problems, k)
    r0 = 0
    for genes, cells in problems:
        n = len(cells)
        want_i, want_d = oracle_rows(x, genes, cells, k)
        np.testing.assert_array_equal(got_i[r0:r0 + n], want_i)
        assert np.array_equal(got_d[r0:r0 + n].view(np.uint64), want_d.view(np.uint64)), "nn_dist must be bit-equal"
        r0 += n
    assert r0 == got_i.shape[0]
    return got_i, got_d


def smoothed(rng, G, C):
    """smoothed-like data: per-gene offsets, cell-level structure, running means along the genes"""
    base = rng.normal(0.0, 0.3, size=(G, C)) + rng.normal(0.0, 1.0, size=(G, 1))
    clusters = rng.integers(0, 5, size=C)
    base += rng.normal(0.0, 0.5, size=(G, 5))[:, clusters]
    kern = np.ones(11) / 11.0
    return np.apply_along_axis(lambda v: np.convolve(v, kern, mode="same"), 0, base)


def test_knn_smoothed_g900_c700_k20(dev):
    rng = np.random.default_rng(1)
    x = smoothed(rng, 900, 700)
    assert_exact(dev, x, [(np.arange(900), np.arange(700))], 20)


def test_knn_odd_gene_count(dev):
    rng = np.random.default_rng(2)
    x = smoothed(rng, 333, 150)
    assert_exact(dev, x, [(np.arange(333), rng.permutation(150)[:131])], 7)


@pytest.mark.parametrize("k", [1, 49])
def test_knn_k_extremes(dev, k):
    rng = np.random.default_rng(3 + k)
    x = rng.normal(size=(33, 60))
    assert_exact(dev, x, [(np.arange(33), np.arange(5, 55))], k)


def test_knn_noncontiguous_gene_list(dev):
    rng = np.random.default_rng(4)
    x = smoothed(rng, 500, 120)
    genes = rng.permutation(500)[:211]          # any order: the list order is the summation order
    assert_exact(dev, x, [(genes, np.arange(120))], 15)


def test_knn_batch_of_problems(dev):
    rng = np.random.default_rng(5)
    G, C = 400, 300
    x = smoothed(rng, G, C)
    problems = []
    for p in range(24):
        Gp = 1 if p in (0, 7) else int(rng.integers(2, 200))
        n = int(rng.integers(12, 260))
        problems.append((rng.choice(G, Gp, replace=False), rng.choice(C, n, replace=False)))
    assert_exact(dev, x, problems, 10)


def test_knn_duplicate_cells_tie_at_zero(dev):
    rng = np.random.default_rng(6)
    x = rng.normal(size=(50, 40))
    cells = np.concatenate([np.arange(40), [3, 3, 17, 3, 25]])      # repeated columns: distance 0, lowest position first
    got_i, got_d = assert_exact(dev, x, [(np.arange(50), cells)], 6)
    assert list(got_i[3][:4]) == [3, 40, 41, 43] and np.all(got_d[3][:4] == 0.0)


def test_knn_integer_lattice_many_equal_distances(dev):
    rng = np.random.default_rng(7)
    x = rng.integers(0, 3, size=(12, 400)).astype(np.float64)
    assert_exact(dev, x, [(np.arange(12), np.arange(400))], 20)


def test_knn_near_ties_inside_the_screen_bound(dev):
    """distances a few ulps apart next to cells far away (large norms after centring): the screen cannot order them,
    the exact pass must"""
    rng = np.random.default_rng(8)
    G = 64
    far = rng.normal(0.0, 10.0, size=(G, 60))
    v = rng.normal(0.0, 10.0, size=G)
    near = np.repeat(v[:, None], 40, axis=1)
    for j in range(40):
        near[j % G, j] += 1.0 + (j % 7) * 2.0 ** -50      # d2 to v: (1 + m 2^-50)^2, a few ulps apart, exact ties within a class
    x = np.concatenate([far, v[:, None], near], axis=1)
    got_i, got_d = assert_exact(dev, x, [(np.arange(G), np.arange(x.shape[1]))], 30)
    assert len(set(got_d[60][1:30].tolist())) > 1


def test_knn_large_offset_small_spread(dev):
    rng = np.random.default_rng(9)
    x = 1e3 + 1e-3 * rng.normal(size=(300, 200))
    assert_exact(dev, x, [(np.arange(300), np.arange(200))], 12)


@pytest.mark.parametrize("env", [{"ICNV_KNN_EXHAUSTIVE": "1"}, {"ICNV_KNN_SCRATCH_MB": "1"}, {"ICNV_KNN_CAP": "1"}])
def test_knn_developer_switches_give_identical_output(dev, monkeypatch, env):
    rng = np.random.default_rng(10)
    x = smoothed(rng, 700, 900)
    problems = [(np.arange(700), np.arange(900)), (rng.permutation(700)[:77], rng.permutation(900)[:300])]
    ref_i, ref_d = run(dev, x, problems, 20)
    for kv in env.items():
        monkeypatch.setenv(*kv)
    dev.knn_stats(reset=True)
    got_i, got_d = run(dev, x, problems, 20)
    st = dev.knn_stats(reset=True)
    np.testing.assert_array_equal(got_i, ref_i)
    assert np.array_equal(got_d.view(np.uint64), ref_d.view(np.uint64))
    rows = 1200
    assert st["query_rows"] == rows and st["calls"] == 1
    if "ICNV_KNN_EXHAUSTIVE" in env:
        assert st["forced_exhaustive_rows"] == rows and st["exhaustive_rows"] == rows and st["screened_rows"] == 0
    elif "ICNV_KNN_CAP" in env:
        assert st["overflow_rows"] == rows and st["exhaustive_rows"] == rows       # every row overflows a capacity of 1
    else:
        assert st["row_blocks"] >= 6 and st["exhaustive_rows"] == 0
        assert st["candidates"] >= rows * 20


def test_knn_default_path_stats(dev):
    rng = np.random.default_rng(11)
    x = smoothed(rng, 900, 700)
    dev.knn_stats(reset=True)
    run(dev, x, [(np.arange(900), np.arange(700))], 20)
    st = dev.knn_stats(reset=True)
    assert st["screened_rows"] == 700 and st["exhaustive_rows"] == 0
    assert 700 * 20 <= st["candidates"] <= 700 * 40          # the bound is tight: few candidates beyond k on continuous data


def test_knn_full_size_sampled_rows(dev):
    """20 000 cells x 10 000 genes, k = 20: 64 sampled query rows against the oracle's exact rows (sequential sums over
    the genes in order, accumulated gene by gene for all cells at once -- the same running sum as np.cumsum)."""
    rng = np.random.default_rng(12)
    G, C, k = 10000, 20000, 20
    x = rng.normal(0.0, 1.0, size=(G, C)) * 0.3 + rng.normal(0.0, 1.0, size=(G, 1))
    got_i, got_d = run(dev, x, [(np.arange(G), np.arange(C))], k)
    rows = np.sort(rng.choice(C, 64, replace=False))
    s = np.zeros((rows.size, C))
    for g in range(G):
        t = x[g, rows][:, None] - x[g][None, :]
        s = s + t * t
    j = np.arange(C)
    for t, i in enumerate(rows):
        order = np.lexsort((j, s[t]))[:k]
        np.testing.assert_array_equal(got_i[i], order)
        assert np.array_equal(got_d[i].view(np.uint64), np.sqrt(s[t][order]).view(np.uint64))


def test_knn_neighbour_sets_match_ckdtree(dev):
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(13)
    x = rng.normal(size=(40, 500))
    got_i, _ = run(dev, x, [(np.arange(40), np.arange(500))], 15)
    _, kd = cKDTree(x.T).query(x.T, k=15)
    for i in range(500):
        assert set(got_i[i].tolist()) == set(kd[i].tolist())


def test_knn_per_chr_matches_nn2_loop_and_r_skip_rules(dev):
    from infercnv_amd import GeneOrder, InfercnvObject, tumor_subclusters as ts
    rng = np.random.default_rng(14)
    chrs = np.repeat(["chr1", "chr2", "chr3", "chr4"], [120, 80, 60, 40])
    G = chrs.size
    x = smoothed(rng, G, 260)
    refs = np.arange(0, 30)
    x[(chrs == "chr4")[:, None] & (np.arange(260) < 30)[None, :]] = 0.0       # chr4 genes: every reference value 0 ...
    x[np.ix_(np.flatnonzero(chrs == "chr4"), refs[::2])] = 40.0                # ... or 40: |z| far above 0.8, all outliers
    groups = {"g_big": np.arange(30, 200), "g_mid": np.arange(200, 240), "g_two": np.array([240, 241]),
              "g_small": np.arange(242, 260)}
    obj = InfercnvObject(expr_data=x, gene_order=GeneOrder(chr=chrs),
                         reference_grouped_cell_indices={"normal": refs}, observation_grouped_cell_indices=groups)
    k_nn = 20
    kept = ts.zscore_kept_genes(obj)
    assert not np.any(chrs[kept] == "chr4") and kept.size >= 200
    res, skipped = ts.knn_per_chr(obj, groups, k_nn, chr_levels=["chr1", "chr2", "chr3", "chr4", "chrX"])
    for c in ("chr4", "chrX"):
        for g in groups:
            assert skipped[(c, g)] == "absent"
    for c in ("chr1", "chr2", "chr3"):
        assert skipped[(c, "g_two")] == "too_few"          # ncol < 3
        assert skipped[(c, "g_small")] == "k_nn"           # k_nn >= ncol (18 cells)
        for g in ("g_big", "g_mid"):
            genes = kept[chrs[kept] == c]
            want_i, want_d = ts.nn2(obj, groups[g], k_nn, genes=genes)
            got_i, got_d = res[(c, g)]
            np.testing.assert_array_equal(got_i, want_i)
            assert np.array_equal(got_d.view(np.uint64), want_d.view(np.uint64))
            o_i, _ = oracle_rows(x, genes, groups[g], k_nn, rows=[0, 5])
            np.testing.assert_array_equal(got_i[[0, 5]], o_i)
    assert len(res) == 6


def test_knn_bad_arguments_fail_before_any_launch(dev):
    import ctypes as ct
    from infercnv_amd import _lib
    L = _lib.load()
    x = to_dev(np.zeros((10, 8)))
    out_i = torch.empty((8, 129), dtype=torch.int32, device="cuda")
    out_d = torch.empty((8, 129), dtype=torch.float64, device="cuda")
    dev.knn_stats(reset=True)

    def call(genes, goff, cells, coff, k):
        g, gp = _lib.i32(genes)
        go, gop = _lib.i32(goff)
        c, cp = _lib.i32(cells)
        co, cop = _lib.i32(coff)
        return L.icnv_knn_dev(ct.c_void_p(x.data_ptr()), 10, 8, gp, gop, cp, cop, len(goff) - 1, k, ct.c_void_p(out_i.data_ptr()),
                              ct.c_void_p(out_d.data_ptr()), ct.c_void_p(torch.cuda.current_stream().cuda_stream))
    g, c = list(range(10)), list(range(8))
    assert call(g, [0, 10], c, [0, 8], 0) == _lib.ERR_ARG                 # k < 1
    assert call(g, [0, 10], c, [0, 8], 9) == _lib.ERR_ARG                 # k > n_p
    assert call(g + g, [0, 10, 20], c[:3] + c, [0, 3, 11], 4) == _lib.ERR_ARG   # k > n_p of one problem of the batch
    assert call(g[:9] + [10], [0, 10], c, [0, 8], 2) == _lib.ERR_ARG      # gene index out of range
    assert call(g, [0, 10], c[:7] + [-1], [0, 8], 2) == _lib.ERR_ARG      # cell index out of range
    assert call(g, [0, 0], c, [0, 8], 2) == _lib.ERR_ARG                  # no gene
    assert call(g + g, [0, 10, 20], c, [0, 8, 8], 2) == _lib.ERR_ARG      # a problem without cells
    big = to_dev(np.zeros((10, 200)))
    x = big
    assert call(g, [0, 10], list(range(200)), [0, 200], 129) == _lib.ERR_UNSUPPORTED
    assert dev.knn_stats(reset=True)["calls"] == 0
