"""Hierarchical clustering on the GPU (icnv_hclust_dev / icnv_hclust_cells_dev, DESIGN K9): fastcluster::hclust as the
reference's subclustering calls it (R/inferCNV_tumor_subclusters.R:191, 582, 609, ...).

icnv_hclust_dev is held bit for bit to the NumPy restatement of tests/hclust_restate.py (same Lance-Williams operation
order, same tie rule); the fused path is held to the reference's own stored hclust objects and to the per-problem calls."""
import os

import numpy as np
import pytest

import hclust_restate as hr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

METHODS = ["ward.D2", "ward.D", "single", "complete", "average", "mcquitty"]
MONOTONE = METHODS   # every supported method is reducible: sorted merge heights are a valid dendrogram


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


def gpu_hclust(dev, D, method):
    m, h, o = dev.hclust(torch.from_numpy(np.ascontiguousarray(D)).cuda(), method)
    return m.cpu().numpy(), h.cpu().numpy(), o.cpu().numpy()


def assert_bit_equal(got, want):
    assert np.array_equal(got[0], want[0]), "merge"
    assert np.array_equal(got[2], want[2]), "order"
    assert np.array_equal(got[1].view(np.int64), want[1].view(np.int64)), "height"


def assert_valid_dendrogram(merge, height, order, n):
    assert merge.shape == (n - 1, 2) and order.shape == (n,)
    assert np.all(np.diff(height) >= 0)
    assert sorted(order.tolist()) == list(range(1, n + 1))
    leaves = merge[merge < 0]
    assert sorted((-leaves).tolist()) == list(range(1, n + 1))
    for i, row in enumerate(merge):
        assert np.all(row[row > 0] <= i)   # a cluster is used only after the step that made it


def random_dist(n, dims=6, seed=0):
    from scipy.spatial.distance import pdist, squareform
    X = np.random.default_rng(seed + n).standard_normal((n, dims))
    return squareform(pdist(X))


# ------------------------------------------------------------------ 1. the reference's own objects, through the HIP path
def test_golden_hclust_cells_reproduces_reference(dev, golden_dir):
    import oracle_c as oc
    import oracle_np as onp
    d = np.load(os.path.join(golden_dir, "infercnv_object_example.npz"))
    g = np.load(os.path.join(golden_dir, "hclust_example.npz"))
    log = onp.log2xplus1(onp.normalize_counts_by_seq_depth(d["count_data"]))
    _, pre = dev.smooth_chain(to_dev(log), oc.chr_starts_from_codes(d["chr_codes"]), [d["ref_normal"]], want_pre_denoise=True)
    genes = np.arange(log.shape[0])
    res = dev.hclust_cells(pre, [(genes, d["obs_tumor"]), (genes, d["ref_normal"])], "ward.D2")
    for grp, (m, h, o) in zip(("tumor", "normal"), res):
        m, h, o = m.cpu().numpy(), h.cpu().numpy(), o.cpu().numpy()
        assert np.array_equal(m, g[f"{grp}_merge"]), grp
        assert np.array_equal(o, g[f"{grp}_order"]), grp
        assert np.max(np.abs(h - g[f"{grp}_height"]) / g[f"{grp}_height"]) <= 1e-12, grp


def test_tumor_subclusters_hclust_record(dev, golden_dir):
    import oracle_np as onp
    from infercnv_amd import tumor_subclusters
    from infercnv_amd.infercnv_object import GeneOrder, InfercnvObject
    rng = np.random.default_rng(5)
    x = rng.standard_normal((40, 30))
    obj = InfercnvObject(expr_data=x, gene_order=GeneOrder(chr=np.array(["chr1"] * 40)))
    cells = np.array([3, 7, 1, 20, 25, 9, 11])
    genes = np.arange(0, 40, 2)
    hc = tumor_subclusters.hclust(obj, cells, genes=genes)
    want = hr.hclust(hr.seq_dist(x[np.ix_(genes, cells)].T), "ward.D2")
    assert np.array_equal(hc.merge, want[0]) and np.array_equal(hc.order, want[2])
    np.testing.assert_allclose(hc.height, want[1], rtol=1e-12)
    assert np.array_equal(hc.height.view(np.int64), want[1].view(np.int64))
    assert hc.method == "ward.D2" and hc.dist_method == "euclidean"
    assert hc.labels.tolist() == [f"cell_{c + 1}" for c in cells]


# ------------------------------------------------------------------ 2./3. bit-equal to the restatement, both paths
@pytest.mark.parametrize("n", [2, 3, 17, 200, 201, 1500, 3000])
def test_hclust_dev_bit_equal_to_restatement(dev, n):
    D = random_dist(n)
    st0 = dev.hclust_stats(reset=True)
    for method in METHODS:
        assert_bit_equal(gpu_hclust(dev, D, method), hr.hclust(D, method))
    st = dev.hclust_stats(reset=True)
    assert st["calls"] == len(METHODS) and st0 is not None
    assert st["lds_problems" if n <= 200 else "hbm_problems"] == len(METHODS)


@pytest.mark.parametrize("n", [2, 17, 200])
def test_hclust_force_hbm_gives_the_same_result(dev, monkeypatch, n):
    D = random_dist(n, seed=3)
    lds = {m: gpu_hclust(dev, D, m) for m in METHODS}
    monkeypatch.setenv("ICNV_HCLUST_FORCE_HBM", "1")
    dev.hclust_stats(reset=True)
    for m in METHODS:
        assert_bit_equal(gpu_hclust(dev, D, m), lds[m])
        assert_bit_equal(lds[m], hr.hclust(D, m))
    assert dev.hclust_stats(reset=True)["hbm_problems"] == len(METHODS)


# ------------------------------------------------------------------ 4. exact ties
@pytest.mark.parametrize("force_hbm", [False, True])
def test_hclust_exact_ties(dev, monkeypatch, force_hbm):
    from scipy.spatial.distance import pdist, squareform
    if force_hbm:
        monkeypatch.setenv("ICNV_HCLUST_FORCE_HBM", "1")
    rng = np.random.default_rng(9)
    base = rng.standard_normal((40, 5))
    dup = np.concatenate([base, base[:25], base[:10]])                        # duplicated cells: zero distances
    lattice = np.array([(i, j) for i in range(12) for j in range(13)], dtype=np.float64)   # many equal distances
    for X in (dup, lattice):
        D = squareform(pdist(X))
        n = D.shape[0]
        for method in METHODS:
            got = gpu_hclust(dev, D, method)
            assert_bit_equal(got, hr.hclust(D, method))
            assert_valid_dendrogram(*got, n)


# ------------------------------------------------------------------ 5. a Leiden-sized batch equals the per-problem calls
def test_hclust_cells_batch_equals_per_problem_calls(dev):
    rng = np.random.default_rng(21)
    G, C = 600, 2500
    x = np.cumsum(rng.standard_normal((G, C)) * 0.1, axis=0)
    xd = to_dev(x)
    problems = []
    for _ in range(300):
        n = int(rng.choice([2, 3, int(rng.integers(4, 60)), int(rng.integers(60, 200)), int(rng.integers(200, 420))]))
        cells = rng.choice(C, size=n, replace=False)
        genes = np.sort(rng.choice(G, size=int(rng.integers(20, G)), replace=False))
        problems.append((genes, cells))
    dev.hclust_stats(reset=True)
    batch = [tuple(t.cpu().numpy() for t in r) for r in dev.hclust_cells(xd, problems, "ward.D2")]
    st = dev.hclust_stats()
    assert st["calls"] == 1 and st["problems"] == 300 and st["lds_problems"] > 0 and st["hbm_problems"] > 0
    for (genes, cells), got in zip(problems, batch):
        (one,) = dev.hclust_cells(xd, [(genes, cells)], "ward.D2")
        assert_bit_equal(got, tuple(t.cpu().numpy() for t in one))
        assert_valid_dendrogram(*got, cells.size)


def test_hclust_cells_matches_restatement_topology(dev):
    """The fused distances are R's sequential dist bit for bit, so the tree is the restatement's bit for bit."""
    rng = np.random.default_rng(4)
    x = rng.standard_normal((300, 500))
    problems = [(np.arange(300), rng.choice(500, size=n, replace=False)) for n in (5, 60, 199, 350)]
    for (genes, cells), r in zip(problems, dev.hclust_cells(to_dev(x), problems, "average")):
        m, h, o = (t.cpu().numpy() for t in r)
        want = hr.hclust(hr.seq_dist(x[np.ix_(genes, cells)].T), "average")
        assert np.array_equal(m, want[0]) and np.array_equal(o, want[2])
        np.testing.assert_allclose(h, want[1], rtol=1e-12)
        assert np.array_equal(h.view(np.int64), want[1].view(np.int64))


# ------------------------------------------------------------------ 6. SciPy at n = 8 000
def test_hclust_ward_matches_scipy_at_8000(dev):
    from scipy.cluster.hierarchy import linkage
    from scipy.spatial.distance import pdist, squareform
    X = np.random.default_rng(8).standard_normal((8000, 10))
    d = pdist(X)
    m, h, o = gpu_hclust(dev, squareform(d), "ward.D2")
    Z = linkage(d, "ward")
    ab = np.sort(Z[:, :2].astype(np.int64), axis=1)
    assert np.array_equal(m, np.where(ab < 8000, -(ab + 1), ab - 8000 + 1))
    np.testing.assert_allclose(h, Z[:, 2], rtol=1e-12, atol=0)
    assert_valid_dendrogram(m, h, o, 8000)


# ------------------------------------------------------------------ 7. bad arguments
def test_hclust_bad_arguments_fail_before_any_launch(dev):
    import ctypes as ct
    from infercnv_amd import _lib
    L = _lib.load()
    st = ct.c_void_p(torch.cuda.current_stream().cuda_stream)
    D = torch.zeros((8, 8), dtype=torch.float64, device="cuda")
    mo = torch.empty(64, dtype=torch.int32, device="cuda")
    ho = torch.empty(64, dtype=torch.float64, device="cuda")
    oo = torch.empty(64, dtype=torch.int32, device="cuda")
    P = lambda t: ct.c_void_p(t.data_ptr())   # noqa: E731
    dev.hclust_stats(reset=True)

    def dev_call(n, ld=8, method=2, dist=D):
        return L.icnv_hclust_dev(P(dist), ld, n, method, P(mo), P(ho), P(oo), st)
    assert dev_call(1) == _lib.ERR_ARG                       # R: must have n >= 2 objects to cluster
    assert dev_call(0) == _lib.ERR_ARG
    assert dev_call(8, ld=7) == _lib.ERR_ARG
    assert L.icnv_hclust_dev(None, 8, 8, 2, P(mo), P(ho), P(oo), st) == _lib.ERR_ARG
    for code in (7, 8, 0, 9, -1):                            # centroid, median, unknown
        assert dev_call(8, method=code) == _lib.ERR_UNSUPPORTED
    for name in ("centroid", "median", "ward"):
        with pytest.raises(_lib.IcnvError):
            dev.hclust(D, name)

    x = to_dev(np.zeros((10, 8)))

    def cells_call(genes, goff, cells, coff, method=2):
        g, gp = _lib.i32(genes)
        go, gop = _lib.i32(goff)
        c, cp = _lib.i32(cells)
        co, cop = _lib.i32(coff)
        return L.icnv_hclust_cells_dev(P(x), 10, 8, gp, gop, cp, cop, len(goff) - 1, method, P(mo), P(ho), P(oo), st)
    g, c = list(range(10)), list(range(8))
    assert cells_call(g, [0, 10], c, [0, 1]) == _lib.ERR_ARG                      # one cell
    assert cells_call(g + g, [0, 10, 20], c, [0, 8, 8]) == _lib.ERR_ARG           # a problem without cells
    assert cells_call(g[:9] + [10], [0, 10], c, [0, 8]) == _lib.ERR_ARG           # gene index out of range
    assert cells_call(g, [0, 10], c[:7] + [8], [0, 8]) == _lib.ERR_ARG            # cell index out of range
    assert cells_call(g, [0, 0], c, [0, 8]) == _lib.ERR_ARG                       # no gene
    assert cells_call(g, [0, 10], c, [0, 8], method=7) == _lib.ERR_UNSUPPORTED
    assert dev.hclust_stats(reset=True)["calls"] == 0

    # a non-finite distance (fastcluster throws): found on the device before the clustering starts
    Dn = torch.from_numpy(random_dist(8)).cuda()
    Dn[2, 5] = Dn[5, 2] = float("nan")
    assert dev_call(8, dist=Dn) == _lib.ERR_ARG
    Dn[2, 5] = Dn[5, 2] = float("inf")
    assert dev_call(8, dist=Dn) == _lib.ERR_ARG
    assert dev.hclust_stats(reset=True)["calls"] == 0
