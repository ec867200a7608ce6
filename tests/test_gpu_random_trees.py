"""The random-trees subclustering on the GPU (icnv_random_trees_dev / icnv_random_trees_matrix_dev, DESIGN K10;
R/inferCNV_tumor_subclusters.random_smoothed_trees.R).

The permutations are held to NumPy's own Generator(Philox), the smoothed and centred matrices bit for bit to the
restatement of tests/random_trees_restate.py, the trees bit for bit to K9's icnv_hclust_cells_dev on the restatement's
matrices, and the whole subclustering to the restatement driven by the same recursion."""
import ctypes as ct

import numpy as np
import pytest

import random_trees_restate as rr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

METHODS = ["ward.D2", "ward.D", "single", "complete", "average", "mcquitty"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infercnv_amd import device
    torch.cuda.set_device(0)
    device.init(0)
    return device


def to_dev(x):
    """A G x C host matrix -> the (C, G) CUDA tensor the device entry points take."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64).T)).cuda()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


# ------------------------------------------------------------------ 1. the permutations are NumPy's
@pytest.mark.parametrize("n,G,genes", [(2, 3, [0, 2]), (3, 4, [1, 3]), (37, 100_000, [0, 77, 99_999]), (1000, 5, [0, 4]),
                                       (70_000, 2, [0, 1])])
def test_permutation_equals_numpy(dev, n, G, genes):
    from infercnv_amd import _lib
    x = np.tile(np.arange(n, dtype=np.float64), (G, 1))            # x[g, c] = c
    xd = to_dev(x)
    cells = np.arange(n)
    for seed, token, r in [(0, 1, 0), (2**63 + 12345, 0xFFFFFFFFFFFFFFFF, 99), (7, 8, 3), (7, 9, 3)]:
        got = dev.random_trees_matrix(xd, cells, 1, seed, token, r, stages=_lib.RT_PERMUTE).cpu().numpy()
        for g in genes:
            assert np.array_equal(got[:, g].astype(np.int64), rr.permutation(seed, token, g, r, n)), (seed, token, g, r)
    a = dev.random_trees_matrix(xd, cells, 1, 7, 8, 3, stages=_lib.RT_PERMUTE).cpu().numpy()
    b = dev.random_trees_matrix(xd, cells, 1, 7, 9, 3, stages=_lib.RT_PERMUTE).cpu().numpy()
    if n > 3:
        assert not np.array_equal(a[:, genes[0]], b[:, genes[0]])   # distinct tokens, distinct streams
    obs = dev.random_trees_matrix(xd, cells, 1, 7, 8, -1, stages=_lib.RT_PERMUTE).cpu().numpy()
    assert np.array_equal(obs, x.T)                                   # the observed matrix is not permuted


# ------------------------------------------------------------------ 2. smoothing and centring, bit for bit
@pytest.mark.parametrize("G", [1, 2, 100, 101, 10_000])
@pytest.mark.parametrize("window", [1, 2, 100, 101, 10_001])
def test_smoothed_centred_bit_equal(dev, G, window):
    from infercnv_amd import _lib
    rng = np.random.default_rng(G + window)
    C = 9
    x = rng.standard_normal((G, C)) * 0.7 + 1.0
    cells = np.array([4, 0, 7, 2, 8])
    xd = to_dev(x)
    for r in (-1, 0, 5):
        for stages, kw in [(_lib.RT_PERMUTE | _lib.RT_SMOOTH | _lib.RT_CENTER, {}),
                           (_lib.RT_PERMUTE | _lib.RT_SMOOTH, {"center": False})]:
            got = dev.random_trees_matrix(xd, cells, window, 11, 12345, r, stages=stages).cpu().numpy()
            want = rr.clade_matrix(x, cells, window, 11, 12345, r, **kw)
            assert np.array_equal(bits(got), bits(want.T)), (r, stages)


# ------------------------------------------------------------------ 3. trees bit-equal to K9 on the restated matrices
def k9_trees(dev, mats, method):
    out = []
    for Z in mats:
        n = Z.shape[1]
        (m, h, o), = dev.hclust_cells(to_dev(Z), [(np.arange(Z.shape[0]), np.arange(n))], method)
        out.append((m.cpu().numpy(), h.cpu().numpy(), o.cpu().numpy()))
    return out


@pytest.mark.parametrize("method", METHODS)
def test_trees_bit_equal_to_k9(dev, method):
    rng = np.random.default_rng(3)
    G, n_iter, window, seed = 40, 2, 7, 99
    sizes = [2, 17, 200, 201, 1500]
    C = sum(sizes) + 10
    x = rng.standard_normal((G, C))
    perm = rng.permutation(C)
    clades, off = [], 0
    for n in sizes:
        clades.append(np.sort(perm[off:off + n]))
        off += n
    tokens = [1000 + p for p in range(len(clades))]
    trees, rand = dev.random_trees(to_dev(x), clades, tokens, window, n_iter, seed, method)
    rand = rand.cpu().numpy()
    for p, cells in enumerate(clades):
        mats = [rr.clade_matrix(x, cells, window, seed, tokens[p], r) for r in range(-1, n_iter)]
        want = k9_trees(dev, mats, method)
        m, h, o = (t.cpu().numpy() for t in trees[p])
        assert np.array_equal(m, want[0][0]) and np.array_equal(o, want[0][2]), (p, method)
        assert np.array_equal(bits(h), bits(want[0][1])), (p, method)
        for r in range(n_iter):
            assert bits(rand[p, r]) == bits(want[r + 1][1].max()), (p, r, method)


# ------------------------------------------------------------------ 4. batch, waves and paths change no bit
def test_batch_waves_and_hbm_path_bit_identical(dev, monkeypatch):
    rng = np.random.default_rng(8)
    G, C, n_iter = 64, 400, 3
    x = to_dev(rng.standard_normal((G, C)))
    clades = [np.sort(rng.choice(C, size=int(rng.integers(2, 260)), replace=False)) for _ in range(40)]
    tokens = [int(t) for t in rng.integers(0, 2**63, size=40)]

    def run(cl, tk):
        trees, rand = dev.random_trees(x, cl, tk, 11, n_iter, 5, "ward.D2")
        return [tuple(t.cpu().numpy() for t in tr) for tr in trees], rand.cpu().numpy()

    dev.random_trees_stats(reset=True)
    batch = run(clades, tokens)
    st = dev.random_trees_stats(reset=True)
    assert st["calls"] == 1 and st["clades"] == 40 and st["permuted"] == 40 * n_iter and st["waves"] == 1

    def same(a, b):
        for (m1, h1, o1), (m2, h2, o2) in zip(a[0], b[0]):
            assert np.array_equal(m1, m2) and np.array_equal(o1, o2) and np.array_equal(bits(h1), bits(h2))
        assert np.array_equal(bits(a[1]), bits(b[1]))

    for p in (0, 7, 39):
        one = run([clades[p]], [tokens[p]])
        same(([batch[0][p]], batch[1][p:p + 1]), one)
    monkeypatch.setenv("ICNV_RT_SCRATCH_MB", "1")
    same(batch, run(clades, tokens))
    assert dev.random_trees_stats(reset=True)["waves"] > 1
    monkeypatch.setenv("ICNV_HCLUST_FORCE_HBM", "1")
    same(batch, run(clades, tokens))


# ------------------------------------------------------------------ 5. end to end through define_signif_...
def make_object(seed=4):
    from infercnv_amd.infercnv_object import GeneOrder, InfercnvObject
    rng = np.random.default_rng(seed)
    G = 240
    nA, nB, nR = 40, 24, 20
    x = 1.0 + rng.normal(0.0, 0.25, size=(G, nA + nB + nR))
    clone = np.repeat([0, 1], nA // 2)
    rng.shuffle(clone)
    A = np.arange(nA)
    x[:80, A[clone == 0]] += 0.8                       # clone 0: a gain on the first chromosome
    x[120:200, A[clone == 1]] -= 0.8                   # clone 1: a loss on the second
    chrs = np.array(["chr1"] * 80 + ["chr2"] * 40 + ["chr3"] * 80 + ["chr4"] * 40)
    obj = InfercnvObject(x, GeneOrder(chrs),
                         reference_grouped_cell_indices={"normal": np.arange(nA + nB, nA + nB + nR)},
                         observation_grouped_cell_indices={"tumA": A, "tumB": np.arange(nA, nA + nB)})
    return obj, A[clone == 0], A[clone == 1]


@pytest.mark.parametrize("cluster_by_groups", [True, False])
def test_define_signif_matches_restatement(dev, cluster_by_groups):
    from infercnv_amd import ops
    from infercnv_amd import tumor_subclusters as ts
    obj, c0, c1 = make_object()
    p_val, method, seed = 0.05, "ward.D2", 3
    out = ts.define_signif_tumor_subclusters_via_random_smooothed_trees(obj, p_val, method, cluster_by_groups, seed=seed)
    assert out.expr_data is obj.expr_data
    sub = ops.subtract_ref_expr_from_obs(obj, inv_log=True).expr_data
    groups = ts.random_trees_groups(obj, cluster_by_groups)
    gaps = []
    inner = rr.clade_fn(sub, 101, seed, ts.RANDOM_TREES_ITERATIONS, method)

    def fn(clades):
        res = inner(clades)
        for (merge, height, order), rand in res:
            mh = float(np.max(height))
            gaps.append(np.min(np.abs(rand - mh)) / mh)
        return res

    hc, want = ts.random_trees_partition(groups, fn, p_val)
    assert min(gaps) >= 1e-9                            # every decision is far from a tie: the comparison is well-posed
    got = out.tumor_subclusters["subclusters"]
    assert list(got) == list(want)
    for g in want:
        assert list(got[g]) == list(want[g]), g
        for name in want[g]:
            assert np.array_equal(got[g][name], want[g][name]), (g, name)
        h = out.tumor_subclusters["hc"][g]
        assert np.array_equal(h.merge, hc[g][0]) and np.array_equal(h.order, hc[g][2])
        np.testing.assert_allclose(h.height, hc[g][1], rtol=1e-9)
        assert h.labels.tolist() == np.asarray(obj.cells())[groups[g]].tolist()
    # the planted clones are recovered: no final subcluster mixes them, and both are split off
    tum = "tumA" if cluster_by_groups else "all_observations"
    names = list(got[tum])
    assert len(names) >= 2
    for name, idx in got[tum].items():
        s = set(idx.tolist())
        assert s <= set(c0.tolist()) or s <= set(c1.tolist()) or not (s & set(c0.tolist()) or s & set(c1.tolist())), name
    if cluster_by_groups:
        assert list(got["tumB"]) == ["tumB.1"]            # the homogeneous group stays whole


# ------------------------------------------------------------------ 6. bad arguments
def test_bad_arguments(dev):
    from infercnv_amd import _lib
    L = _lib.load()
    G, C = 10, 6
    x = to_dev(np.random.default_rng(0).standard_normal((G, C)))
    merge = torch.full((64,), -7, dtype=torch.int32, device="cuda")
    height = torch.full((64,), -7.0, dtype=torch.float64, device="cuda")
    order = torch.full((64,), -7, dtype=torch.int32, device="cuda")
    rand = torch.full((64,), -7.0, dtype=torch.float64, device="cuda")
    dev.random_trees_stats(reset=True)

    def call(cells, off, window=5, n_iter=3, method=2, xx=x, n_prob=None):
        ci, cp = _lib.i32(cells)
        co, cop = _lib.i32(off)
        tok = (ct.c_uint64 * 8)(*range(8))
        return L.icnv_random_trees_dev(ct.c_void_p(xx.data_ptr()), G, C, cp, cop, tok, len(off) - 1 if n_prob is None else n_prob,
                                       window, n_iter, 0, method, ct.c_void_p(merge.data_ptr()), ct.c_void_p(height.data_ptr()),
                                       ct.c_void_p(order.data_ptr()), ct.c_void_p(rand.data_ptr()), None)

    assert call([0, 1, 2], [0, 3]) == _lib.OK
    dev.random_trees_stats(reset=True)
    merge.fill_(-7)
    height.fill_(-7.0)
    order.fill_(-7)
    rand.fill_(-7.0)
    assert call([0], [0, 1]) == _lib.ERR_ARG                     # n_p < 2
    assert call([0, 1], [0, 2], window=0) == _lib.ERR_ARG
    assert call([0, 1], [0, 2], n_iter=0) == _lib.ERR_ARG
    assert call([0, 6], [0, 2]) == _lib.ERR_ARG                  # index out of range
    assert call([0, -1], [0, 2]) == _lib.ERR_ARG
    assert call([0, 1], [0, 2], n_prob=0) == _lib.ERR_ARG
    assert call([0, 1], [0, 2], method=7) == _lib.ERR_UNSUPPORTED   # centroid
    assert call([0, 1], [0, 2], method=8) == _lib.ERR_UNSUPPORTED   # median
    xn = x.clone()
    xn[1, 3] = float("nan")
    assert call([0, 1, 2], [0, 3], xx=xn) == _lib.ERR_ARG        # non-finite input, flagged before any clustering
    xn[1, 3] = float("inf")
    assert call([0, 1, 2], [0, 3], xx=xn) == _lib.ERR_ARG
    torch.cuda.synchronize()
    assert bool((merge == -7).all()) and bool((height == -7.0).all()) and bool((order == -7).all()) and bool((rand == -7.0).all())
    st = dev.random_trees_stats(reset=True)
    assert st["calls"] == 0 and st["waves"] == 0
    from infercnv_amd import tumor_subclusters as ts
    from infercnv_amd.infercnv_object import GeneOrder, InfercnvObject
    obj = InfercnvObject(np.ones((G, C)), GeneOrder(np.array(["1"] * G)), observation_grouped_cell_indices={"a": np.array([2])})
    with pytest.raises(ValueError):
        ts.define_signif_tumor_subclusters_via_random_smooothed_trees(obj, 0.05, "ward.D2", True)
