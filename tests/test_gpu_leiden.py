"""Leiden community detection on the GPU (icnv_leiden_dev / icnv_snn_graph_dev, DESIGN K11): cluster_leiden of
.leiden_simple_snn (R/inferCNV_tumor_subclusters.R:726-741) under the library's own contract (include/icnv.h), held bit
for bit to the sequential restatement of tests/leiden_restate.py, and the subclustering driver built on it."""
import ctypes as ct
import os

import numpy as np
import pytest

import leiden_restate as lr

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


def knn_of(X, k):
    """Exact kNN of the rows of X with the K8 tie rule (equal distances by position): (n, k) int32, self included."""
    X = np.asarray(X, dtype=np.float64)
    out = np.empty((X.shape[0], k), dtype=np.int32)
    for i in range(X.shape[0]):
        d = np.sum((X - X[i]) ** 2, axis=1)
        out[i] = np.lexsort((np.arange(X.shape[0]), d))[:k]
    return out


def clones(n, dims=8, n_clones=4, seed=0, sep=6.0):
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, n_clones, size=n)
    X = rng.normal(0.0, 1.0, size=(n, dims))
    X[np.arange(n), lab % dims] += sep
    return X, lab


def knn_fast(X, k):
    from scipy.spatial import cKDTree
    _, idx = cKDTree(X).query(X, k=k)
    return np.asarray(idx, dtype=np.int32).reshape(X.shape[0], k)


def gamma_of(g, n):
    return (11.98 / n) ** (1 / 1.165) if g == "auto" else float(g)


def run_gpu(dev, nn, objective, gamma, beta, iters, seed=0, token=0):
    t = torch.from_numpy(np.ascontiguousarray(nn, dtype=np.int32)).cuda()
    m, ncl = dev.leiden(t, [nn.shape[0]], objective, gamma, beta, iters, seed, [token])
    return m.cpu().numpy(), int(ncl[0])


OBJ = {"CPM": lr.CPM, "modularity": lr.MODULARITY}

CASES = [   # (n, k, objective, gamma, beta, n_iterations)
    (1, 1, "CPM", "auto", 0.01, 2), (2, 1, "modularity", 1, 0.01, 2), (2, 2, "CPM", 0, 0.01, 1),
    (3, 2, "modularity", 1, 1e3, 2), (3, 1, "CPM", 50, 0.05, 5),
    (21, 2, "CPM", "auto", 0.01, 2), (21, 20, "modularity", 1, 0.05, 5), (21, 20, "CPM", 1, 1e3, 2), (21, 1, "CPM", 0, 0.01, 2),
    (200, 20, "CPM", "auto", 0.01, 2), (200, 20, "modularity", 1, 1e3, 2), (200, 128, "CPM", "auto", 0.05, 1),
    (200, 2, "modularity", 50, 0.01, 5), (200, 1, "CPM", 0, 0.01, 2), (200, 20, "CPM", 50, 1e3, 2), (200, 128, "modularity", 0, 1e3, 2),
    (2001, 20, "CPM", "auto", 0.01, 2), (2001, 20, "modularity", 1, 1e3, 2), (2001, 2, "CPM", "auto", 1e3, 5),
    (5000, 20, "modularity", 1, 0.01, 2), (5000, 20, "CPM", "auto", 1e3, 1),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_leiden_identical_to_restatement(dev, case):
    n, k, obj, g, beta, iters = case
    X, _ = clones(n, seed=n + k)
    nn = knn_of(X, k) if n <= 2001 else knn_fast(X, k)
    gam = gamma_of(g, n)
    got, K = run_gpu(dev, nn, obj, gam, beta, iters, seed=3, token=11)
    want, Kw = lr.leiden(nn, OBJ[obj], gam, beta, iters, seed=3, token=11)
    assert K == Kw
    assert np.array_equal(got, want)


@pytest.mark.parametrize("k", [2, 3, 7])
@pytest.mark.parametrize("objective", ["CPM", "modularity"])
def test_leiden_duplicated_cells(dev, k, objective):
    """Groups of identical cells: K8 orders the copies by position, so self is not the first neighbour or is missing."""
    rng = np.random.default_rng(k)
    base = rng.normal(size=(30, 5))
    X = np.repeat(base, 4, axis=0)[rng.permutation(120)]
    nn = knn_of(X, k)
    assert any(nn[i, 0] != i for i in range(120))
    assert any(i not in nn[i] for i in range(120)) == (k < 4)   # 4 copies: self is missing only for k < 4
    for beta in (0.01, 1e3):
        gam = gamma_of("auto", 120) if objective == "CPM" else 1.0
        got, K = run_gpu(dev, nn, objective, gam, beta, 2)
        want, Kw = lr.leiden(nn, OBJ[objective], gam, beta, 2)
        assert K == Kw and np.array_equal(got, want)


def test_snn_graph_is_max_of_a_and_its_transpose(dev):
    from scipy.sparse import csr_matrix
    rng = np.random.default_rng(4)
    X = np.repeat(rng.normal(size=(60, 4)), 2, axis=0)
    sizes = [120, 37, 5]
    nns = [knn_of(X, 5), knn_of(rng.normal(size=(37, 3)), 5), knn_of(rng.normal(size=(5, 2)), 5)]
    t = torch.from_numpy(np.concatenate(nns)).cuda()
    row_off, col, strength = dev.snn_graph(t, sizes)
    row_off, col, strength = row_off.cpu().numpy(), col.cpu().numpy(), strength.cpu().numpy()
    r0 = 0
    for n, nn in zip(sizes, nns):
        A = csr_matrix((np.ones(nn.size), (np.repeat(np.arange(n), nn.shape[1]), nn.ravel())), shape=(n, n))
        A.data[:] = 1
        M = A.maximum(A.T).tolil()
        loops = M.diagonal().astype(np.int64)
        M.setdiag(0)
        M = M.tocsr()
        M.eliminate_zeros()
        M.sort_indices()
        off = row_off[r0:r0 + n + 1] - row_off[r0]
        assert np.array_equal(off, M.indptr)
        assert np.array_equal(col[row_off[r0]:row_off[r0 + n]], M.indices)
        assert np.array_equal(strength[r0:r0 + n], np.diff(M.indptr) + 2 * loops)
        ro, co, so = lr.snn_graph(nn)
        assert np.array_equal(ro, off) and np.array_equal(co, M.indices) and np.array_equal(so, strength[r0:r0 + n])
        r0 += n


def test_batch_equals_per_problem_calls_and_streams_are_keyed(dev):
    rng = np.random.default_rng(9)
    sizes = [int(s) for s in rng.integers(5, 300, size=100)]
    nns = [knn_of(clones(n, seed=i)[0], 5) for i, n in enumerate(sizes)]
    tokens = [int(t) for t in rng.integers(0, 2**63, size=100)]
    gammas = [gamma_of("auto", n) for n in sizes]
    t = torch.from_numpy(np.concatenate(nns)).cuda()
    memb, ncl = dev.leiden(t, sizes, "CPM", gammas, 0.05, 2, 7, tokens)
    memb = memb.cpu().numpy()
    r0 = 0
    for p, n in enumerate(sizes):
        one, K = run_gpu(dev, nns[p], "CPM", gammas[p], 0.05, 2, seed=7, token=tokens[p])
        assert K == ncl[p] and np.array_equal(memb[r0:r0 + n], one), p
        r0 += n
    nn = nns[int(np.argmax(sizes))]
    ref, _ = run_gpu(dev, nn, "CPM", 0.05, 1e3, 2, seed=7, token=1)
    assert not np.array_equal(ref, run_gpu(dev, nn, "CPM", 0.05, 1e3, 2, seed=8, token=1)[0])
    assert not np.array_equal(ref, run_gpu(dev, nn, "CPM", 0.05, 1e3, 2, seed=7, token=2)[0])


def test_fifty_thousand_cells(dev):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    n, k = 50000, 20
    X, lab = clones(n, dims=10, n_clones=5, seed=1, sep=12.0)
    nn = knn_fast(X, k)
    assert np.all(lab[nn] == lab[:, None])       # the clones are apart in the kNN graph
    gam = gamma_of("auto", n)
    a, Ka = run_gpu(dev, nn, "CPM", gam, 0.01, 2)
    b, Kb = run_gpu(dev, nn, "CPM", gam, 0.01, 2)
    assert Ka == Kb and np.array_equal(a, b)
    assert Ka >= 5
    A = csr_matrix((np.ones(nn.size), (np.repeat(np.arange(n), k), nn.ravel())), shape=(n, n))
    A = A.maximum(A.T).tocsr()
    for c in range(1, Ka + 1):
        members = np.flatnonzero(a == c)
        assert np.unique(lab[members]).size == 1, c
        assert connected_components(A[members][:, members], directed=False)[0] == 1, c


def test_bad_arguments_fail_before_clustering_and_leave_outputs_untouched(dev):
    from infercnv_amd import _lib
    L = _lib.load()
    nn = knn_of(clones(40, seed=2)[0], 5)
    d_nn = torch.from_numpy(nn).cuda()
    memb = torch.full((40,), -7, dtype=torch.int32, device="cuda")
    ncl = np.full(1, -5, dtype=np.int32)

    def call(nn_t=d_nn, k=5, off=(0, 40), obj=1, res=(0.1,), beta=0.01, iters=2):
        o = np.asarray(off, dtype=np.int32)
        r = np.asarray(res, dtype=np.float64)
        tok = np.zeros(len(off) - 1, dtype=np.uint64)
        return L.icnv_leiden_dev(ct.c_void_p(nn_t.data_ptr()), k, o.ctypes.data_as(_lib._ip), len(off) - 1, obj,
                                 r.ctypes.data_as(_lib._dp), beta, iters, 0, tok.ctypes.data_as(ct.POINTER(ct.c_uint64)),
                                 ct.c_void_p(memb.data_ptr()), ncl.ctypes.data_as(_lib._ip), None)

    assert call(k=0) == _lib.ERR_ARG
    assert call(k=41) == _lib.ERR_ARG
    assert call(k=129, off=(0, 40)) in (_lib.ERR_ARG, _lib.ERR_UNSUPPORTED)
    assert call(off=(0, 30, 20)) == _lib.ERR_ARG
    assert call(obj=3) == _lib.ERR_ARG
    assert call(res=(float("nan"),)) == _lib.ERR_ARG and call(res=(-1.0,)) == _lib.ERR_ARG and call(res=(float("inf"),)) == _lib.ERR_ARG
    assert call(beta=0.0) == _lib.ERR_ARG and call(beta=float("inf")) == _lib.ERR_ARG
    assert call(iters=0) == _lib.ERR_ARG and call(iters=1001) == _lib.ERR_ARG
    for bad in (-1, 40, 2**31 - 1):
        b = nn.copy()
        b[17, 3] = bad
        assert call(nn_t=torch.from_numpy(b).cuda()) == _lib.ERR_ARG
        assert b"nn_idx" in L.icnv_last_error()
    assert (memb.cpu().numpy() == -7).all() and ncl[0] == -5
    assert call() == _lib.OK
    assert ncl[0] >= 1 and memb.cpu().numpy().min() == 1


def test_stats(dev):
    nn = knn_of(clones(300, seed=5)[0], 10)
    dev.leiden_stats(reset=True)
    m, K = run_gpu(dev, nn, "CPM", 0.05, 1e3, 2)
    st = dev.leiden_stats()
    ref = {"levels": 0, "move_visits": 0, "refine_visits": 0, "draws": 0}
    lr.leiden(nn, lr.CPM, 0.05, 1e3, 2, stats=ref)
    assert st["calls"] == 1 and st["problems"] == 1 and st["us"] > 0
    for key in ref:
        assert st[key] == ref[key], key
    assert dev.leiden_stats(reset=True)["calls"] == 1 and dev.leiden_stats()["calls"] == 0


# ------------------------------------------------------------------ the subclustering driver
def make_obj(seed=0):
    from infercnv_amd.infercnv_object import GeneOrder, InfercnvObject
    rng = np.random.default_rng(seed)
    G = 240
    chrs = np.repeat(["chr1", "chr2", "chr3", "chr4"], 60)
    groups = {"tumA": 70, "tumB": 45, "tiny": 2}
    refs = {"normal": 40}
    C = sum(groups.values()) + sum(refs.values())
    x = rng.normal(0.0, 0.15, size=(G, C))
    obs, ref, c0 = {}, {}, 0
    for name, n in groups.items():
        obs[name] = np.arange(c0, c0 + n)
        c0 += n
    for name, n in refs.items():
        ref[name] = np.arange(c0, c0 + n)
        c0 += n
    a = obs["tumA"]
    x[:60, a[:35]] += 0.8                     # two clones in tumA (chr1 gain in one half)
    x[120:180, a[35:]] -= 0.8                 # chr3 loss in the other
    x[60:120, obs["tumB"][::2]] += 0.7
    x[0:10, :] += rng.normal(0, 3.0, size=(10, C))   # noisy genes: the z-score filter takes them out
    return InfercnvObject(expr_data=x, gene_order=GeneOrder(chr=chrs), reference_grouped_cell_indices=ref,
                          observation_grouped_cell_indices=obs)


def restated_leiden_fn(seed):
    def fn(nn_idx, sizes, objective, gammas, tokens):
        return lr.leiden_batch(nn_idx.cpu().numpy(), sizes, OBJ[objective], gammas, 0.01, 2, seed, tokens)[0]
    return fn


def assert_same_result(a, b):
    (oa, pa), (ob, pb) = a, b
    ta, tb = oa.tumor_subclusters, ob.tumor_subclusters
    assert list(ta["subclusters"]) == list(tb["subclusters"])
    for g in ta["subclusters"]:
        assert list(ta["subclusters"][g]) == list(tb["subclusters"][g]), g
        for name in ta["subclusters"][g]:
            assert np.array_equal(ta["subclusters"][g][name], tb["subclusters"][g][name]), name
        ha, hb = ta["hc"][g], tb["hc"][g]
        ha, hb = (ha if isinstance(ha, list) else [ha]), (hb if isinstance(hb, list) else [hb])
        assert len(ha) == len(hb)
        for x, y in zip(ha, hb):
            assert (x is None) == (y is None)
            if x is not None:
                assert np.array_equal(x.merge, y.merge) and np.array_equal(x.order, y.order)
                assert np.array_equal(x.height.view(np.int64), y.height.view(np.int64))
    assert (pa is None) == (pb is None)
    if pa is not None:
        assert list(pa) == list(pb)
        for c in pa:
            assert list(pa[c]) == list(pb[c]), c
            for name in pa[c]:
                assert np.array_equal(pa[c][name], pb[c][name]), (c, name)


@pytest.mark.parametrize("cluster_by_groups", [True, False])
@pytest.mark.parametrize("refs_per_chr", [False, True])
def test_define_signif_tumor_subclusters_equals_restated_driver(dev, cluster_by_groups, refs_per_chr):
    from infercnv_amd import tumor_subclusters as ts
    obj = make_obj()
    kw = dict(k_nn=10, leiden_method="simple", cluster_by_groups=cluster_by_groups, per_chr_hmm_subclusters=True,
              per_chr_hmm_subclusters_references=refs_per_chr, seed=4)
    got = ts.define_signif_tumor_subclusters(obj, **kw)
    want = ts.define_signif_tumor_subclusters(obj, leiden_fn=restated_leiden_fn(4), **kw)
    assert_same_result(got, want)
    subs = got[0].tumor_subclusters["subclusters"]
    if cluster_by_groups:
        assert list(subs["tiny"]) == ["tiny_s1"] and got[0].tumor_subclusters["hc"]["tiny"] is None
    per_chr = got[1]
    assert list(per_chr) == ["chr1", "chr2", "chr3", "chr4"]
    if not refs_per_chr:
        assert all("normal" in per_chr[c] and np.array_equal(per_chr[c]["normal"], np.arange(117, 157)) for c in per_chr)
    # the Leiden branch splits tumA by its planted clones: every subcluster within one clone
    if cluster_by_groups:
        a = obj.observation_grouped_cell_indices["tumA"]
        for cells in subs["tumA"].values():
            assert np.all(cells < a[35]) or np.all(cells >= a[35])
        sizes = [len(v) for v in subs["tumA"].values()]
        assert sizes == sorted(sizes, reverse=True)


def test_golden_partition_none_reproduces_reference(dev, golden_dir):
    import oracle_c as oc
    import oracle_np as onp
    from infercnv_amd import tumor_subclusters as ts
    from infercnv_amd.infercnv_object import GeneOrder, InfercnvObject
    d = np.load(os.path.join(golden_dir, "infercnv_object_example.npz"))
    g = np.load(os.path.join(golden_dir, "hclust_example.npz"))
    log = onp.log2xplus1(onp.normalize_counts_by_seq_depth(d["count_data"]))
    x = torch.from_numpy(np.ascontiguousarray(log.T)).cuda()
    _, pre = dev.smooth_chain(x, oc.chr_starts_from_codes(d["chr_codes"]), [d["ref_normal"]], want_pre_denoise=True)
    pre = pre.cpu().numpy().T
    obj = InfercnvObject(expr_data=pre, gene_order=GeneOrder(chr=np.asarray(d["chr_levels"])[d["chr_codes"]]),
                         reference_grouped_cell_indices={"normal": d["ref_normal"]},
                         observation_grouped_cell_indices={"tumor": d["obs_tumor"]})
    out, per_chr = ts.define_signif_tumor_subclusters(obj, partition_method="none", z_score_filter=0)
    assert per_chr is None
    subs = out.tumor_subclusters["subclusters"]
    assert list(subs) == ["tumor", "normal"]
    assert list(subs["tumor"]) == ["tumor_s1"] and list(subs["normal"]) == ["normal_s1"]
    assert np.array_equal(subs["tumor"]["tumor_s1"], d["subcluster_0"])
    assert np.array_equal(subs["normal"]["normal_s1"], d["subcluster_1"])
    for grp in ("tumor", "normal"):
        hc = out.tumor_subclusters["hc"][grp]
        assert np.array_equal(hc.merge, g[f"{grp}_merge"]) and np.array_equal(hc.order, g[f"{grp}_order"])
        assert np.max(np.abs(hc.height - g[f"{grp}_height"]) / g[f"{grp}_height"]) <= 1e-12
    # the Leiden route on the same object: 10 cells per group <= k_nn = 20, one subcluster named after the group
    out2, _ = ts.define_signif_tumor_subclusters(obj, leiden_method="simple", z_score_filter=0)
    s2 = out2.tumor_subclusters["subclusters"]
    assert list(s2["tumor"]) == ["tumor"] and np.array_equal(s2["tumor"]["tumor"], d["obs_tumor"])
    assert np.array_equal(out2.tumor_subclusters["hc"]["tumor"].merge, g["tumor_merge"])
