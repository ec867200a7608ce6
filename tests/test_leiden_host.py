"""CPU tests of the Leiden contract (DESIGN K11): the sequential restatement of tests/leiden_restate.py on graphs whose
answer is known, its streams against NumPy, the driver's naming / ordering / skip rules and its "none" branch, and the
C ABI's argument validation (every check runs before any device work) and export."""
import ctypes as ct
import os

import numpy as np
import pytest

import leiden_restate as lr
from infercnv_amd import GeneOrder, InfercnvObject, _lib, tumor_subclusters as ts


def cliques_nn(sizes):
    """kNN blocks of disjoint cliques: row i lists every member of its clique, itself first (k = min size)."""
    k = min(sizes)
    rows, c0 = [], 0
    for n in sizes:
        for i in range(n):
            rows.append([c0 + (i + j) % n for j in range(k)])
        c0 += n
    return np.array(rows, dtype=np.int32)


def paths_nn(lengths):
    """Disjoint paths: row i = [i, next] (the last node of a path points back)."""
    rows, c0 = [], 0
    for n in lengths:
        for i in range(n):
            rows.append([c0 + i, c0 + (i + 1 if i + 1 < n else i - 1)])
        c0 += n
    return np.array(rows, dtype=np.int32)


def components(nn):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    n, k = nn.shape
    A = csr_matrix((np.ones(n * k), (np.repeat(np.arange(n), k), nn.ravel())), shape=(n, n))
    return connected_components(A, directed=False)[1], A.maximum(A.T).tocsr()


@pytest.mark.parametrize("objective", [lr.CPM, lr.MODULARITY])
def test_disjoint_cliques_and_paths_give_their_components(objective):
    for nn in (cliques_nn([5, 7, 6, 9]), paths_nn([4, 6, 5])):
        comp, _ = components(nn)
        gamma = 0.05                         # low enough that a whole component is the optimum of either objective
        memb, K = lr.leiden(nn, objective, gamma, 0.01, 2, seed=1, token=2)
        assert K == comp.max() + 1
        for c in range(1, K + 1):          # each community is exactly one component
            assert np.unique(comp[memb == c]).size == 1
        assert np.unique(memb[np.unique(comp, return_index=True)[1]]).size == K


def planted(n_blocks=4, per=60, p_in=0.3, p_out=0.01, seed=0):
    """A planted-partition graph as a (n, k) kNN block: each node's k draws from its block (p_in) or outside."""
    rng = np.random.default_rng(seed)
    n = n_blocks * per
    lab = np.repeat(np.arange(n_blocks), per)
    k = 8
    nn = np.empty((n, k), dtype=np.int32)
    for i in range(n):
        nn[i, 0] = i
        for j in range(1, k):
            same = rng.random() < p_in / (p_in + p_out)
            pool = np.flatnonzero((lab == lab[i]) == same)
            nn[i, j] = rng.choice(pool)
    return nn, lab


def modularity(A, memb):
    A = A.tocsr()
    deg = np.asarray(A.sum(axis=1)).ravel()
    m2 = deg.sum()
    q = 0.0
    for c in np.unique(memb):
        idx = np.flatnonzero(memb == c)
        q += A[idx][:, idx].sum() / m2 - (deg[idx].sum() / m2) ** 2
    return q


def test_communities_are_connected_and_modularity_matches_louvain():
    nx = pytest.importorskip("networkx")
    for seed in range(3):
        nn, _ = planted(seed=seed)
        comp, A = components(nn)
        A.setdiag(0)
        A.eliminate_zeros()
        memb, K = lr.leiden(nn, lr.MODULARITY, 1.0, 0.01, 2, seed=seed)
        from scipy.sparse.csgraph import connected_components
        for c in range(1, K + 1):
            idx = np.flatnonzero(memb == c)
            assert connected_components(A[idx][:, idx], directed=False)[0] == 1
        G = nx.from_scipy_sparse_array(A)
        louv = nx.community.louvain_communities(G, seed=0)
        lm = np.empty(A.shape[0], dtype=np.int64)
        for c, members in enumerate(louv):
            lm[list(members)] = c
        assert modularity(A, memb) >= modularity(A, lm) - 1e-3


def test_streams_equal_numpy():
    from infercnv_amd import tumor_subclusters as _  # noqa: F401  (the package imports)
    bg = np.random.Philox(key=np.array([5, 77], dtype=np.uint64), counter=np.array([0, 2, (3 << 32) | 4, 9], dtype=np.uint64))
    want = np.random.Generator(bg).permutation(1000)
    assert np.array_equal(lr.generator(5, 77, 2, 3, 4, 9).permutation(1000), want)
    # the draws: Generator.random() is (next_uint64 >> 11) * 2^-53 of the raw Philox words
    g = lr.generator(5, 77, 3, 0, 1, 2)
    raw = np.random.Philox(key=np.array([5, 77], dtype=np.uint64), counter=np.array([0, 3, 1, 2], dtype=np.uint64))
    words = raw.random_raw(16)
    got = np.array([g.random() for _ in range(16)])
    assert np.array_equal(got, (words >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0))


def test_exp_lib_is_close_to_exp_and_overflows_at_its_threshold():
    x = np.concatenate([np.linspace(0, 50, 1001), np.linspace(700, 709, 101)])
    got = np.array([lr.exp_lib(v) for v in x])
    assert np.max(np.abs(got / np.exp(x) - 1)) < 1e-14
    assert lr.exp_lib(0.0) == 1.0
    assert lr.exp_lib(709.0) < np.inf and lr.exp_lib(709.0000001) == np.inf and lr.exp_lib(np.inf) == np.inf


def test_auto_resolution():
    assert ts.auto_leiden_resolution(2000) == (11.98 / 2000) ** (1 / 1.165)
    assert ts.auto_leiden_resolution(12) == pytest.approx(0.998, rel=1e-2)


def make_obj(sizes, refs=0, G=30, seed=0):
    rng = np.random.default_rng(seed)
    C = sum(sizes.values()) + refs
    x = rng.normal(size=(G, C))
    obs, c0 = {}, 0
    for g, n in sizes.items():
        obs[g] = np.arange(c0, c0 + n)
        c0 += n
    ref = {"normal": np.arange(c0, c0 + refs)} if refs else {}
    return InfercnvObject(expr_data=x, gene_order=GeneOrder(chr=np.repeat(["chr1", "chr2", "chr3"], G // 3)),
                          reference_grouped_cell_indices=ref, observation_grouped_cell_indices=obs)


def fake_leiden(labels):
    """A leiden_fn returning fixed labels per problem (the driver's naming and ordering, without a GPU)."""
    def fn(nn_idx, sizes, objective, gammas, tokens):
        fn.calls.append((list(sizes), objective, list(gammas), list(tokens)))
        return np.concatenate([labels[n] for n in sizes])
    fn.calls = []
    return fn


def test_driver_rejects_what_it_does_not_implement():
    obj = make_obj({"a": 30}, refs=10)
    with pytest.raises(NotImplementedError, match="restrict_to_DE_genes"):
        ts.define_signif_tumor_subclusters(obj, leiden_method="simple", restrict_to_DE_genes=True)
    for pm in ("qnorm", "pheight", "qgamma"):
        with pytest.raises(NotImplementedError, match=pm):
            ts.define_signif_tumor_subclusters(obj, partition_method=pm)
    with pytest.raises(ValueError):
        ts.define_signif_tumor_subclusters(obj, partition_method="shc")
    flat = make_obj({"a": 30}, refs=10)
    flat.expr_data[:, :] = 1.0
    flat.expr_data[:, 30:] += np.tile([0.1, -0.1], 5)
    with pytest.raises(ValueError, match="keeps no gene"):
        ts.define_signif_tumor_subclusters(flat, leiden_method="simple", partition_method="none")


def test_driver_naming_ordering_and_skip_rules(monkeypatch):
    """Main route: decreasing size, ties by label (:604); per chromosome: ascending label (:687); < 3 cells: "<g>_s1";
    k_nn >= n: one subcluster "<g>"; references appended per chromosome (:145-149)."""
    import torch
    obj = make_obj({"big": 9, "small": 2, "mid": 5}, refs=4)
    monkeypatch.setattr(ts, "_to_device", lambda o: None)
    monkeypatch.setattr(ts.device, "knn", lambda x, problems, k: (torch.zeros((sum(c.size for _, c in problems), k), dtype=torch.int32), None))
    trees = []

    def hclust_cells(x, problems, method):
        trees.extend(c.tolist() for _, c in problems)
        return [(torch.zeros((c.size - 1, 2), dtype=torch.int32), torch.zeros(c.size - 1, dtype=torch.float64),
                 torch.arange(1, c.size + 1, dtype=torch.int32)) for _, c in problems]
    monkeypatch.setattr(ts.device, "hclust_cells", hclust_cells)
    part = np.array([3, 1, 3, 2, 1, 2, 4, 2, 1], dtype=np.int32)    # sizes: 1 -> 3, 2 -> 3, 3 -> 2, 4 -> 1
    fn = fake_leiden({9: part})
    out, per_chr = ts.define_signif_tumor_subclusters(obj, k_nn=5, leiden_method="simple", z_score_filter=0,
                                                      per_chr_hmm_subclusters=True, leiden_fn=fn)
    subs, hc = out.tumor_subclusters["subclusters"], out.tumor_subclusters["hc"]
    assert list(subs) == ["big", "small", "mid", "normal"]
    assert list(subs["big"]) == ["big_s1", "big_s2", "big_s3", "big_s4"]
    assert subs["big"]["big_s1"].tolist() == [1, 4, 8] and subs["big"]["big_s4"].tolist() == [6]
    assert list(subs["small"]) == ["small_s1"] and hc["small"] is None
    assert list(subs["mid"]) == ["mid"] and subs["mid"]["mid"].tolist() == [11, 12, 13, 14, 15]
    assert isinstance(hc["big"], list) and len(hc["big"]) == 3            # partitions of >= 2 cells, in subcluster order
    assert [t for t in trees if t[0] < 9] == [[1, 4, 8], [3, 5, 7], [0, 2]] and [11, 12, 13, 14, 15] in trees
    first = fn.calls[0]
    assert first[0] == [9] and first[1] == "CPM" and first[2] == [ts.auto_leiden_resolution(9)]
    assert first[3] == [ts.fnv1a64("big")]
    # per chromosome: obs groups only, ascending labels, the references appended
    chr_call = fn.calls[1]
    assert chr_call[1] == "modularity" and chr_call[2] == [1.0] * 3
    assert chr_call[3] == [ts.fnv1a64(f"chr{i}\0big") for i in (1, 2, 3)]
    assert list(per_chr) == ["chr1", "chr2", "chr3"]
    assert list(per_chr["chr1"]) == ["big_s1", "big_s2", "big_s3", "big_s4", "small", "mid", "normal"]
    assert per_chr["chr2"]["normal"].tolist() == [16, 17, 18, 19]


def test_driver_absent_chromosome_gets_every_cell(monkeypatch):
    import torch
    obj = make_obj({"a": 8}, refs=0, G=30)
    obj.gene_order = GeneOrder(chr=np.array(["chr1"] * 20 + ["chr2"] * 10))
    monkeypatch.setattr(ts, "_to_device", lambda o: None)
    monkeypatch.setattr(ts.device, "knn", lambda x, problems, k: (torch.zeros((sum(c.size for _, c in problems), k), dtype=torch.int32), None))
    monkeypatch.setattr(ts.device, "hclust_cells", lambda x, problems, m: [
        (torch.zeros((c.size - 1, 2), dtype=torch.int32), torch.zeros(c.size - 1, dtype=torch.float64),
         torch.arange(1, c.size + 1, dtype=torch.int32)) for _, c in problems])
    monkeypatch.setattr(ts, "zscore_kept_genes", lambda o, z: np.arange(20))   # chr2 filtered away entirely
    fn = fake_leiden({8: np.array([2, 1, 2, 1, 1, 2, 2, 2], dtype=np.int32)})
    _, per_chr = ts.define_signif_tumor_subclusters(obj, k_nn=3, leiden_method="simple", per_chr_hmm_subclusters=True,
                                                    leiden_fn=fn)
    assert list(per_chr["chr1"]) == ["a_s1", "a_s2"]
    assert list(per_chr["chr2"]) == ["a"] and per_chr["chr2"]["a"].tolist() == list(range(8))


def test_driver_pca_is_refused_when_a_group_needs_it(monkeypatch):
    import torch
    obj = make_obj({"a": 30})
    monkeypatch.setattr(ts, "_to_device", lambda o: None)
    monkeypatch.setattr(ts.device, "knn", lambda *a: (torch.zeros((30, 20), dtype=torch.int32), None))
    with pytest.raises(NotImplementedError, match="PCA"):
        ts.define_signif_tumor_subclusters(obj)       # R's default leiden_method is "PCA"


def test_partition_none_branch(monkeypatch):
    import torch
    obj = make_obj({"a": 5, "b": 2}, refs=3)
    monkeypatch.setattr(ts, "_to_device", lambda o: None)
    monkeypatch.setattr(ts.device, "hclust_cells", lambda x, problems, m: [
        (torch.zeros((c.size - 1, 2), dtype=torch.int32), torch.zeros(c.size - 1, dtype=torch.float64),
         torch.arange(c.size, 0, -1, dtype=torch.int32)) for _, c in problems])
    out, per_chr = ts.define_signif_tumor_subclusters(obj, partition_method="none", z_score_filter=0)
    subs = out.tumor_subclusters["subclusters"]
    assert per_chr is None
    assert subs["a"] == {"a_s1": subs["a"]["a_s1"]} and subs["a"]["a_s1"].tolist() == [4, 3, 2, 1, 0]   # hc$order
    assert subs["b"]["b_s1"].tolist() == [5, 6] and out.tumor_subclusters["hc"]["b"] is None
    assert subs["normal"]["normal_s1"].tolist() == [9, 8, 7]


def _host_call(L, nn, k, off, obj=1, res=None, beta=0.01, iters=2):
    nn = np.ascontiguousarray(nn, dtype=np.int32)
    o = np.asarray(off, dtype=np.int32)
    P = len(off) - 1
    r = np.full(P, 0.1) if res is None else np.asarray(res, dtype=np.float64)
    memb = np.full(max(int(o[-1]), 1), -3, dtype=np.int32)
    ncl = np.full(max(P, 1), -4, dtype=np.int32)
    rc = L.icnv_leiden(nn.ctypes.data_as(ct.c_void_p), k, o.ctypes.data_as(_lib._ip), P, obj, r.ctypes.data_as(_lib._dp), beta,
                       iters, 0, None, memb.ctypes.data_as(ct.c_void_p), ncl.ctypes.data_as(_lib._ip))
    assert (memb == -3).all() and (ncl == -4).all()       # untouched on error
    return rc


def test_leiden_argument_validation_needs_no_gpu():
    L = _lib.load()
    nn = cliques_nn([5, 5])
    assert _host_call(L, nn, 0, [0, 10]) == _lib.ERR_ARG
    assert _host_call(L, nn, 11, [0, 10]) == _lib.ERR_ARG
    assert _host_call(L, nn, 5, [0, 6, 4]) == _lib.ERR_ARG             # offsets not monotone
    assert _host_call(L, nn, 5, [1, 10]) == _lib.ERR_ARG
    assert _host_call(L, nn, 5, [0, 10], obj=0) == _lib.ERR_ARG
    assert _host_call(L, nn, 5, [0, 10], res=[float("nan")]) == _lib.ERR_ARG
    assert _host_call(L, nn, 5, [0, 10], res=[-0.5]) == _lib.ERR_ARG
    assert _host_call(L, nn, 5, [0, 10], beta=0.0) == _lib.ERR_ARG
    assert _host_call(L, nn, 5, [0, 10], beta=float("nan")) == _lib.ERR_ARG
    assert _host_call(L, nn, 5, [0, 10], iters=0) == _lib.ERR_ARG
    assert _host_call(L, nn, 5, [0, 10], iters=1001) == _lib.ERR_ARG
    big = np.zeros((200, 129), dtype=np.int32)
    assert _host_call(L, big, 129, [0, 200]) == _lib.ERR_UNSUPPORTED
    assert b"128" in L.icnv_last_error()


def test_leiden_entry_points_are_declared_bound_and_exported():
    L = _lib.load()
    names = ("icnv_leiden", "icnv_leiden_dev", "icnv_snn_graph_dev", "icnv_leiden_stats", "icnv_leiden_stats_reset")
    for name in names:
        assert name in _lib.PROTOTYPES and hasattr(L, name)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "icnv.h")).read()
    for name in names:
        assert name + "(" in header
    assert "#define ICNV_LEIDEN_CPM 1" in header and "#define ICNV_LEIDEN_MODULARITY 2" in header
