"""The PCA route of the Leiden subclustering on the GPU (DESIGN K18; .leiden_seurat_preprocess_routine,
R/inferCNV_tumor_subclusters.R:699-723) under the library's own contract (include/icnv.h), held to the sequential
restatement of tests/leiden_pca_restate.py: bit for bit where the contract fixes the operation order (v_std, Z, the
projection, the SNN graph, the weighted Leiden), by derived bounds where it cannot (the Gram matrix, the eigenpairs)."""
import logging

import numpy as np
import pytest

import leiden_pca_restate as pr
import leiden_restate as lr
from test_leiden_pca_host import planted_obj

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

OBJ = {"CPM": lr.CPM, "modularity": lr.MODULARITY}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infercnv_amd import device
    torch.cuda.set_device(0)
    device.init(0)
    return device


def matrix(G, C, seed):
    """Positive values with a mean-variance trend; genes x cells."""
    rng = np.random.default_rng(seed)
    mu = rng.uniform(0.5, 3.0, size=G)
    sd = 0.05 * mu ** 0.7 * rng.uniform(0.7, 1.4, size=G)
    return mu[:, None] + sd[:, None] * rng.normal(size=(G, C))


def build_batch():
    """One batch of three problems of different n on one matrix: n = 70 over 37 genes (k = 8), n = 200 over 2100 genes
    (k = 20, the cut at 2000 features), n = 21 over 37 genes (k = 5).  Planted: a gene with one cell 30 trend-sd out at
    n = 70 (the sqrt(n) clip binds), a constant gene, a spike gene at n = 200 whose z exceeds 10, a centroid cell."""
    G, C = 2100, 291
    X = matrix(G, C, 5)
    cells = [np.arange(0, 70), np.arange(70, 270), np.arange(270, 291)]
    genes = [np.arange(100, 137), np.arange(G), np.arange(300, 337)]
    X[110, 70 + 3] += 30 * 0.05 * 3.0          # more than 30 sd of any gene of this generator: d > sqrt(70)
    X[105, :] = 1.25                            # constant over every cell
    X[50, 70 + 17] += 40.0                      # n = 200: z = (n - 1) / sqrt(n) = 14.07 > 10 for a single-cell spike
    X[:, 70 + 100] = X[:, 70:270].mean(axis=1)  # a centroid: a hub of the kNN graph
    return X, genes, cells, [8, 20, 5]


def build_edge_batch():
    """One batch on tile and block edges, nothing planted: n = 256 over 64 genes (k = 8), n = 257 over 65 genes (k = 8),
    n = 33 over 129 genes (k = 5) -- a Gram tile exactly and one row more, a projection block exactly and one cell more,
    an odd n shorter than two LDS stages under three tile rows."""
    X = matrix(200, 700, 21)
    cells = [np.arange(0, 256), np.arange(256, 513), np.arange(513, 546)]
    genes = [np.arange(0, 64), np.arange(64, 129), np.arange(71, 200)]
    return X, genes, cells, [8, 8, 5]


BUILDERS = {"planted": build_batch, "edge": build_edge_batch}
BATCHES = {}


def get_batch(name):
    """The GPU's stages and the restatement's, computed once and left unchanged."""
    if name not in BATCHES:
        from infercnv_amd import tumor_subclusters as ts
        X, genes, cells, ks = BUILDERS[name]()
        x = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()
        gpu = [ts.pca_stages(x, [genes[p]], [cells[p]], ks[p]) for p in range(3)]
        ref = [pr.stages(X, genes[p], cells[p], ks[p]) for p in range(3)]
        BATCHES[name] = dict(name=name, X=X, x=x, genes=genes, cells=cells, ks=ks, gpu=gpu, ref=ref)
    return BATCHES[name]


@pytest.fixture(scope="module", params=["planted", "edge"])
def batch(dev, request):
    """Either batch: the shape-generic assertions run on both, the planted values are asserted on theirs."""
    return get_batch(request.param)


@pytest.fixture(scope="module")
def planted(dev):
    """The batch of build_batch: the weighted Leiden and the CSR refusals are tied to it."""
    return get_batch("planted")


def test_vstd_and_features_identical(batch):
    for p in range(3):
        g, r = batch["gpu"][p], batch["ref"][p]
        assert g["active"] == [0] and not g["fallback"]
        assert np.array_equal(g["mean"][0], r["mean"]) and np.array_equal(g["var"][0], r["var"])
        assert np.array_equal(g["sd_e"][0], r["sd_e"])
        assert np.array_equal(g["v_std"][0], r["v_std"])
        assert np.array_equal(g["features"][0], r["features"])
    if batch["name"] != "planted":
        assert [r["features"].size for r in batch["ref"]] == [64, 65, 129]
        return
    r = batch["ref"][0]                         # n = 70: the clip binds on the planted gene, the constant gene is 0
    j = 110 - 100
    d = (batch["X"][110, 73] - r["mean"][j]) / r["sd_e"][j]
    assert d > 30 > np.sqrt(70.0)             # one cell 30 trend-sd out: the clip at sqrt(n) binds
    assert r["v_std"][105 - 100] == 0.0 and batch["gpu"][0]["v_std"][0][105 - 100] == 0.0
    assert batch["ref"][1]["features"].size == 2000 and batch["ref"][0]["features"].size == 37


def z_blocks(st):
    n, F = st["n_cells"][0], st["n_feat"][0]
    ldz = n + (n & 1)
    Z = st["Z"].cpu().numpy().reshape(F, ldz)
    return Z[:, :n], Z[:, n:]


def test_scaled_matrix_identical(batch):
    for p in range(3):
        Z, pad = z_blocks(batch["gpu"][p])
        assert np.array_equal(Z, batch["ref"][p]["Z"])
        assert not pad.any()
    if batch["name"] != "planted":
        return
    Z = batch["ref"][1]["Z"]
    f = int(np.flatnonzero(batch["ref"][1]["features"] == 50)[0])
    assert Z[f, 17] == 10.0 and Z.max() == 10.0             # the spike gene is clipped
    assert batch["ref"][0]["Z"].max() < 10.0               # n <= 101: |z| <= (n - 1) / sqrt(n) < 10


def test_gram_within_the_dot_product_bound_and_symmetric(batch):
    for p in range(3):
        st = batch["gpu"][p]
        F, n = st["n_feat"][0], st["n_cells"][0]
        M = st["M"].cpu().numpy().reshape(F, F)
        assert np.array_equal(M, M.T)
        Z, _ = z_blocks(st)
        u = 2.0 ** -53
        gamma = n * u / (1 - n * u)
        bound = gamma * (np.abs(Z) @ np.abs(Z).T)
        err = np.abs(M - Z @ Z.T)
        print(f"gram p={p}: max err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert np.all(err <= bound)


def test_eigenpairs_orthonormal_small_residual_and_signed(batch):
    for p in range(3):
        st = batch["gpu"][p]
        F, c = st["n_feat"][0], st["npcs"][0]
        assert c == min(10, F - 1, st["n_cells"][0] - 1)
        M = st["M"].cpu().numpy().reshape(F, F)
        V, lam = st["V"][0], st["eigenvalues"][0]
        assert V.shape == (F, c) and np.all(np.diff(lam) <= 0)
        assert np.max(np.abs(V.T @ V - np.eye(c))) <= 64 * F * 2.0 ** -53
        norm = np.linalg.norm(M, 2)

        def residual(lam, V):
            return max(np.linalg.norm(M @ V[:, j] - lam[j] * V[:, j]) for j in range(V.shape[1])) / norm

        w, vec = np.linalg.eigh(M)
        ref = residual(w[::-1][:c], vec[:, ::-1][:, :c])
        got = residual(lam, V)
        print(f"eigenpairs p={p}: residual {got:.3e}, numpy.linalg.eigh {ref:.3e}")
        assert got <= 16 * ref
        for j in range(c):
            assert V[int(np.argmax(np.abs(V[:, j]))), j] > 0


def test_projection_identical_given_the_gpus_eigenvectors(batch):
    for p in range(3):
        st = batch["gpu"][p]
        Z, _ = z_blocks(st)
        E = st["E"].cpu().numpy()
        c = st["npcs"][0]
        assert np.array_equal(E[:, :c], pr.project(Z, st["V"][0]))
        assert not E[:, c:].any()


def test_one_batch_of_three_problems_equals_the_single_calls(batch):
    """The three problems as ONE batch (one k for all, as a route has): every stage's block equals the single call's."""
    from infercnv_amd import tumor_subclusters as ts
    st = ts.pca_stages(batch["x"], batch["genes"], batch["cells"], 5)
    assert st["active"] == [0, 1, 2] and st["n_cells"] == [c.size for c in batch["cells"]]
    assert st["n_feat"] == [r["features"].size for r in batch["ref"]]
    if batch["name"] == "planted":
        assert st["n_cells"] == [70, 200, 21] and st["n_feat"] == [37, 2000, 37]
    z0 = m0 = r0 = 0
    Zb, Mb, Eb, nnb = st["Z"].cpu().numpy(), st["M"].cpu().numpy(), st["E"].cpu().numpy(), st["nn_idx"].cpu().numpy()
    got = csr_of(st)
    e0 = 0
    for p in range(3):
        one = batch["gpu"][p]
        F, n = one["n_feat"][0], one["n_cells"][0]
        assert np.array_equal(st["v_std"][p], one["v_std"][0]) and np.array_equal(st["features"][p], one["features"][0])
        assert np.array_equal(Zb[z0:z0 + one["Z"].numel()], one["Z"].cpu().numpy())
        assert np.array_equal(Mb[m0:m0 + F * F], one["M"].cpu().numpy())
        assert np.array_equal(Eb[r0:r0 + n], one["E"].cpu().numpy())
        nn = pr.knn(Eb[r0:r0 + n, :one["npcs"][0]], 5)
        assert np.array_equal(nnb[r0:r0 + n], nn)
        off, col, shared, weight, loop = pr.snn(nn)
        assert np.array_equal(got[0][r0:r0 + n + 1], off + e0)
        assert np.array_equal(got[1][e0:e0 + col.size], col) and np.array_equal(got[3][e0:e0 + col.size], weight)
        z0 += one["Z"].numel()
        m0 += F * F
        r0 += n
        e0 += col.size
    assert got[1].size == e0


def csr_of(st):
    return tuple(st[k].cpu().numpy() for k in ("row_off", "col", "shared", "weight", "loop"))


def test_snn_graph_identical_given_the_gpus_embedding(batch):
    for p in range(3):
        st = batch["gpu"][p]
        E = st["E"].cpu().numpy()[:, :st["npcs"][0]]
        nn = pr.knn(E, batch["ks"][p])
        assert np.array_equal(st["nn_idx"].cpu().numpy(), nn)
        for got, want in zip(csr_of(st), pr.snn(nn)):
            assert got.dtype == want.dtype and np.array_equal(got, want)
    off = batch["gpu"][1]["row_off"].cpu().numpy()
    if batch["name"] == "planted":
        assert np.diff(off)[100] > 64                   # the planted centroid's row is longer than a wavefront and than 2 k
    else:
        assert np.diff(off).max() > 64                  # so are rows of the edge batch, with nothing planted


def hub_block(n, k, seed):
    """A kNN block in which node 0 is in every row: row 0 of the SNN graph has n - 1 entries."""
    rng = np.random.default_rng(seed)
    nn = np.empty((n, k), dtype=np.int32)
    for i in range(n):
        others = rng.permutation(np.setdiff1d(np.arange(1, n), [i]))
        nn[i] = np.concatenate([[i, 0], others[:k - 2]]) if i else np.concatenate([[0], others[:k - 1]])
    return nn


@pytest.mark.parametrize("k", [5, 8, 9, 20])
def test_snn_prune_rule_hub_rows_and_a_batch(dev, k):
    """k = 8 keeps a shared count of 1 (16 = 2 k), k = 9 prunes it; a hub row longer than 64 and 2 k; three problems."""
    sizes = [70, 200, 21]
    nns = [hub_block(n, k, n + k) for n in sizes]
    t = torch.from_numpy(np.concatenate(nns)).cuda()
    got = [a.cpu().numpy() for a in dev.snn_jaccard(t, sizes)]
    r0, e0 = 0, 0
    ones = pairs_sharing_one = 0
    for n, nn in zip(sizes, nns):
        off, col, shared, weight, loop = pr.snn(nn)
        assert np.array_equal(got[0][r0:r0 + n + 1] - got[0][r0], off)
        assert got[0][r0] == e0
        for a, b in zip(got[1:4], (col, shared, weight)):
            assert np.array_equal(a[e0:e0 + col.size], b)
        assert np.array_equal(got[4][r0:r0 + n], loop)
        ones += int(np.count_nonzero(shared == 1))
        A = np.zeros((n, n), dtype=np.int64)
        A[np.repeat(np.arange(n), k), nn.ravel()] = 1
        S = A @ A.T
        np.fill_diagonal(S, 0)
        assert col.size == np.count_nonzero(16 * S >= 2 * k)
        assert np.all(S[0, 1:] >= 1)                    # node 0 shares itself with every row
        pairs_sharing_one += int(np.count_nonzero(S == 1))
        if n > 64 and k <= 8:
            assert off[1] - off[0] == n - 1 > max(64, 2 * k)
        r0 += n
        e0 += col.size
    assert got[1].size == e0
    assert pairs_sharing_one > 0 and (ones > 0) == (k <= 8)      # pairs with a shared count of 1 exist: kept iff 16 >= 2 k


GRAPH_CASES = [   # (problem, objective, gamma, beta, n_iterations)
    (0, "CPM", "auto", 0.01, 2), (0, "modularity", 1, 0.05, 5), (0, "CPM", 1, 1e3, 2), (0, "CPM", 0, 0.01, 2),
    (1, "CPM", "auto", 0.01, 2), (1, "modularity", 1, 1e3, 2), (1, "CPM", 0.02, 0.05, 1), (1, "modularity", 50, 0.01, 5),
    (2, "CPM", "auto", 0.01, 2), (2, "modularity", 1, 0.05, 5), (2, "CPM", 50, 0.05, 5),
]


@pytest.mark.parametrize("case", GRAPH_CASES, ids=lambda c: "-".join(map(str, c)))
def test_weighted_leiden_identical_to_restatement(dev, planted, case):
    p, obj, g, beta, iters = case
    st = planted["gpu"][p]
    n = st["n_cells"][0]
    gam = (11.98 / n) ** (1 / 1.165) if g == "auto" else float(g)
    gam = gam * pr.ONE if obj == "CPM" else gam
    memb, ncl = dev.leiden_graph(st["row_off"], st["col"], st["weight"], st["loop"], [n], obj, gam, beta, iters, 3, [11])
    off, col, _, weight, loop = csr_of(st)
    stats = {"levels": 0, "move_visits": 0, "refine_visits": 0, "draws": 0}
    want, K = pr.leiden_graph(off, col, weight, loop, OBJ[obj], gam, beta, iters, seed=3, token=11, stats=stats)
    assert int(ncl[0]) == K and np.array_equal(memb.cpu().numpy(), want)
    if case == (1, "CPM", "auto", 0.01, 2):
        assert stats["levels"] > 2 * iters              # some iteration of this graph takes at least two levels


def test_weighted_leiden_batch_equals_single_calls(dev, planted):
    sts = planted["gpu"]
    sizes = [st["n_cells"][0] for st in sts]
    offs = [st["row_off"] for st in sts]
    base = np.concatenate([[0], np.cumsum([int(o[-1].item()) for o in offs])])
    row_off = torch.cat([offs[0][:-1] + int(base[0]), offs[1][:-1] + int(base[1]), offs[2] + int(base[2])])
    col = torch.cat([st["col"] for st in sts])
    weight = torch.cat([st["weight"] for st in sts])
    loop = torch.cat([st["loop"] for st in sts])
    for obj, gam in (("CPM", 0.05 * pr.ONE), ("modularity", 1.0)):
        memb, ncl = dev.leiden_graph(row_off, col, weight, loop, sizes, obj, gam, 0.01, 2, 7, [1, 2, 3])
        memb = memb.cpu().numpy()
        r0 = 0
        for p, st in enumerate(sts):
            one, K = dev.leiden_graph(st["row_off"], st["col"], st["weight"], st["loop"], [sizes[p]], obj, gam, 0.01, 2, 7, [p + 1])
            assert int(K[0]) == int(ncl[p]) and np.array_equal(one.cpu().numpy(), memb[r0:r0 + sizes[p]])
            r0 += sizes[p]


def test_leiden_graph_refuses_a_bad_csr(dev, planted):
    from infercnv_amd import IcnvError, _lib
    st = planted["gpu"][2]
    n = st["n_cells"][0]
    for name, change in (("col", lambda t: t.index_fill(0, torch.tensor([0]).cuda(), n)),
                         ("weight", lambda t: t.index_fill(0, torch.tensor([1]).cuda(), 0)),
                         ("loop", lambda t: t.index_fill(0, torch.tensor([2]).cuda(), 2))):
        args = {k: st[k] for k in ("row_off", "col", "weight", "loop")}
        args[name] = change(args[name].clone())
        with pytest.raises(IcnvError) as e:
            dev.leiden_graph(args["row_off"], args["col"], args["weight"], args["loop"], [n], "CPM", 1.0)
        assert e.value.code == _lib.ERR_ARG
    with pytest.raises(IcnvError) as e:   # a total edge weight of 2^53 and more is refused
        dev.leiden_graph(st["row_off"], st["col"], torch.full_like(st["weight"], 1 << 50), st["loop"], [n], "CPM", 1.0)
    assert e.value.code == _lib.ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------- end to end
def test_default_call_recovers_planted_clones(dev):
    """define_signif_tumor_subclusters(obj) with no further arguments: R's defaults, leiden_method = "PCA",
    leiden_resolution = "auto" (0.0893 at n = 200).  test_leiden_pca_host.py asserts that the restatement alone recovers the
    clones from these inputs."""
    from infercnv_amd import tumor_subclusters as ts
    obj, lab = planted_obj()
    out, per_chr = ts.define_signif_tumor_subclusters(obj)
    assert per_chr is None
    subs = out.tumor_subclusters["subclusters"]["tumor"]
    assert len(subs) == 4 and sorted(c.size for c in subs.values()) == [50] * 4
    for name, members in subs.items():
        assert np.unique(lab[members]).size == 1, name
    want = pr.routine(obj.expr_data, np.arange(60), np.arange(200), 20, ts.auto_leiden_resolution(200), lr.CPM, 0.01, 2, seed=0,
                      token=ts.fnv1a64("tumor"))
    for i in range(1, 5):
        assert np.array_equal(np.sort(subs[f"tumor_s{i}"]), np.flatnonzero(want == i))


def test_per_chromosome_route_equals_the_restatement(dev):
    from infercnv_amd import GeneOrder, InfercnvObject
    from infercnv_amd import tumor_subclusters as ts
    X = matrix(37 + 48 + 60, 110, 9)
    chrs = np.array(["chr1"] * 37 + ["chr2"] * 48 + ["chr3"] * 60)
    rng = np.random.default_rng(10)
    for c0, c1 in ((0, 37), (37, 85), (85, 145)):          # two clones per chromosome, in a few genes of it
        half = rng.permutation(70) < 35
        X[c0:c0 + 4][:, :70][:, half] += 0.8
    obj = InfercnvObject(expr_data=X, gene_order=GeneOrder(chr=chrs),
                         observation_grouped_cell_indices={"a": np.arange(70), "b": np.arange(70, 110)})
    _, per_chr = ts.define_signif_tumor_subclusters(obj, k_nn=8, leiden_method="simple", per_chr_hmm_subclusters=True,
                                                    leiden_method_per_chr="PCA")
    for c, (c0, c1) in zip(("chr1", "chr2", "chr3"), ((0, 37), (37, 85), (85, 145))):
        for g, cells in (("a", np.arange(70)), ("b", np.arange(70, 110))):
            want = pr.routine(X, np.arange(c0, c1), cells, 8, 1.0, lr.MODULARITY, 0.01, 2, seed=0, token=ts.fnv1a64(f"{c}\0{g}"))
            names = [k for k in per_chr[c] if k.startswith(g + "_s")]
            assert len(names) == want.max()
            for i in range(1, want.max() + 1):
                assert np.array_equal(per_chr[c][f"{g}_s{i}"], cells[want == i]), (c, g, i)


def test_nine_genes_fall_back_to_the_simple_route(dev, caplog):
    from infercnv_amd import GeneOrder, InfercnvObject
    from infercnv_amd import tumor_subclusters as ts
    X = matrix(9, 40, 11)
    X[:3, :20] += 0.5
    obj = InfercnvObject(expr_data=X, gene_order=GeneOrder(chr=np.array(["chr1"] * 9)),
                         observation_grouped_cell_indices={"a": np.arange(40)})
    with caplog.at_level(logging.INFO, logger="infercnv_amd"):
        got = ts.leiden_seurat_preprocess_routine(obj, np.arange(40), 5, 0.1, "CPM", seed=2, token=7)
    want = ts.leiden_simple_snn(obj, np.arange(40), 5, 0.1, "CPM", seed=2, token=7)
    assert np.array_equal(got, want)
    assert np.array_equal(got, pr.routine(X, np.arange(9), np.arange(40), 5, 0.1, lr.CPM, seed=2, token=7))
    lines = [r.getMessage() for r in caplog.records if "Falling back to simple Leiden clustering" in r.getMessage()]
    assert len(lines) == 1
