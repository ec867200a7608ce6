"""The Bayesian filter of the predicted CNV regions on the GPU (icnv_bayes_loglik_dev / icnv_bayes_sample_dev, DESIGN K13):
every log-likelihood, every likelihood ratio, every kept theta sample, every chain sum and every state count bit-equal to
the sequential restatement of tests/bayes_restate.py; then steps 18-19 end to end on objects with planted truth."""
import os

import numpy as np
import pytest

import bayes_restate as br

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MU6 = np.array([0.1, 0.5, 1.0, 1.5, 2.0, 3.0])
TAU6 = 1.0 / np.array([0.2, 0.25, 0.3, 0.3, 0.35, 0.4]) ** 2
MU3 = np.array([0.8, 1.0, 1.2])
TAU3 = np.full(3, 1.0 / 0.3 ** 2)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infercnv_amd import device
    torch.cuda.set_device(0)
    device.init(0)
    return device


def same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    both_nan = np.isnan(a) & np.isnan(b)
    bad = ~both_nan & (a.view(np.uint64) != b.view(np.uint64))
    assert not bad.any(), f"{int(bad.sum())} differ, first at {np.argwhere(bad)[0]}: {a[bad][0]!r} vs {b[bad][0]!r}"


def on_dev(expr):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(expr, dtype=np.float64).T)).cuda()


def gpu_run(dev, x, regions, names, mu, tau, sched, seed):
    ll, L, off = dev.bayes_loglik(x, regions, mu, tau)
    ts, smp, fr = dev.bayes_sample(L, off, [br.fnv1a64(n) for n in names], *sched, seed=seed, want_samples=True)
    return ll.cpu().numpy(), L.cpu().numpy(), off, ts.cpu().numpy(), smp.cpu().numpy(), fr.cpu().numpy()


def check(dev, expr, regions, names, mu, tau, sched=(3, 2, 6), seed=0):
    ll, L, off, ts, smp, fr = gpu_run(dev, on_dev(expr), regions, names, mu, tau, sched, seed)
    rll, rL = br.loglik(expr, [(range(g0, g0 + ng), cells) for g0, ng, cells in regions], mu, tau)
    same(ll, rll)
    same(L, rL)
    rts, rsmp, rfr = br.sample(rL, off, [br.fnv1a64(n) for n in names], len(mu), *sched, seed=seed)
    same(ts, rts)
    same(smp, rsmp)
    assert np.array_equal(fr, rfr)
    assert (fr.sum(axis=1) == len(mu) * sched[2]).all()
    return L, fr


@pytest.mark.parametrize("K", [6, 3])
def test_fixture_regions(dev, golden_dir, K):
    """The nine regions of the reference's stored run (data/mcmc_obj.rda @cell_gene) on its example object."""
    cg = np.load(os.path.join(golden_dir, "mcmc_cell_gene.npz"))
    expr = np.load(os.path.join(golden_dir, "infercnv_object_example.npz"))["expr_data"]
    hs = np.load(os.path.join(golden_dir, "hmm_states_example.npz"))
    mu, tau = (hs["mu"], hs["sig"]) if K == 6 else (hs["mu"][[1, 2, 4]], np.full(3, hs["sig"][2]))
    regions, names = [], []
    for i, name in enumerate(cg["names"]):
        genes = cg[f"genes_{i}"].astype(np.int64) - 1
        assert np.all(np.diff(genes) == 1)
        regions.append((int(genes[0]), int(genes.size), cg[f"cells_{i}"].astype(np.int32) - 1))
        names.append(str(name))
    check(dev, expr, regions, names, mu, tau, sched=(5, 3, 12), seed=7)


def ragged_case(K, seed):
    """1 and 2 cells, 1 gene, an empty region, a group beyond the LDS-resident limit with near-equal likelihoods (every cell
    undecided), 64 / 65 cells, and decisive regions."""
    rng = np.random.default_rng(seed)
    mu, tau = (MU6, TAU6) if K == 6 else (MU3, TAU3)
    G, C = 300, 900
    expr = rng.normal(1.0, 0.05, size=(G, C))
    expr[100:200, :300] = rng.normal(6.0, 0.3, size=(100, 300))             # decisive: every other state's L underflows to 0
    expr[200:260, 300:400] = rng.normal(7.0, 0.2, size=(60, 100))
    cells = rng.permutation(C).astype(np.int32)
    regions = [(0, 3, cells[:1]), (5, 2, cells[1:3]), (17, 1, cells[3:40]), (20, 4, np.zeros(0, dtype=np.int32)),
               (30, 2, np.sort(cells[:700])), (40, 1, cells[100:164]), (41, 2, cells[200:265]),
               (100, 100, np.arange(300, dtype=np.int32)), (200, 60, np.arange(250, 420, dtype=np.int32)),
               (90, 120, np.arange(0, 600, 2, dtype=np.int32))]
    return expr, regions, [f"chr{i}-region_{i + 1}" for i in range(len(regions))], mu, tau


@pytest.mark.parametrize("K", [6, 3])
def test_ragged_batch(dev, K):
    expr, regions, names, mu, tau = ragged_case(K, K)
    dev.bayes_stats(reset=True)
    L, fr = check(dev, expr, regions, names, mu, tau, sched=(3, 2, 6), seed=K)
    st = dev.bayes_stats()
    assert st["regions_streamed"] >= 1 and st["regions_lds"] >= 1          # both residency classes ran
    und = ((L > 0).sum(axis=1) > 1).sum()
    assert st["undecided_rows"] == und and 0 < und < L.shape[0]            # near-equal and decisive cells both present
    assert (np.isin(fr, (0, K * 6)).all(axis=1)).sum() >= L.shape[0] - und


def test_thousand_regions(dev):
    rng = np.random.default_rng(11)
    G, C, R = 64, 40, 1024
    expr = rng.normal(1.0, 0.1, size=(G, C))
    regions, names = [], []
    for r in range(R):
        ng = int(rng.integers(1, 4))
        g0 = int(rng.integers(0, G - ng + 1))
        regions.append((g0, ng, rng.choice(C, size=int(rng.integers(0, 4)), replace=False).astype(np.int32)))
        names.append(f"chr{r % 22 + 1}-region_{r + 1}")
    check(dev, expr, regions, names, MU3, TAU3, sched=(1, 1, 2), seed=3)


def test_default_schedule(dev):
    """500 + 200 discarded and 1 000 kept iterations, once: 7 ambiguous cells, i3."""
    rng = np.random.default_rng(5)
    expr = rng.normal(1.0, 0.15, size=(6, 7))
    L, fr = check(dev, expr, [(1, 4, np.arange(7, dtype=np.int32))], ["chr1-region_1"], MU3, TAU3, sched=(500, 200, 1000), seed=1)
    assert ((L > 0).sum(axis=1) == 3).all()


def test_decided_shortcut_on_off(dev, monkeypatch):
    expr, regions, names, mu, tau = ragged_case(6, 21)
    x = on_dev(expr)
    dev.bayes_stats(reset=True)
    on = gpu_run(dev, x, regions, names, mu, tau, (4, 3, 9), 5)
    und_on = dev.bayes_stats(reset=True)["undecided_rows"]
    monkeypatch.setenv("ICNV_BAYES_DECIDED", "0")
    off = gpu_run(dev, x, regions, names, mu, tau, (4, 3, 9), 5)
    st = dev.bayes_stats(reset=True)
    monkeypatch.delenv("ICNV_BAYES_DECIDED")
    assert st["undecided_rows"] == st["rows"] > und_on > 0
    for a, b in zip(on[3:5], off[3:5]):
        same(a, b)
    assert np.array_equal(on[5], off[5])


def test_permuted_regions_and_repeat(dev):
    expr, regions, names, mu, tau = ragged_case(3, 31)
    x = on_dev(expr)
    a = gpu_run(dev, x, regions, names, mu, tau, (3, 2, 6), 9)
    b = gpu_run(dev, x, regions, names, mu, tau, (3, 2, 6), 9)
    for u, v in zip(a[:2] + a[3:5], b[:2] + b[3:5]):
        same(u, v)
    assert np.array_equal(a[5], b[5])
    perm = np.random.default_rng(2).permutation(len(regions))
    p = gpu_run(dev, x, [regions[i] for i in perm], [names[i] for i in perm], mu, tau, (3, 2, 6), 9)
    for j, i in enumerate(perm):
        same(p[3][j], a[3][i])
        same(p[4][j], a[4][i])
        ra, rp = slice(a[2][i], a[2][i + 1]), slice(p[2][j], p[2][j + 1])
        same(p[0][rp], a[0][ra])
        same(p[1][rp], a[1][ra])
        assert np.array_equal(p[5][rp], a[5][ra])


# ---- steps 18-19 end to end -------------------------------------------------------------------------------------------
def planted_object(seed=0, half_normal=False):
    """3 chromosomes x 100 genes, 20 reference and 200 tumour cells.  The HMM calls: A, chr1 genes 10-59, a gain (state 5)
    whose data sit at the neutral mean (with half_normal: only for the first 100 tumour cells, the others at state 5's mean);
    B, chr2 genes 20-79, state 4 with the data at state 5's mean; C, chr3 genes 30-89, state 2 with data at state 2's mean."""
    from infercnv_amd.infercnv_object import GeneOrder, InfercnvObject
    rng = np.random.default_rng(seed)
    G, C = 300, 220
    tum = np.arange(20, 220)
    expr = rng.normal(MU6[2], 0.3, size=(G, C))
    states = np.full((G, C), 3, dtype=np.int8)
    states[10:60, 20:] = 5
    if half_normal:
        expr[10:60, 120:] = rng.normal(MU6[4], 0.3, size=(50, 100))
    states[120:180, 20:] = 4
    expr[120:180, 20:] = rng.normal(MU6[4], 0.3, size=(60, 200))
    states[230:290, 20:] = 2
    expr[230:290, 20:] = rng.normal(MU6[1], 0.25, size=(60, 200))
    chrs = np.repeat(np.array(["chr1", "chr2", "chr3"]), 100)
    pos = np.tile(np.arange(100) * 1000 + 1, 3)
    obj = InfercnvObject(expr_data=expr, gene_order=GeneOrder(chr=chrs, start=pos, stop=pos + 500),
                         reference_grouped_cell_indices={"normal": np.arange(20)},
                         observation_grouped_cell_indices={"tumor": tum},
                         gene_names=np.array([f"g{i}" for i in range(G)]), cell_names=np.array([f"c{i}" for i in range(C)]))
    return obj, states, tum


def restated_means(expr, cell_gene, sched, seed):
    regions = [(range(int(cg["Genes"][0]), int(cg["Genes"][-1]) + 1), cg["Cells"]) for cg in cell_gene]
    _, rL = br.loglik(expr, regions, MU6, TAU6)
    off = np.concatenate([[0], np.cumsum([len(c) for _, c in regions])])
    ts, _, fr = br.sample(rL, off, [br.fnv1a64(cg["cnv_regions"]) for cg in cell_gene], 6, *sched, seed=seed)
    return br.theta_mean(ts, sched[2]).T, [(fr[off[r]:off[r + 1]] / (6.0 * sched[2])).T for r in range(len(regions))]


def test_filter_removes_reassigns_keeps(dev, tmp_path):
    from infercnv_amd import bayes_net, cnv_regions
    from infercnv_amd.infercnv_object import InfercnvObject
    obj, states, tum = planted_object()
    sched = (10, 5, 30)
    st_obj = obj.copy()
    st_obj.expr_data = states.astype(np.float64)
    cnv_regions.generate_cnv_region_reports(st_obj, "17_HMM_pred", str(tmp_path), ignore_neutral_state=3, by="consensus")
    m = bayes_net.inferCNVBayesNet(obj, states, "i6", by="consensus", seed=4, n_adapt=sched[0], n_burn=sched[1], n_keep=sched[2],
                                   mu=MU6, sig=TAU6, out_dir=str(tmp_path / "bayes"))
    assert [cg["State"] for cg in m.cell_gene] == [5, 4, 2] and all(np.array_equal(cg["Cells"], tum) for cg in m.cell_gene)
    means, cellp = restated_means(obj.expr_data, m.cell_gene, sched, 4)
    same(m.cnv_means, means)
    for a, b in zip(m.cell_probabilities, cellp):
        same(a, b)
    # every cell of region A sits at the neutral state in every iteration, so the 6 x 30 kept theta are independent draws
    # of Dirichlet(201, 1, 1, 1, 1, 1): its mean within 5 standard errors of the exact distribution
    assert abs(m.cnv_means[2, 0] - 201.0 / 206.0) < 5 * np.sqrt(201.0 * 5.0 / (206.0 ** 2 * 207.0) / 180.0)
    f, new_states = bayes_net.filterHighPNormals(m, states, 0.5)
    want = states.copy()
    want[10:60, 20:] = 3                        # removed
    want[120:180, 20:] = 5                      # re-assigned
    assert np.array_equal(new_states, want) and new_states.dtype == states.dtype
    assert [cg["cnv_regions"] for cg in f.cell_gene] == m.cnv_regions[1:] and [cg["State"] for cg in f.cell_gene] == [5, 2]
    assert len(m.cell_gene) == 3 and m.cell_gene[1]["State"] == 4          # the input object is untouched
    dev_states = torch.from_numpy(np.ascontiguousarray(states.T)).cuda()
    _, on_device = bayes_net.filterHighPNormals(m, dev_states, 0.5)
    assert on_device.is_cuda and np.array_equal(on_device.cpu().numpy().T, want)
    lines = open(tmp_path / "bayes" / "CNV_State_Probabilities.dat").read().splitlines()
    assert lines[0].split("\t") == m.cnv_regions[1:] and [ln.split("\t")[0] for ln in lines[1:]] == [f"State:{k}" for k in range(1, 7)]
    # the adjusted reports against those written from the restatement's probabilities by the rule itself
    keep = [i for i in range(3) if not means[2, i] > 0.5]
    ref = bayes_net.MCMCInferCNV(infercnv_obj=obj)
    ref.cell_gene = [dict(m.cell_gene[i], State=int(np.argmax(means[:, i])) + 1) for i in keep]
    for sub, o in (("gpu", f), ("ref", ref)):
        cnv_regions.adjust_genes_regions_report(o, "17_HMM_pred", "HMM_CNV_predictions." + sub, str(tmp_path))
    for suffix in (".pred_cnv_genes.dat", ".pred_cnv_regions.dat"):
        got = open(tmp_path / ("HMM_CNV_predictions.gpu" + suffix)).read()
        assert got == open(tmp_path / ("HMM_CNV_predictions.ref" + suffix)).read()
        assert m.cnv_regions[0] not in got and m.cnv_regions[1] + "\t5\t" in got


def test_filter_remove_cells(dev):
    from infercnv_amd import bayes_net
    obj, states, tum = planted_object(seed=1, half_normal=True)
    sched = (10, 5, 30)
    m = bayes_net.inferCNVBayesNet(obj, states, "i6", by="consensus", postMcmcMethod="removeCells", seed=2, n_adapt=sched[0],
                                   n_burn=sched[1], n_keep=sched[2], mu=MU6, sig=TAU6)
    f, new_states = bayes_net.filterHighPNormals(m, states, 0.5)
    assert np.array_equal(f.cell_gene[0]["Cells"], tum[100:]) and np.array_equal(f.cell_gene[1]["Cells"], tum)
    means, cellp = restated_means(obj.expr_data, f.cell_gene, sched, 2)     # the second run, on the shrunken regions
    same(f.cnv_means, means)
    for a, b in zip(f.cell_probabilities, cellp):
        same(a, b)
    want = states.copy()
    want[10:60, 20:120] = 3                     # the neutral half of A leaves the region
    want[120:180, 20:] = 5
    assert np.array_equal(new_states, want)
    assert [cg["State"] for cg in f.cell_gene] == [5, 5, 2]
