"""The per-cell CNV feature table of add_to_seurat and the run-length segmentation on the GPU (icnv_cnv_features /
icnv_cnv_runs, DESIGN K14): every count, every feature, every run record and every top_ vector equal to the sequential
restatement of tests/cnv_summary_restate.py, which works from the report tables; through the C ABI and through device.py."""
import ctypes as ct
import os

import numpy as np
import pytest

import cnv_summary_restate as rs
import oracle_np as onp

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MU6 = np.array([0.1, 0.5, 1.0, 1.5, 2.0, 3.0])
TAU6 = 1.0 / np.array([0.2, 0.25, 0.3, 0.3, 0.35, 0.4]) ** 2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infercnv_amd import device
    torch.cuda.set_device(0)
    device.init(0)
    return device


def state_obj(obj, states):
    o = obj.copy()
    o.expr_data = np.asarray(states).astype(np.float64)
    return o


def both_routes(dev, states, chr_start, K, s0, order=None, padded=False, neutral=None):
    """states: genes x columns.  The counts, run counts and run records through the C ABI's host flavour and through
    device.py (contiguous or padded rows), asserted equal to each other; returns (counts, run_counts, records, n_runs)."""
    from infercnv_amd import _lib
    L = _lib.load()
    st = np.asfortranarray(np.asarray(states).astype(np.uint8))
    G, C = st.shape
    cs = np.ascontiguousarray(chr_start, dtype=np.int32)
    csp = cs.ctypes.data_as(ct.POINTER(ct.c_int32))
    neutral = s0 if neutral is None else neutral
    counts = np.full((cs.size - 1, C, 4), -1, dtype=np.int32)
    run_counts = np.full((C, 2), -1, dtype=np.int32)
    _lib.check(L.icnv_cnv_features(st.ctypes.data_as(ct.c_void_p), G, C, csp, cs.size - 1, K, s0, counts.ctypes.data_as(ct.c_void_p),
                                   run_counts.ctypes.data_as(ct.c_void_p)))
    idx = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
    ip = None if idx is None else idx.ctypes.data_as(ct.POINTER(ct.c_int32))
    n_cols = C if idx is None else idx.size
    n_rec, n_runs = ct.c_int64(), ct.c_int64()
    _lib.check(L.icnv_cnv_runs(st.ctypes.data_as(ct.c_void_p), G, C, csp, cs.size - 1, ip, n_cols, K, neutral, 0, None, ct.byref(n_rec),
                               ct.byref(n_runs)))
    rec = np.full((6, max(n_rec.value, 1)), -1, dtype=np.int32)
    _lib.check(L.icnv_cnv_runs(st.ctypes.data_as(ct.c_void_p), G, C, csp, cs.size - 1, ip, n_cols, K, neutral, rec.shape[1],
                               rec.ctypes.data_as(ct.c_void_p), ct.byref(n_rec), ct.byref(n_runs)))
    rec = rec[:, :n_rec.value]
    if padded:
        d_st = dev.padded_matrix(C, G, dtype=torch.uint8)
        d_st.copy_(torch.from_numpy(np.ascontiguousarray(st.T)))
    else:
        d_st = torch.from_numpy(np.ascontiguousarray(st.T)).cuda()
    d_counts, d_runs = dev.cnv_features(d_st, cs, K, s0, want_run_counts=True)
    assert np.array_equal(d_counts.cpu().numpy(), counts) and np.array_equal(d_runs.cpu().numpy(), run_counts)
    d_rec, d_n = dev.cnv_runs(d_st, cs, neutral=neutral, K=K, col_idx=idx)
    assert np.array_equal(d_rec.cpu().numpy(), rec) and d_n == n_runs.value
    if neutral == s0:                                      # the counting pass saved: the same records
        d_rec2, _ = dev.cnv_runs(d_st, cs, neutral=neutral, K=K, col_idx=idx, run_counts=d_runs)
        assert np.array_equal(d_rec2.cpu().numpy(), rec)
    return counts, run_counts, rec, n_runs.value


def check_against_numpy(dev, states, chr_start, K, s0, order=None, padded=False, neutral=None):
    counts, run_counts, rec, n_runs = both_routes(dev, states, chr_start, K, s0, order, padded, neutral)
    C = np.asarray(states).shape[1]
    order = np.arange(C) if order is None else np.asarray(order)
    want_counts, want = rs.counts_and_runs_np(states, chr_start, s0, order, neutral=neutral)
    assert np.array_equal(counts, want_counts)
    for k, key in enumerate(("col", "chr", "gene_first", "gene_last", "state", "ordinal")):
        assert np.array_equal(rec[k], want[key]), key
    _, every = rs.counts_and_runs_np(states, chr_start, s0, np.arange(C), neutral=0)
    assert np.array_equal(run_counts[:, 0], np.bincount(every["col"], minlength=C))
    _, nn = rs.counts_and_runs_np(states, chr_start, s0, np.arange(C))
    assert np.array_equal(run_counts[:, 1], np.bincount(nn["col"], minlength=C))
    _, every_listed = rs.counts_and_runs_np(states, chr_start, s0, order, neutral=0)
    assert n_runs == every_listed["col"].size
    return counts, rec


# ---- the reference's fixture --------------------------------------------------------------------------------------------
def fixture_object(golden_dir):
    from infercnv_amd.infercnv_object import GeneOrder, InfercnvObject
    d = np.load(os.path.join(golden_dir, "infercnv_object_example.npz"))
    hs = np.load(os.path.join(golden_dir, "hmm_states_example.npz"))["HMM_states"]
    chr_names = d["chr_levels"][d["chr_codes"] - d["chr_codes"].min()]
    obj = InfercnvObject(expr_data=hs.astype(np.float64), gene_order=GeneOrder(chr_names, d["gene_start"], d["gene_stop"]),
                         reference_grouped_cell_indices={}, observation_grouped_cell_indices={"tumor": d["obs_tumor"], "normal": d["ref_normal"]},
                         tumor_subclusters={"subclusters": {"tumor": {"tumor_s1": d["obs_tumor"]}, "normal": {"normal_s1": d["ref_normal"]}}})
    return obj, hs


@pytest.mark.parametrize("mode", ["i6", "i3"])
@pytest.mark.parametrize("by_cells", [False, True])
def test_fixture(dev, golden_dir, tmp_path, mode, by_cells):
    from infercnv_amd import seurat_interaction as si
    obj, hs = fixture_object(golden_dir)
    if mode == "i3":                                       # states mapped to 1 .. 3: loss, neutral, gain
        hs = np.where(hs < 3, 1, np.where(hs > 3, 3, 2)).astype(np.int8)
    K, s0 = si.N_STATES[mode], si.CENTER_STATE[mode]
    _, chr_start = obj.chr_layout()
    check_against_numpy(dev, hs, chr_start, K, s0)
    want = rs.run_on_object(obj, hs, mode, by_cells)
    got = si.add_to_seurat(obj, state_obj(obj, hs), str(tmp_path), HMM_type=mode, by_cells=by_cells)
    rs.assert_equal_to_library(want, got["features"], got["lines"])
    assert ("proportion_scaled_cnv" in got["features"]) == (mode == "i6")
    assert open(tmp_path / "map_metadata_from_infercnv.txt").read().splitlines() == want["lines"]
    assert open(tmp_path / "top_losses.txt").read().splitlines() == want["top_losses.txt"]
    assert open(tmp_path / "top_duplis.txt").read().splitlines() == want["top_duplis.txt"]
    if not by_cells and mode == "i6":                  # (mapped to i3, neighbouring gains of different states become one run)
        names = [str(n) for n in np.load(os.path.join(golden_dir, "mcmc_cell_gene.npz"))["names"]]
        assert sorted(n for t in got["features"]["top_loss_region_names"] + got["features"]["top_dupli_region_names"] for n in t) == sorted(names)


# ---- the segmentation against the oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("by", ["consensus", "subcluster", "cell"])
def test_runs_and_predicted_regions_against_the_oracle(dev, by):
    """An object whose reference cells are the LAST columns: the by-cell report order is not the matrix order."""
    from infercnv_amd import cnv_regions
    obj, states = rs.synthetic_object(90, 7, seed=3)
    chrs = [str(c) for c in obj.gene_order.chr]
    res = cnv_regions.get_predicted_CNV_regions(obj, by)
    runs = cnv_regions.predicted_cnv_runs(obj, by, neutral=3, K=6)
    groups = cnv_regions._cell_groups(obj, by)
    assert [x["cell_group_name"] for x in res] == [n for n, _ in groups] and len(res) == {"consensus": 2, "subcluster": 8, "cell": 90}[by]
    if by == "cell":
        assert res[0]["cell_group_name"] == "c81" and [int(g[0]) for _, g in groups[:9]] == list(range(81, 90))
    counter, k = 0, 0
    for gi, (entry, (name, idx)) in enumerate(zip(res, groups)):
        cons = onp.state_consensus(states.astype(np.float64), [idx])[:, 0]
        want, counter = onp.define_cnv_gene_regions(cons, chrs, counter)
        assert [rn for rn, _ in entry["gene_regions"]] == [w[0] for w in want]
        for (rn, r), w in zip(entry["gene_regions"], want):
            assert r["state"] == w[1] and r["gene"].tolist() == w[2] and r["chr"] == chrs[w[2][0]]
        for (rn, state, c, s, e), w in zip(entry["cnv_ranges"], want):
            assert rn == w[0] and s == obj.gene_order.start[w[2]].min() and e == obj.gene_order.stop[w[2]].max()
        for w in want:
            if w[1] != 3:
                assert (runs["name"][k], runs["col"][k], runs["state"][k], runs["gene_first"][k], runs["gene_last"][k]) == \
                    (w[0], gi, w[1], w[2][0], w[2][-1])
                assert runs["start"][k] == obj.gene_order.start[w[2]].min() and runs["end"][k] == obj.gene_order.stop[w[2]].max()
                k += 1
    assert k == len(runs["name"]) and runs["n_runs"] == counter
    # device.cnv_runs on the same columns, in the same order: the cells' own columns, or the groups' consensus columns
    _, chr_start = obj.chr_layout()
    if by == "cell":
        _, rec = check_against_numpy(dev, states, chr_start, 6, 3, order=np.concatenate([g for _, g in groups]))
    else:
        d_st = torch.from_numpy(np.ascontiguousarray(states.astype(np.uint8).T)).cuda()
        cons = dev.state_consensus(d_st, [g for _, g in groups]).cpu().numpy().T
        _, rec = check_against_numpy(dev, cons, chr_start, 6, 3)
    assert [f"{chrs[chr_start[c]]}-region_{o}" for c, o in zip(rec[1], rec[5])] == runs["name"]
    assert np.array_equal(rec[0], runs["col"]) and np.array_equal(rec[2], runs["gene_first"]) and np.array_equal(rec[3], runs["gene_last"])


def test_permuted_gene_order(dev):
    """chr_layout() returns a permutation: the genes are gathered first and the regions come back in the object's rows."""
    from infercnv_amd import cnv_regions, seurat_interaction as si
    obj, states = rs.synthetic_object(30, 3, seed=8)
    perm = np.random.default_rng(0).permutation(states.shape[0])
    perm = perm[np.argsort(np.asarray(obj.gene_order.start)[perm], kind="stable")]     # shuffled chromosomes, ordered within
    sh = obj.copy()
    sh.gene_order = type(obj.gene_order)(chr=obj.gene_order.chr[perm], start=obj.gene_order.start[perm], stop=obj.gene_order.stop[perm])
    sh.gene_names, sh.expr_data = obj.gene_names[perm], obj.expr_data[perm]
    assert sh.chr_layout()[0] is not None
    chrs = [str(c) for c in sh.gene_order.chr]
    counter = 0
    for entry, (name, idx) in zip(cnv_regions.get_predicted_CNV_regions(sh, "subcluster"), cnv_regions._cell_groups(sh, "subcluster")):
        want, counter = onp.define_cnv_gene_regions(onp.state_consensus(sh.expr_data, [idx])[:, 0], chrs, counter)
        assert [(rn, r["state"], r["gene"].tolist()) for rn, r in entry["gene_regions"]] == [(w[0], w[1], w[2]) for w in want]
    want = rs.run_on_object(sh, states[perm], "i6", by_cells=False)
    rs.assert_equal_to_library(want, si.get_features(sh, state_obj(sh, states[perm]), "i6", by_cells=False))


# ---- the reports of the existing writers, read back ----------------------------------------------------------------------
@pytest.mark.parametrize("by_cells", [False, True])
def test_reports_read_back_equal_the_state_matrix_route(dev, tmp_path, by_cells):
    from infercnv_amd import cnv_regions, seurat_interaction as si
    obj, states = rs.synthetic_object(140, 12, seed=11)
    cnv_regions.generate_cnv_region_reports(obj, "17_HMM_predHMMi6", str(tmp_path), ignore_neutral_state=3,
                                            by="cell" if by_cells else "subcluster")
    tables = (rs.read_table(tmp_path / "17_HMM_predHMMi6.pred_cnv_regions.dat"), rs.read_table(tmp_path / "17_HMM_predHMMi6.pred_cnv_genes.dat"))
    want = rs.run_on_object(obj, None, "i6", by_cells, tables=tables)
    assert len(want["top_loss"]) == 10 and len(want["top_dupli"]) == 10
    assert max(len(t) for t in want["top_loss_regions"] + want["top_dupli_regions"]) >= (3 if by_cells else 2)
    got = si.add_to_seurat(obj, state_obj(obj, states), str(tmp_path / "out"), by_cells=by_cells)
    rs.assert_equal_to_library(want, got["features"], got["lines"])
    no_group = obj.observation_grouped_cell_indices["tumor"][-2:]
    if not by_cells:                                       # the two cells in no subcluster: zeros and NA
        for c in no_group:
            f = got["lines"][1 + c].split("\t")
            assert f[1] == "NA" and set(f[2:]) == {"0"}
    assert open(tmp_path / "out" / "top_losses.txt").read().splitlines() == want["top_losses.txt"]
    assert open(tmp_path / "out" / "top_duplis.txt").read().splitlines() == want["top_duplis.txt"]


def test_overlapping_groups_and_missing_hmm(dev):
    from infercnv_amd import seurat_interaction as si
    obj, states = rs.synthetic_object(40, 3, seed=1)
    subs = obj.tumor_subclusters["subclusters"]["tumor"]
    subs["tumor_s2"] = np.append(subs["tumor_s2"], subs["tumor_s1"][0])
    with pytest.raises(ValueError):
        si.get_features(obj, state_obj(obj, states), "i6", by_cells=False)
    si.get_features(obj, state_obj(obj, states), "i6", by_cells=True)     # by cell the subclusters play no part
    with pytest.raises(ValueError):
        si.add_to_seurat(obj, None, "unused")


# ---- after the Bayesian filter (K13) --------------------------------------------------------------------------------------
def planted_object(seed=0):
    """The planted object of the K13 tests: 3 chromosomes x 100 genes, 20 reference and 200 tumour cells; A, chr1 genes 10-59,
    state 5 with data at the neutral mean; B, chr2 genes 20-79, state 4 with data at state 5's mean; C, chr3 genes 30-89,
    state 2 with data at state 2's mean.  Here with one subcluster per group, which is what add_to_seurat reports on."""
    from infercnv_amd.infercnv_object import GeneOrder, InfercnvObject
    rng = np.random.default_rng(seed)
    G, C = 300, 220
    tum = np.arange(20, 220)
    expr = rng.normal(MU6[2], 0.3, size=(G, C))
    states = np.full((G, C), 3, dtype=np.int8)
    states[10:60, 20:] = 5
    states[120:180, 20:] = 4
    expr[120:180, 20:] = rng.normal(MU6[4], 0.3, size=(60, 200))
    states[230:290, 20:] = 2
    expr[230:290, 20:] = rng.normal(MU6[1], 0.25, size=(60, 200))
    chrs = np.repeat(np.array(["chr1", "chr2", "chr3"]), 100)
    pos = np.tile(np.arange(100) * 1000 + 1, 3)
    obj = InfercnvObject(expr_data=expr, gene_order=GeneOrder(chr=chrs, start=pos, stop=pos + 500),
                         reference_grouped_cell_indices={"normal": np.arange(20)}, observation_grouped_cell_indices={"tumor": tum},
                         tumor_subclusters={"subclusters": {"normal": {"normal_s1": np.arange(20)}, "tumor": {"tumor_s1": tum}}},
                         gene_names=np.array([f"g{i}" for i in range(G)]), cell_names=np.array([f"c{i}" for i in range(C)]))
    return obj, states, tum


def test_filtered_states_agree_with_adjusted_reports(dev, tmp_path):
    """filterHighPNormals rewrites the state matrix, adjust_genes_regions_report rewrites the step-17 reports: the feature
    table from the filtered states equals the one the reference's route derives from the adjusted reports."""
    from infercnv_amd import bayes_net, cnv_regions, seurat_interaction as si
    obj, states, tum = planted_object()
    cnv_regions.generate_cnv_region_reports(state_obj(obj, states), "17_HMM_predHMMi6", str(tmp_path), ignore_neutral_state=3, by="subcluster")
    m = bayes_net.inferCNVBayesNet(obj, states, "i6", by="subcluster", seed=4, n_adapt=10, n_burn=5, n_keep=30, mu=MU6, sig=TAU6)
    f, new_states = bayes_net.filterHighPNormals(m, states, 0.5)
    assert [cg["State"] for cg in f.cell_gene] == [5, 2] and not np.array_equal(new_states, states)
    cnv_regions.adjust_genes_regions_report(f, "17_HMM_predHMMi6", "HMM_CNV_predictions.HMMi6.Pnorm_0.5", str(tmp_path))
    tables = tuple(rs.read_table(tmp_path / ("HMM_CNV_predictions.HMMi6.Pnorm_0.5" + sfx)) for sfx in (".pred_cnv_regions.dat", ".pred_cnv_genes.dat"))
    want = rs.run_on_object(obj, None, "i6", False, tables=tables)
    got = si.get_features(obj, state_obj(obj, new_states), "i6", by_cells=False)
    rs.assert_equal_to_library(want, got)
    assert got["has_dupli"][:, tum[0]].tolist() == [False, True, False] and got["has_loss"][:, tum[0]].tolist() == [False, False, True]
    assert got["proportion_scaled_dupli"][1, tum[0]] == 120 / 200 and not got["has_cnv"][:, :20].any()


# ---- geometry -------------------------------------------------------------------------------------------------------------
def random_states(rng, G, C, K, s0, density=0.02):
    st = np.full((G, C), s0, dtype=np.uint8)
    for _ in range(max(int(density * G * C / 20), 1)):
        g, c, n = int(rng.integers(0, G)), int(rng.integers(0, C)), int(rng.integers(1, 40))
        st[g:g + n, c] = rng.integers(1, K + 1)
    return st


@pytest.mark.parametrize("G,C,padded", [(1000, 70, False), (1003, 70, False), (1003, 70, True), (131, 1, False), (2600, 129, True),
                                        (1029, 64, False)])
def test_geometry(dev, G, C, padded):
    rng = np.random.default_rng(G + C)
    cuts = np.sort(rng.choice(np.arange(4, G - 4), size=6, replace=False))
    one = int(cuts[2])                                     # gene `one` is a chromosome of its own
    chr_start = np.unique(np.concatenate([[0], cuts, [one + 1, G]]))
    k_one = int(np.searchsorted(chr_start, one))
    assert chr_start[k_one] == one and chr_start[k_one + 1] == one + 1
    st = random_states(rng, G, C, 6, 3)
    st[one, :] = 5                                         # non-neutral on the one-gene chromosome: counted nowhere
    st[chr_start[1] - 3:chr_start[1] + 3, : max(C // 2, 1)] = 2   # one state across a border: two runs
    st[:, 0] = 3                                           # an all-neutral column
    if C > 2:
        st[:, 1] = 1                                       # all non-neutral: state 1
        st[:, 2] = 6                                       # ... and state K
    counts, rec = check_against_numpy(dev, st, chr_start, 6, 3, padded=padded)
    assert not counts[:, 0].any() and not (rec[0] == 0).any()
    if C > 2:
        sizes = np.diff(chr_start)
        assert np.array_equal(counts[:, 1, 0], np.where(sizes >= 2, sizes, 0)) and np.array_equal(counts[:, 2, 3], np.where(sizes >= 2, 3 * sizes, 0))
    assert not counts[k_one].any() and not ((rec[2] <= one) & (rec[3] >= one)).any()
    order = rng.permutation(C)[: max(C - 3, 1)]            # a list that is neither complete nor in order
    check_against_numpy(dev, st, chr_start, 6, 3, order=order, padded=padded)


@pytest.mark.parametrize("G,padded", [(1003, False), (1003, True), (1000, False)])
def test_every_run_of_a_validated_matrix(dev, G, padded):
    """neutral = 0 with K = 6: every run is recorded and every byte is still held to 1 .. K, whatever borders cut the words
    (G and the chromosome starts are not multiples of 4)."""
    rng = np.random.default_rng(G)
    C = 37
    chr_start = np.concatenate([[0], np.sort(rng.choice(np.arange(1, G), size=9, replace=False)), [G]])
    assert (chr_start[1:-1] % 4 != 0).any()
    st = random_states(rng, G, C, 6, 3, density=0.2)
    _, rec = check_against_numpy(dev, st, chr_start, 6, 3, padded=padded, neutral=0)
    assert (rec[4] == 3).any() and (rec[4] != 3).any()     # neutral runs are among the records
    check_against_numpy(dev, st, chr_start, 6, 3, order=rng.permutation(C)[:20], padded=padded, neutral=0)
    st[G - 1, C - 1] = 7
    with pytest.raises(ValueError):
        dev.cnv_runs(torch.from_numpy(np.ascontiguousarray(st.T)).cuda(), chr_start, neutral=0, K=6)


def test_ninety_two_chromosomes_and_i3(dev):
    rng = np.random.default_rng(92)
    G, C = 3001, 77
    chr_start = np.concatenate([[0], np.sort(rng.choice(np.arange(1, G), size=91, replace=False)), [G]])
    check_against_numpy(dev, random_states(rng, G, C, 3, 2, density=0.1), chr_start, 3, 2)
    check_against_numpy(dev, random_states(rng, G, C, 6, 3, density=0.3), chr_start, 6, 3, padded=True)


@pytest.mark.parametrize("byte", [0, 7, 255])
def test_invalid_state_is_refused(dev, byte):
    from infercnv_amd import _lib
    L = _lib.load()
    rng = np.random.default_rng(byte)
    G, C = 700, 40
    st = np.asfortranarray(random_states(rng, G, C, 6, 3))
    st[G - 1, C - 1] = byte
    cs = np.array([0, 300, 699, G], dtype=np.int32)        # the byte sits on a one-gene chromosome
    csp = cs.ctypes.data_as(ct.POINTER(ct.c_int32))
    counts = np.zeros((3, C, 4), dtype=np.int32)
    n_rec = ct.c_int64()
    assert L.icnv_cnv_features(st.ctypes.data_as(ct.c_void_p), G, C, csp, 3, 6, 3, counts.ctypes.data_as(ct.c_void_p), None) == _lib.ERR_ARG
    assert L.icnv_cnv_runs(st.ctypes.data_as(ct.c_void_p), G, C, csp, 3, None, C, 6, 3, 0, None, ct.byref(n_rec), None) == _lib.ERR_ARG
    st[G - 1, C - 1], st[5, 0] = 3, byte                   # ... and inside a chromosome
    assert L.icnv_cnv_features(st.ctypes.data_as(ct.c_void_p), G, C, csp, 3, 6, 3, counts.ctypes.data_as(ct.c_void_p), None) == _lib.ERR_ARG
    d_st = torch.from_numpy(np.ascontiguousarray(st.T)).cuda()
    with pytest.raises(ValueError):
        dev.cnv_features(d_st, cs, 6, 3)
    with pytest.raises(ValueError):
        dev.cnv_runs(d_st, cs, neutral=3, K=6)
    rec, n_runs = dev.cnv_runs(d_st, cs, neutral=0, K=0)   # K = 0: bytes as they are, every run
    _, want = rs.counts_and_runs_np(st, cs, 3, np.arange(C), neutral=0)
    assert np.array_equal(rec.cpu().numpy()[4], want["state"]) and n_runs == want["col"].size
    st[5, 0] = 3
    assert L.icnv_cnv_features(st.ctypes.data_as(ct.c_void_p), G, C, csp, 3, 6, 3, counts.ctypes.data_as(ct.c_void_p), None) == _lib.OK
    small = np.zeros((6, 1), dtype=np.int32)               # a capacity below the record count: refused, nothing written
    assert L.icnv_cnv_runs(st.ctypes.data_as(ct.c_void_p), G, C, csp, 3, None, C, 6, 3, 1, small.ctypes.data_as(ct.c_void_p),
                           ct.byref(n_rec), None) == _lib.ERR_ARG and n_rec.value > 1 and not small.any()


# ---- 2 000 cells by cell --------------------------------------------------------------------------------------------------
def test_two_thousand_cells_by_cell(dev, tmp_path):
    from infercnv_amd import seurat_interaction as si
    obj, states = rs.synthetic_object(2000, 40, seed=2)
    want = rs.run_on_object(obj, states, "i6", by_cells=True)
    assert len(want["top_loss"]) == 10 and len(want["top_dupli"]) == 10          # top_n reached for both signs
    assert max(len(t) for t in want["top_loss_regions"] + want["top_dupli_regions"]) >= 3
    got = si.add_to_seurat(obj, state_obj(obj, states), str(tmp_path), by_cells=True)
    rs.assert_equal_to_library(want, got["features"], got["lines"])
    assert open(tmp_path / "top_losses.txt").read().splitlines() == want["top_losses.txt"]


# ---- past 2^31 bytes ------------------------------------------------------------------------------------------------------
def test_large_shape_against_torch_reductions(dev):
    G, C, K, s0 = 10000, 250000, 6, 3
    gen = torch.Generator(device="cuda").manual_seed(7)
    st = torch.full((C, G), s0, dtype=torch.uint8, device="cuda")
    for _ in range(60):                                    # blocks of non-neutral states, the last columns included
        g = int(torch.randint(0, G - 300, (1,), generator=gen, device="cuda").item())
        c = int(torch.randint(0, C - 5000, (1,), generator=gen, device="cuda").item())
        st[c:c + 5000, g:g + 300] = int(torch.randint(1, K + 1, (1,), generator=gen, device="cuda").item())
    st[C - 3:, 17:9000] = torch.randint(1, K + 1, (3, 8983), generator=gen, device="cuda", dtype=torch.uint8)
    chr_start = np.concatenate([[0], np.sort(np.random.default_rng(1).choice(np.arange(1, G), size=21, replace=False)), [G]])
    assert st.numel() > 2 ** 31
    counts, runs = dev.cnv_features(st, chr_start, K, s0, want_run_counts=True)
    want_all = torch.zeros(C, dtype=torch.int64, device="cuda")
    want_nn = torch.zeros(C, dtype=torch.int64, device="cuda")
    for k in range(chr_start.size - 1):
        a, b = int(chr_start[k]), int(chr_start[k + 1])
        s = st[:, a:b].to(torch.int16)
        if b - a < 2:
            assert not counts[k].any()
            continue
        want = torch.stack([(s < s0).sum(1), (s > s0).sum(1), torch.clamp(s0 - s, min=0).sum(1), torch.clamp(s - s0, min=0).sum(1)], dim=1)
        assert torch.equal(counts[k].to(torch.int64), want), k
        starts = torch.cat([torch.ones((C, 1), dtype=torch.bool, device="cuda"), s[:, 1:] != s[:, :-1]], dim=1)
        want_all += starts.sum(1)
        want_nn += (starts & (s != s0)).sum(1)
    assert torch.equal(runs[:, 0].to(torch.int64), want_all) and torch.equal(runs[:, 1].to(torch.int64), want_nn)
    rec, n_runs = dev.cnv_runs(st, chr_start, neutral=s0, K=K, run_counts=runs)
    assert rec.shape[1] == int(want_nn.sum().item()) and n_runs == int(want_all.sum().item())
    last = rec[:, rec[0] == C - 1].cpu().numpy()           # the last column's records, checked on the host
    _, want = rs.counts_and_runs_np(st[C - 1:].cpu().numpy().T, chr_start, s0, [0])
    assert np.array_equal(last[2], want["gene_first"]) and np.array_equal(last[3], want["gene_last"]) and np.array_equal(last[4], want["state"])
    assert int(last[5][-1]) <= n_runs and int(rec[5][-1].item()) <= n_runs
