"""GPU parity tests (-m gpu) of BASELINE.json configs[0] -- example/run.R's real inputs -- and of the C-ABI entry
points / host-mirror functions that had no GPU test in round 1 (VERDICT r01 "untested entry points"):
icnv_average_bounds[_dev] and threshold "auto", the K = 3 proxy table, the three i3HMM_predict_* wrappers,
i3HMM_get_sd_trend, use_KS."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import oracle_c as oc  # noqa: E402
import oracle_np as onp  # noqa: E402
from parity_util import check_denoise_flips  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infercnv_amd import device
    torch.cuda.set_device(0)
    device.init(0)
    device.viterbi_set_mode(0)
    return device


def to_dev(x_gc):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x_gc, dtype=np.float64).T)).cuda()


def to_host(t_cg):
    return t_cg.cpu().numpy().T


@pytest.fixture(scope="module")
def run_inputs(golden_dir):
    """The infercnv object example/run.R hands to run(): CreateInfercnvObject replayed by tests/golden/make_golden.py."""
    d = np.load(os.path.join(golden_dir, "example_run_inputs.npz"))
    x = d["mant"].astype(np.float64) / 10.0 ** d["neg_exp"].astype(np.float64)
    refs = {str(n): d[f"ref_{i}"] for i, n in enumerate(d["ref_names"])}
    obs = {str(n): d[f"obs_{i}"] for i, n in enumerate(d["obs_names"])}
    return {"counts": x, "chr": d["chr_levels"][d["chr_codes"]], "chr_codes": d["chr_codes"], "refs": refs, "obs": obs}


def test_config1_example_run_inputs_through_the_hip_path(dev, run_inputs):
    """BASELINE.json configs[0] (example/run.R: 184 cells, cutoff = 1, denoise, sd_amplifier = 2, HMM i6): run()'s
    steps 2, 3, 4 (gene filters, depth normalisation, log2(x + 1)), the smoothing chain 8-14 + 22 and the i6 HMM
    (per cell and on whole samples), every step through the host mirror -> C ABI -> HIP kernels, against the oracle.
    Real chromosome layout (chrX/Y/M excluded by CreateInfercnvObject, 22 autosomes of 108 .. 1011 genes), two reference
    groups of 19 / 23 cells, four tumour groups."""
    from infercnv_amd import GeneOrder, InfercnvObject, hmm, ops
    x = run_inputs["counts"]
    assert x.shape == (9939, 184) and len(run_inputs["refs"]) == 2 and len(run_inputs["obs"]) == 4
    obj = InfercnvObject(expr_data=x, count_data=x, gene_order=GeneOrder(chr=run_inputs["chr"]),
                         reference_grouped_cell_indices=run_inputs["refs"],
                         observation_grouped_cell_indices=run_inputs["obs"])
    # step 2 (R/inferCNV_ops.R:560-564)
    o = ops.require_above_min_mean_expr_cutoff(obj, 1)
    o = ops.require_above_min_cells_ref(o, 3)
    drop1 = onp.below_min_mean_expr_cutoff(x, 1)
    keep = np.setdiff1d(np.arange(x.shape[0]), drop1)
    keep = keep[onp.genes_passing_min_cells(x[keep], 3)]
    assert o.expr_data.shape[0] == keep.size and 3000 < keep.size < x.shape[0]
    np.testing.assert_array_equal(o.expr_data, x[keep])
    np.testing.assert_array_equal(np.asarray(o.gene_order.chr), run_inputs["chr"][keep])
    # steps 3, 4 (:586, :614)
    o = ops.log2xplus1(ops.normalize_counts_by_seq_depth(o))
    want_log = onp.log2xplus1(onp.normalize_counts_by_seq_depth(x[keep]))
    assert np.abs(o.expr_data - want_log).max() < 1e-12
    # chain: stand-alone steps in run()'s order and the fused entry, sd_amplifier = 2 as example/run.R passes
    refs = list(run_inputs["refs"].values())
    cs = oc.chr_starts_from_codes(run_inputs["chr_codes"][keep])
    assert len(cs) == 23
    want_out, want_pre, musd = oc.smooth_chain(o.expr_data, cs, refs, sd_amplifier=2.0, want_pre_denoise=True)
    s = ops.subtract_ref_expr_from_obs(o)
    s = ops.apply_max_threshold_bounds(s, 3)
    s = ops.smooth_by_chromosome(s, 101)
    s = ops.center_cell_expr_across_chromosome(s, "median")
    s = ops.subtract_ref_expr_from_obs(s)
    s14 = ops.invert_log2(s)
    s22 = ops.clear_noise_via_ref_mean_sd(s14, 2)
    fused, hmm_in = ops.hip_smooth_chain(o, sd_amplifier=2, return_hmm_input=True)
    for got in (s14.expr_data, hmm_in.expr_data):
        assert np.abs(got - want_pre).max() / np.abs(want_pre).max() < 1e-5      # north-star tolerance
        assert np.abs(got - want_pre).max() < 1e-11
    for got, label in ((s22.expr_data, "config 1, step functions"), (fused.expr_data, "config 1, fused")):
        check_denoise_flips(got, want_out, want_pre, *musd, tol=1e-11, label=label)   # strict select at the bounds
    # i6 HMM: identical inputs (the HIP chain's own output) -> bit-exact states
    cnv = {k: {"mean": m, "sd": sdv} for k, m, sdv in zip(hmm.CNV_LEVELS, (0.41234766, 0.84075773, 1.01693983, 1.12238786,
                                                                       1.23842619, 1.44298781),
                                                          (0.02889, 0.16455, 0.10555, 0.19057, 0.24409, 0.29007))}
    means = [cnv[k]["mean"] for k in hmm.CNV_LEVELS]
    sd = float(onp.r_median(np.array([cnv[k]["sd"] for k in hmm.CNV_LEVELS])))
    Pi, delta = onp.get_HMM_i6(1e-6)
    cells = hmm.predict_CNV_via_HMM_on_indiv_cells(hmm_in, cnv)
    want_cells, bad = oc.viterbi_cells(hmm_in.expr_data, cs, means, sd, np.log(Pi), np.log(delta))
    assert bad == 0
    np.testing.assert_array_equal(cells.expr_data, want_cells)
    assert len(np.unique(want_cells)) >= 4                                     # real CNV calls, not one flat state
    samples = hmm.predict_CNV_via_HMM_on_whole_tumor_samples(hmm_in, True, cnv)
    groups = list(run_inputs["obs"].values()) + list(run_inputs["refs"].values())
    gm = to_host(dev.group_means(to_dev(hmm_in.expr_data), groups))
    for q, g in enumerate(groups):
        w, _ = oc.viterbi_cells(gm[:, q:q + 1], cs, means, sd, np.log(Pi), np.log(delta))
        for c in (g[0], g[-1]):
            np.testing.assert_array_equal(samples.expr_data[:, c], w[:, 0])
    # the known biology of this data set shows: oligodendroglioma = 1p / 19q co-deletion in the malignant cells
    chr_of = run_inputs["chr"][keep]
    mal = np.concatenate(list(run_inputs["obs"].values()))
    ref = np.concatenate(refs)
    for arm_chr in ("chr1", "chr19"):
        rows = chr_of == arm_chr
        assert (samples.expr_data[np.ix_(rows, mal)] < 3).mean() > 0.3
        assert (samples.expr_data[np.ix_(rows, ref)] == 3).mean() > 0.9


@pytest.mark.parametrize("which", ["B", "C"])
def test_hmm_states_rda_through_the_hip_path(dev, golden_dir, which):
    """A regression target, NOT a pin (tests/test_hmm_pin.py says why: seven FITTED parameters; with the fixture's paired means
    9 142 / 9 226).  data/HMM_states.rda through the HIP path: counts of the example object -> steps 3, 4 -> fused chain ->
    group means -> i6 Viterbi per group (C ABI, device-resident) with a fitted parameter set (HMM_STATES_PINS): the HIP path
    agrees with the NumPy and the C restatement in all 9 226 group-gene calls; and with the PAIRED means (mcmc_obj@mu) it gives
    the oracle's 9 142, call for call."""
    import oracle_np as onp
    from test_hmm_pin import HMM_STATES_PINS
    d = np.load(os.path.join(golden_dir, "infercnv_object_example.npz"))
    gold = np.load(os.path.join(golden_dir, "hmm_states_example.npz"))["HMM_states"].astype(np.uint8)
    log = onp.log2xplus1(onp.normalize_counts_by_seq_depth(d["count_data"]))
    cs = oc.chr_starts_from_codes(d["chr_codes"])
    _, pre = dev.smooth_chain(to_dev(log), cs, [d["ref_normal"]], want_pre_denoise=True)
    groups = [d["obs_tumor"], d["ref_normal"]]
    Pi, delta = onp.get_HMM_i6(1e-6)
    mu, sd = HMM_STATES_PINS[which]
    st, bad = dev.viterbi_groups(pre, cs, groups, np.array(mu), [sd, sd], np.log(Pi), np.log(delta))
    torch.cuda.synchronize()
    assert int(bad.item()) == 0
    np.testing.assert_array_equal(to_host(st), gold)
    paired = np.load(os.path.join(golden_dir, "hmm_states_example.npz"))["mu"]
    st2, _ = dev.viterbi_groups(pre, cs, groups, paired, [0.24, 0.24], np.log(Pi), np.log(delta))
    want2, _ = oc.viterbi_groups(to_host(pre), cs, groups, paired, [0.24, 0.24], np.log(Pi), np.log(delta))
    np.testing.assert_array_equal(to_host(st2), want2)
    assert int((want2 == gold).sum()) == 9142 * 10      # 20 cells: 10 per group, every cell carries its group's call


def test_mcmc_obj_cell_gene_regions_through_the_hip_path(dev, golden_dir):
    """SURVEY.md 8f #2 against the reference-held golden (tests/golden/mcmc_cell_gene.npz = data/mcmc_obj.rda @cell_gene /
    @cnv_regions, the nine CNV regions the reference derived from data/HMM_states.rda): the device consensus
    (icnv_state_consensus) + the host mirror of .define_cnv_gene_regions / generate_cnv_region_reports give the nine names,
    their 1-based gene rows and their cell columns exactly, and the pred_cnv_genes.dat / cell_groupings files read back the way
    getGenesCells does (R/inferCNV_BayesNet.R:245-266) give @cell_gene.  The fixture's counter starts at the tumour group
    (observation groups only: the legacy group order, R/inferCNV_HMM.R:720), so the object here has no reference group."""
    import tempfile
    from infercnv_amd import cnv_regions
    from infercnv_amd.infercnv_object import GeneOrder, InfercnvObject
    d = np.load(os.path.join(golden_dir, "infercnv_object_example.npz"))
    hs = np.load(os.path.join(golden_dir, "hmm_states_example.npz"))["HMM_states"].astype(np.float64)
    cg = np.load(os.path.join(golden_dir, "mcmc_cell_gene.npz"))
    names = [str(n) for n in cg["names"]]
    chr_names = d["chr_levels"][d["chr_codes"] - d["chr_codes"].min()]
    obj = InfercnvObject(expr_data=hs, gene_order=GeneOrder(chr_names, d["gene_start"], d["gene_stop"]),
                         reference_grouped_cell_indices={}, observation_grouped_cell_indices={"tumor": d["obs_tumor"]})
    res = cnv_regions.get_predicted_CNV_regions(obj, "consensus")
    assert len(res) == 1 and res[0]["cell_group_name"] == "tumor"
    reported = [(rn, r) for rn, r in res[0]["gene_regions"] if r["state"] != 3]
    assert [rn for rn, _ in reported] == names
    for i, (rn, r) in enumerate(reported):
        assert np.array_equal(r["gene"] + 1, cg[f"genes_{i}"])
    cells = obj.cells()
    assert np.array_equal(np.sort(np.nonzero(np.isin(cells, res[0]["cells"]))[0]) + 1, cg["cells_0"])
    # ... and through the report files, read back like getGenesCells
    with tempfile.TemporaryDirectory() as tmp:
        cnv_regions.generate_cnv_region_reports(obj, "17_HMM_pred", tmp, ignore_neutral_state=3, by="consensus")
        rows = [l.split("\t") for l in open(os.path.join(tmp, "17_HMM_pred.pred_cnv_genes.dat")).read().splitlines()[1:]]
        grp = [l.split("\t") for l in open(os.path.join(tmp, "17_HMM_pred.cell_groupings")).read().splitlines()[1:]]
    seen = list(dict.fromkeys(r[1] for r in rows))                       # unique(gene_region_name), order of appearance
    assert seen == names and sorted(seen) == [str(v) for v in cg["levels"]]
    genes = obj.genes()
    for i, n in enumerate(names):
        cur = [r for r in rows if r[1] == n]
        gene_idx = np.nonzero(np.isin(genes, [r[3] for r in cur]))[0] + 1
        sub = {r[0] for r in cur}
        cells_idx = np.nonzero(np.isin(cells, [c for g, c in grp if g in sub]))[0] + 1
        assert np.array_equal(gene_idx, cg[f"genes_{i}"]) and np.array_equal(cells_idx, cg[f"cells_{i}"])


def test_below_min_mean_expr_cutoff_reference_literals_through_the_hip_path(dev):
    """tests/testthat/test_infer_cnv.R:175-220 through ops.require_above_min_mean_expr_cutoff -> icnv_gene_stats /
    icnv_select_genes: the genes the reference's literal answers list are the ones removed."""
    from infercnv_amd import GeneOrder, InfercnvObject, ops
    m1 = np.arange(1, 6, dtype=float).reshape(5, 1)
    m3 = np.arange(1, 16, dtype=float).reshape(3, 5).T
    cases = [(m1, 10, [1, 2, 3, 4, 5]), (m3, 10, [1, 2, 3, 4]), (m1, 2, [1]), (m3, 8.4, [1, 2, 3]), (m1, 0, []), (m3, 100, [1, 2, 3, 4, 5])]
    for m, cut, below in cases:
        obj = InfercnvObject(expr_data=m.copy(), count_data=m.copy(), gene_order=GeneOrder(chr=["chr1"] * 5),
                             reference_grouped_cell_indices={"a": np.array([0])},
                             observation_grouped_cell_indices={"b": np.arange(m.shape[1])})
        keep = np.array([g for g in range(1, 6) if g not in below], dtype=np.int64)
        o = ops.require_above_min_mean_expr_cutoff(obj, cut)      # (no gene left: a 0-row object, like remove_genes in R)
        np.testing.assert_array_equal(o.expr_data, m[keep - 1])
        assert o.expr_data.shape == (keep.size, m.shape[1]) and len(o.gene_order.chr) == keep.size


def test_remove_outliers_norm_reference_literals_through_the_hip_path(dev):
    """Step 16 of run() (remove_outliers_norm, R/inferCNV_ops.R:1969-2054): the reference's three literal cases
    (tests/testthat/test_infer_cnv.R:404-433) through ops.remove_outliers_norm -> icnv_remove_outliers, the hspike mirror,
    the refusals, and a random matrix against the oracle (host buffers and device-resident)."""
    from infercnv_amd import GeneOrder, InfercnvObject, ops

    def obj_of(m, hspike=None):
        return InfercnvObject(expr_data=np.array(m, dtype=np.float64), gene_order=GeneOrder(chr=["chr1"] * m.shape[0]),
                              reference_grouped_cell_indices={"a": np.array([0])},
                              observation_grouped_cell_indices={"b": np.arange(1, m.shape[1])}, hspike=hspike)
    in1 = np.arange(1, 21, dtype=float).reshape(4, 5).T
    np.testing.assert_array_equal(ops.remove_outliers_norm(obj_of(in1), lower_bound=-1, upper_bound=30).expr_data, in1)
    out1 = np.array([5] * 5 + list(range(6, 15)) + [15] * 6, dtype=float).reshape(4, 5).T
    np.testing.assert_array_equal(ops.remove_outliers_norm(obj_of(in1), lower_bound=5, upper_bound=15).expr_data, out1)
    col = np.arange(1, 16, dtype=float)
    in2 = np.stack([col, np.array([-5, -4] + list(range(3, 14)) + [21, 26], dtype=float), col, col], axis=1)
    out2 = in2.copy()
    out2[:2, 1] = -0.5
    out2[13:, 1] = 17.75
    got = ops.remove_outliers_norm(obj_of(in2, hspike=obj_of(in1)), out_method="average_bound")
    np.testing.assert_array_equal(got.expr_data, out2)
    np.testing.assert_array_equal(got.hspike.expr_data, onp.remove_outliers_norm(in1))          # mirrored with ITS own average bounds
    with pytest.raises(ValueError):
        ops.remove_outliers_norm(obj_of(in1), out_method="quantile")
    with pytest.raises(ValueError):
        ops.remove_outliers_norm(obj_of(in1), out_method=None)
    rng = np.random.default_rng(8)
    x = np.asfortranarray(rng.normal(1.0, 0.3, size=(3001, 257)))
    x[5, 7] = np.nan                                                                             # a NaN passes through both tests
    want = onp.remove_outliers_norm(np.nan_to_num(x, nan=1.0))
    got = ops.remove_outliers_norm(obj_of(np.nan_to_num(x, nan=1.0))).expr_data
    np.testing.assert_array_equal(got, want)
    xd = to_dev(np.nan_to_num(x, nan=1.0))
    outd, (lo, hi) = dev.remove_outliers(xd)
    wlo, whi = onp.get_average_bounds(np.nan_to_num(x, nan=1.0))
    assert abs(lo - wlo) < 1e-15 and abs(hi - whi) < 1e-15
    np.testing.assert_array_equal(to_host(outd), want)
    outd2, _ = dev.remove_outliers(to_dev(x), 0.8, 1.2)
    h = to_host(outd2)
    assert np.isnan(h[5, 7]) and np.nanmin(h) == 0.8 and np.nanmax(h) == 1.2


def test_scale_infercnv_expr_vs_oracle(dev):
    """Step 5 of run() (scale_data; R/inferCNV_ops.R:3174-3185): t(scale(t(x))) through ops.scale_infercnv_expr ->
    icnv_scale_genes against the oracle's restatement of scale.default; the hspike mirror; a constant gene becomes NaN as in R."""
    from infercnv_amd import GeneOrder, InfercnvObject, ops
    rng = np.random.default_rng(4)
    x = np.asfortranarray(rng.lognormal(0.5, 0.8, size=(2501, 333)))
    x[17] = 2.5                                                                           # constant gene: 0 / 0
    hs = InfercnvObject(expr_data=x[:40, :9].copy() + 1.0, gene_order=GeneOrder(chr=["c"] * 40),
                        reference_grouped_cell_indices={"a": np.array([0])}, observation_grouped_cell_indices={"b": np.arange(1, 9)})
    obj = InfercnvObject(expr_data=x, gene_order=GeneOrder(chr=["c"] * x.shape[0]), reference_grouped_cell_indices={"a": np.array([0])},
                         observation_grouped_cell_indices={"b": np.arange(1, x.shape[1])}, hspike=hs)
    got = ops.scale_infercnv_expr(obj)
    want = onp.scale_rows(x)
    assert np.isnan(got.expr_data[17]).all() and np.isnan(want[17]).all()
    ok = np.arange(x.shape[0]) != 17
    assert np.abs(got.expr_data[ok] - want[ok]).max() < 1e-12
    assert np.abs(got.expr_data[ok].mean(axis=1)).max() < 1e-13 and np.abs(got.expr_data[ok].std(axis=1, ddof=1) - 1.0).max() < 1e-12
    whs = onp.scale_rows(hs.expr_data)                                                    # (gene 17 is constant there too)
    assert np.array_equal(np.isnan(got.hspike.expr_data), np.isnan(whs)) and np.nanmax(np.abs(got.hspike.expr_data - whs)) < 1e-12


def test_remove_genes_at_ends_of_chromosomes(dev):
    """Step 13 of run() (R/inferCNV_ops.R:3000-3033): (window_length - 1) / 2 genes off either end of every chromosome, a
    short chromosome loses a third at either end, one shorter than 3 genes nothing; rows selected on the device."""
    from infercnv_amd import GeneOrder, InfercnvObject, ops
    sizes = {"chr1": 30, "chr2": 7, "chr3": 2, "chr4": 12}
    chrs = np.concatenate([[k] * n for k, n in sizes.items()])
    G = chrs.size
    x = np.arange(G * 3, dtype=np.float64).reshape(3, G).T.copy()
    obj = InfercnvObject(expr_data=x, gene_order=GeneOrder(chr=chrs), reference_grouped_cell_indices={"a": np.array([0])},
                         observation_grouped_cell_indices={"b": np.array([1, 2])})
    got = ops.remove_genes_at_ends_of_chromosomes(obj, 11)          # tail 5
    # chr1 (30 genes): 5 off either end; chr2 (7 < 2 * 5): floor(7 / 3) = 2 off either end; chr3 (2 genes): untouched; chr4 (12): 5 off either end
    keep = list(range(5, 25)) + list(range(32, 35)) + [37, 38] + list(range(39 + 5, 39 + 7))
    np.testing.assert_array_equal(got.expr_data, x[keep])
    assert list(got.gene_order.chr) == list(chrs[keep])
    with pytest.raises(ValueError, match="No genes removed"):       # tail 2 < 3: nothing to remove -> the reference stops (stop(1234), R/inferCNV_ops.R:3029-3031)
        ops.remove_genes_at_ends_of_chromosomes(obj, 5)
    # mirrored on the hidden spike-in (its own gene order): R/inferCNV_ops.R:3035-3038
    hchrs = np.concatenate([["chrA"] * 20, ["chrB"] * 9])
    hx = np.arange(29 * 2, dtype=np.float64).reshape(2, 29).T.copy()
    hs = InfercnvObject(expr_data=hx, gene_order=GeneOrder(chr=hchrs), reference_grouped_cell_indices={"a": np.array([0])},
                        observation_grouped_cell_indices={"b": np.array([1])})
    obj2 = InfercnvObject(expr_data=x, gene_order=GeneOrder(chr=chrs), reference_grouped_cell_indices={"a": np.array([0])},
                          observation_grouped_cell_indices={"b": np.array([1, 2])}, hspike=hs)
    got2 = ops.remove_genes_at_ends_of_chromosomes(obj2, 11)
    np.testing.assert_array_equal(got2.expr_data, x[keep])
    hkeep = list(range(5, 15)) + list(range(20 + 3, 20 + 6))        # chrA: 5 off either end; chrB (9 < 10): floor(9 / 3) = 3 off either end
    np.testing.assert_array_equal(got2.hspike.expr_data, hx[hkeep])
    assert list(got2.hspike.gene_order.chr) == list(hchrs[hkeep])


def test_average_bounds_and_auto_threshold(dev):
    """icnv_average_bounds[_dev] (get_average_bounds, R/inferCNV_ops.R:2723-2742) and step 9 with threshold "auto"
    (run(): mean(abs(get_average_bounds()), :802-817)."""
    from infercnv_amd import GeneOrder, InfercnvObject, ops, synth
    for G, C in ((10000, 130), (4613, 20), (257, 3), (1, 5)):
        rng = np.random.default_rng(G)
        x = rng.normal(0.0, 0.4, size=(G, C))
        x[rng.integers(0, G, 8), rng.integers(0, C, 8)] = rng.choice([7.5, -6.25, 0.0], 8)
        lo, hi = dev.average_bounds(to_dev(x))
        wlo, whi = oc.get_average_bounds(x)
        nlo, nhi = onp.get_average_bounds(x)
        assert abs(lo - wlo) < 1e-15 and abs(hi - whi) < 1e-15 and abs(lo - nlo) < 1e-15 and abs(hi - nhi) < 1e-15
    # the reference's own literal (tests/testthat/test_infer_cnv.R:405-433 shape): per-cell min / max, then means
    m = np.array([[1.0, -2.0, 3.0], [4.0, 5.0, -6.0], [0.5, 0.25, 0.0]])
    lo, hi = dev.average_bounds(to_dev(m))
    assert lo == np.mean([0.5, -2.0, -6.0]) and hi == np.mean([4.0, 5.0, 3.0])
    # host flavour + "auto" through the host mirror
    cs = synth.chr_layout(600)
    x = np.random.default_rng(9).normal(0.0, 1.0, size=(600, 40))    # symmetric: both clamps bite
    chr_names = np.repeat(np.arange(22), np.diff(cs)).astype(str)
    obj = InfercnvObject(expr_data=x, gene_order=GeneOrder(chr=chr_names),
                         reference_grouped_cell_indices={"n": np.arange(4, dtype=np.int32)},
                         observation_grouped_cell_indices={"t": np.arange(4, 40, dtype=np.int32)})
    lo, hi = ops.get_average_bounds(obj)
    assert (lo, hi) == tuple(oc.get_average_bounds(x))
    thr = (abs(lo) + abs(hi)) / 2
    got = ops.apply_max_threshold_bounds(obj, "auto").expr_data
    np.testing.assert_array_equal(got, onp.apply_max_threshold_bounds(x, thr))
    assert (got == thr).any() and (got == -thr).any()
    with pytest.raises(ValueError):
        ops.apply_max_threshold_bounds(obj, "automatic")


def test_states_to_proxy_i3_and_i6_tables(dev):
    """assign_HMM_states_to_proxy_expr_vals: i6 {1..6} -> {0, 0.5, 1, 1.5, 2, 3} (R/inferCNV_HMM.R:1191-1206), i3
    {1, 2, 3} -> {0.5, 1, 1.5} (R/inferCNV_i3HMM.R:405-417); device and host flavours."""
    from infercnv_amd import GeneOrder, InfercnvObject, hmm
    rng = np.random.default_rng(0)
    for K, table in ((3, [0.5, 1.0, 1.5]), (6, [0.0, 0.5, 1.0, 1.5, 2.0, 3.0])):
        st = rng.integers(1, K + 1, size=(301, 17)).astype(np.uint8)
        st[:K, 0] = np.arange(1, K + 1)
        got = to_host(dev.states_to_proxy(torch.from_numpy(np.ascontiguousarray(st.T)).cuda(), K))
        want = np.asarray(table)[st.astype(np.int64) - 1]
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got, oc.states_to_proxy(st, K))
        np.testing.assert_array_equal(got, (onp.i3HMM_assign_HMM_states_to_proxy_expr_vals if K == 3
                                            else onp.assign_HMM_states_to_proxy_expr_vals)(st))
        obj = InfercnvObject(expr_data=st.astype(np.float64), gene_order=GeneOrder(chr=np.array(["chr1"] * 301)))
        f = hmm.i3HMM_assign_HMM_states_to_proxy_expr_vals if K == 3 else hmm.assign_HMM_states_to_proxy_expr_vals
        np.testing.assert_array_equal(f(obj).expr_data, want)


def test_i3_wrappers_and_sd_trend(dev):
    """i3HMM_get_sd_trend (mu, sigma over all reference values, delta = |qnorm(p, 0, sigma)|: R/inferCNV_i3HMM.R:17-80,
    435-445) against oracle_np.i3_params, and the three i3HMM_predict_CNV_via_HMM_on_* wrappers
    (R/inferCNV_i3HMM.R:180-225, 249-308, 332-389) against the oracle on identical inputs."""
    from infercnv_amd import GeneOrder, InfercnvObject, hmm, synth
    G, C = 3000, 96
    x, cs = synth.make_matrix_np(G, C)
    refs, obs = synth.groups(C)
    _, pre, _ = oc.smooth_chain(x, cs, refs, want_pre_denoise=True)
    chr_names = np.repeat(np.arange(22), np.diff(cs)).astype(str)
    sub = {"subclusters": {"t0": {"t0_s1": obs[0][:10], "t0_s2": obs[0][10:]}, "t1": {"t1_s1": obs[1]},
                           "t2": {"t2_s1": obs[2]}, "t3": {"t3_s1": obs[3]},
                           "r0": {"r0_s1": refs[0]}, "r1": {"r1_s1": refs[1]}}}
    obj = InfercnvObject(expr_data=pre, gene_order=GeneOrder(chr=chr_names),
                         reference_grouped_cell_indices={"r0": refs[0], "r1": refs[1]},
                         observation_grouped_cell_indices={f"t{q}": obs[q] for q in range(4)}, tumor_subclusters=sub)
    for p_val in (0.05, 0.01):
        tr = hmm.i3HMM_get_sd_trend(obj, p_val)
        mu, sigma, delta = onp.i3_params(pre, np.concatenate(refs), p_val)
        assert abs(tr["mu"] - mu) < 1e-13 and abs(tr["sigma"] - sigma) < 1e-13 and abs(tr["mean_delta"] - delta) < 1e-12
    tr = hmm.i3HMM_get_sd_trend(obj, 0.05)
    m3 = np.array([tr["mu"] - tr["mean_delta"], tr["mu"], tr["mu"] + tr["mean_delta"]])
    Pi, delta = onp.get_HMM_i3(1e-6)
    assert abs(Pi[0].sum() - (1 - 3e-6)) < 1e-15                 # the reference's 1 - 5t diagonal with three states
    # per cell
    got = hmm.i3HMM_predict_CNV_via_HMM_on_indiv_cells(obj, 0.05, use_KS=False)
    want, _ = oc.viterbi_cells(pre, cs, m3, tr["sigma"], np.log(Pi), np.log(delta))
    np.testing.assert_array_equal(got.expr_data, want)
    assert set(np.unique(want)) == {1, 2, 3}
    # subclusters and whole samples: Viterbi on the group means (the GPU's own means as the oracle's input), broadcast
    xd = to_dev(pre)
    for fn, groups in ((lambda: hmm.i3HMM_predict_CNV_via_HMM_on_tumor_subclusters(obj, 0.05, use_KS=False),
                        [np.asarray(v) for g in sub["subclusters"].values() for v in g.values()]),
                       (lambda: hmm.i3HMM_predict_CNV_via_HMM_on_whole_tumor_samples(obj, True, 0.05, use_KS=False),
                        [obs[q] for q in range(4)] + list(refs)),
                       # cluster_by_groups = FALSE: the reference's c(all_observations = unlist(.), refs) makes every
                       # observation cell a sample of its own (R/inferCNV_i3HMM.R:355) -- its own profile, not a mean
                       (lambda: hmm.i3HMM_predict_CNV_via_HMM_on_whole_tumor_samples(obj, False, 0.05, use_KS=False),
                        [np.array([c]) for c in np.concatenate(obs)] + list(refs))):
        got = fn().expr_data
        gm = to_host(dev.group_means(xd, groups))
        for q, g in enumerate(groups):
            w, _ = oc.viterbi_cells(gm[:, q:q + 1], cs, m3, tr["sigma"], np.log(Pi), np.log(delta))
            for c in (g[0], g[len(g) // 2], g[-1]):
                np.testing.assert_array_equal(got[:, c], w[:, 0])
        # end to end against the oracle's own group means (R's rowMeans arithmetic): bit-exact states
        full = onp.predict_cnv_on_groups(pre, np.repeat(np.arange(22), np.diff(cs)), groups, m3,
                                         [np.full(3, tr["sigma"])] * len(groups), Pi, delta)
        member = np.concatenate([np.asarray(g) for g in groups])
        np.testing.assert_array_equal(got[:, member], full[:, member])
    # no subclusters -> whole samples (R/inferCNV_i3HMM.R:262-266)
    obj2 = obj.copy()
    obj2.tumor_subclusters = None
    np.testing.assert_array_equal(hmm.i3HMM_predict_CNV_via_HMM_on_tumor_subclusters(obj2, 0.05, use_KS=False).expr_data,
                                  hmm.i3HMM_predict_CNV_via_HMM_on_whole_tumor_samples(obj, True, 0.05, use_KS=False).expr_data)
    # use_KS = TRUE is the reference's default: the KS-based delta draws from R's RNG stream (R/inferCNV_i3HMM.R:469-493), so
    # without its state the call is refused (not a TypeError) ...
    with pytest.raises(NotImplementedError, match="use_KS"):
        hmm.i3HMM_predict_CNV_via_HMM_on_indiv_cells(obj, 0.05)
    # ... with a seed (as in set.seed(seed) before the call) it is get_HoneyBADGER_setGexpDev on R's own stream: product
    # against the oracle's independent restatement, k_cells = the number of reference cells
    tr11 = hmm.i3HMM_get_sd_trend(obj, 0.05, seed=11)
    ks = onp.honeybadger_set_gexp_dev(tr["sigma"], 0.05, len(np.concatenate(refs)), 11)
    assert abs(tr11["KS_delta"] - ks) < 1e-12 and 0.0 < ks < 3 * tr["sigma"]
    m3k = np.array([tr["mu"] - ks, tr["mu"], tr["mu"] + ks])
    want, _ = oc.viterbi_cells(pre, cs, m3k, tr["sigma"], np.log(Pi), np.log(delta))
    np.testing.assert_array_equal(hmm.i3HMM_predict_CNV_via_HMM_on_indiv_cells(obj, 0.05, seed=11).expr_data, want)
    np.testing.assert_array_equal(hmm.i3HMM_predict_CNV_via_HMM_on_indiv_cells(obj, 0.05, sd_trend=tr11).expr_data, want)
    # ... or the caller brings the KS delta computed in R
    tr_ks = dict(tr, KS_delta=0.07)
    got = hmm.i3HMM_predict_CNV_via_HMM_on_indiv_cells(obj, 0.05, sd_trend=tr_ks, use_KS=True)
    m3k = np.array([tr["mu"] - 0.07, tr["mu"], tr["mu"] + 0.07])
    want, _ = oc.viterbi_cells(pre, cs, m3k, tr["sigma"], np.log(Pi), np.log(delta))
    np.testing.assert_array_equal(got.expr_data, want)


# ------------------------------------------------------------------ host-buffer path: residency, several devices
def _host_chain_and_hmm(L, x, cs, refs, hmm):
    import ctypes as ct
    from infercnv_amd._lib import Cfg, check, f64, i32
    G, C = x.shape
    out = np.empty_like(x, order="F")
    pre = np.empty_like(x, order="F")
    st = np.empty((G, C), dtype=np.uint8, order="F")
    cfg = Cfg(G, C, cs, refs)
    vp = lambda a: a.ctypes.data_as(ct.c_void_p)
    check(L.icnv_smooth_chain(vp(x), vp(out), vp(pre), cfg.ptr()))
    means, sd, logPi, logDelta = hmm
    m, mp = f64(means)
    lp = np.asfortranarray(logPi)
    ld, ldp = f64(logDelta)
    csa, csp = i32(cs)
    check(L.icnv_viterbi_cells(vp(pre), vp(st), G, C, csp, csa.size - 1, len(means), mp, float(sd),
                               lp.ctypes.data_as(ct.POINTER(ct.c_double)), ldp))
    return out, pre, st


def test_residency_skips_uploads_and_notices_changes(dev):
    """icnv_residency(1): a host matrix the library produced (or uploaded) is recognised when it comes back -- by content:
    length, a strided sample as the quick reject, then a 64-bit hash of every value -- and not uploaded again; same
    results as without; a matrix that differs in ONE element the sample does not see, at the same address and of the same
    shape (what an in-place edit or R's allocator reusing a freed address produce), is uploaded again."""
    import ctypes as ct
    from infercnv_amd import _lib, synth
    from infercnv_amd._lib import Cfg, check
    L = _lib.load()
    G, C = 3000, 257
    x, cs = synth.make_matrix_np(G, C)
    x = np.asfortranarray(x)
    refs, _ = synth.groups(C)
    hmm = synth.hmm_params_i6()
    stats = lambda: list((lambda b: (check(L.icnv_residency_stats(b)), b)[1])((ct.c_int64 * 4)()))
    base = _host_chain_and_hmm(L, x, cs, refs, hmm)
    try:
        check(L.icnv_residency(1))
        s0 = stats()
        got = _host_chain_and_hmm(L, x, cs, refs, hmm)          # x uploaded; out, pre published; pre recognised by the Viterbi
        s1 = stats()
        assert s1[0] - s0[0] == 1 and s1[1] - s0[1] == 1 and s1[3] >= 3
        for a, b in zip(base, got):
            np.testing.assert_array_equal(a, b)
        got2 = _host_chain_and_hmm(L, x, cs, refs, hmm)         # now x is recognised as well
        s2 = stats()
        assert s2[0] - s1[0] == 2 and s2[1] == s1[1]
        for a, b in zip(base, got2):
            np.testing.assert_array_equal(a, b)
        # identity is by content, not by address: a copy of x elsewhere in memory is recognised
        x2 = x.copy(order="F")
        ref2 = _host_chain_and_hmm(L, x2, cs, refs, hmm)
        s2b = stats()
        assert s2b[0] - s2[0] == 2 and s2b[1] == s2[1]
        s2 = s2b
        # run()'s stand-alone steps, each fed the previous step's result: only the first matrix is uploaded
        vp = lambda a: a.ctypes.data_as(ct.c_void_p)
        bufs = [np.empty_like(x, order="F") for _ in range(2)]
        cur = x
        for i, mask in enumerate((0x01, 0x02, 0x04, 0x08, 0x10, 0x20)):
            check(L.icnv_smooth_chain(vp(cur), vp(bufs[i & 1]), None, Cfg(G, C, cs, refs, stage_mask=mask).ptr()))
            cur = bufs[i & 1]
        s3 = stats()
        assert s3[0] - s2[0] == 6 and s3[1] == s2[1]
        assert np.abs(cur - base[1]).max() < 1e-12              # six steps == the fused chain's pre-denoise output
        # ONE element changed in place -- same address, same shape, a position the strided sample skips (the
        # sample takes every 47th value of this matrix) -- is noticed: uploaded again, the result follows the data
        assert (G * C) // 16384 == 47
        for pos, delta in (((1, 0), 0.5), ((G // 2 + 1, C // 2), 1e-9), ((0, 0), 0.25)):
            assert pos == (0, 0) or (pos[0] + G * pos[1]) % 47 != 0
            x2[pos] += delta
            s5 = stats()
            got3 = _host_chain_and_hmm(L, x2, cs, refs, hmm)
            assert stats()[1] - s5[1] == 1, pos                 # x2 uploaded; its outputs are new content as well
            want3 = oc.smooth_chain(x2, cs, refs, want_pre_denoise=True)[1]
            assert np.abs(got3[1] - want3).max() < 1e-12
            assert not np.array_equal(got3[1], ref2[1])
            ref2 = got3
    finally:
        check(L.icnv_residency(0))
    assert stats()[3] == 0


def test_in_library_multi_device_on_one_gpu(dev, tmp_path):
    """icnv_set_devices(n): one host thread per device, cells in contiguous blocks, the chain's reference statistics added on
    the host in device order.  Without an 8-GPU node the path runs with ICNV_FAKE_DEVICES=3 (three logical devices on this
    GPU, separate streams and pool partitions) in a child process and is compared with the one-device result: the
    chain within rounding of the differently ordered reference sums, the Viterbi -- same input -- bit for bit; with and
    without residency; an empty reference share on one device; an error raised on every device."""
    import inspect
    import subprocess
    import sys
    code = r'''
import ctypes as ct, os, sys
import numpy as np
sys.path.insert(0, %r)
from infercnv_amd import _lib, synth
from infercnv_amd._lib import Cfg, check
%s
L = _lib.load()
check(L.icnv_init(0))
G, C = 4000, 331
x, cs = synth.make_matrix_np(G, C); x = np.asfortranarray(x)
refs, _ = synth.groups(C)                      # reference cells first: all of them land on device 0
hmm = synth.hmm_params_i6()
check(L.icnv_set_devices(1))
one = _host_chain_and_hmm(L, x, cs, refs, hmm)
vals = one[1][:, np.concatenate(refs)]         # step 22's parameters from the pre-denoise matrix (R/inferCNV_ops.R:2311-2318)
mu_s = (vals.mean(), vals.std(axis=0, ddof=1).mean() * 1.5)
assert L.icnv_set_devices(4) != 0              # only 3 logical devices
for resident in (0, 1, 1):
    check(L.icnv_residency(resident))
    check(L.icnv_set_devices(0)); assert L.icnv_get_devices() == 3
    many = _host_chain_and_hmm(L, x, cs, refs, hmm)
    assert np.abs(many[1] - one[1]).max() < 1e-12, np.abs(many[1] - one[1]).max()
    d = np.abs(many[0] - one[0]) > 1e-10          # step 22 is a strict select: only an element sitting on a bound may differ
    lo_hi = np.array([mu_s[0] - mu_s[1], mu_s[0] + mu_s[1]])
    assert d.sum() <= 8 and (np.abs(one[1][d][:, None] - lo_hi[None, :]).min(axis=1) < 1e-10).all(), int(d.sum())
    # the Viterbi on ONE input: the three blocks together == the single device
    st3 = np.empty((G, C), dtype=np.uint8, order="F"); st1 = np.empty_like(st3)
    from infercnv_amd._lib import f64, i32
    m, mp = f64(hmm[0]); lp = np.asfortranarray(hmm[2]); ld, ldp = f64(hmm[3]); csa, csp = i32(cs)
    vp = lambda a: a.ctypes.data_as(ct.c_void_p)
    args = (G, C, csp, csa.size - 1, 6, mp, float(hmm[1]), lp.ctypes.data_as(ct.POINTER(ct.c_double)), ldp)
    check(L.icnv_viterbi_cells(vp(one[1]), vp(st3), *args))
    check(L.icnv_set_devices(1))
    check(L.icnv_viterbi_cells(vp(one[1]), vp(st1), *args))
    assert np.array_equal(st1, st3) and np.array_equal(st1, one[2])
check(L.icnv_residency(0))
# group HMM and median filter: whole groups / tiles per device (uneven groups, scattered cells, a cell in two groups --
# the later group wins --, cells in no group), identical to the one-device result
rng = np.random.default_rng(3)
perm = rng.permutation(C)
sizes = [60, 5, 41, 1, 33, 80, 17]
offs = np.concatenate([[0], np.cumsum(sizes)])
groups = [perm[offs[i]:offs[i + 1]].astype(np.int32) for i in range(len(sizes))]
groups_dup = groups[:-1] + [np.concatenate([groups[-1], groups[0][:3]]).astype(np.int32)]
from infercnv_amd._lib import pack_groups
def run_groups(gr):
    idx, off = pack_groups(gr); idx, ip = i32(idx); off, op = i32(off)
    sds, sdp = f64(np.linspace(0.06, 0.2, len(gr)))
    st = np.empty((G, C), dtype=np.uint8, order="F")
    check(L.icnv_viterbi_groups(vp(one[1]), vp(st), G, C, csp, csa.size - 1, ip, op, len(gr), 6, mp, sdp, lp.ctypes.data_as(ct.POINTER(ct.c_double)), ldp))
    return st
def run_median(gr):
    idx, off = pack_groups(gr); idx, ip = i32(idx); off, op = i32(off)
    o = np.empty_like(x)
    check(L.icnv_median_filter(vp(one[0]), vp(o), G, C, csp, csa.size - 1, ip, op, len(gr), 7))
    return o
check(L.icnv_set_devices(3)); g3, g3d, m3 = run_groups(groups), run_groups(groups_dup), run_median(groups)
check(L.icnv_set_devices(1)); g1, g1d, m1 = run_groups(groups), run_groups(groups_dup), run_median(groups)
assert np.array_equal(g3, g1) and np.array_equal(g3d, g1d) and np.array_equal(m3, m1)
assert (g1[:, perm[offs[-1]:]] == 255).all() and (g1[:, perm[:offs[-1]]] != 255).all()
assert np.array_equal(m1[:, perm[offs[-1]:]], one[0][:, perm[offs[-1]:]]) and not np.array_equal(m1, one[0])
# errors surface from the workers: an empty reference group, an even window
check(L.icnv_set_devices(3))
out = np.empty_like(x)
bad = Cfg(G, C, cs, [refs[0], np.zeros(0, dtype=np.int32)])
assert L.icnv_smooth_chain(vp(x), vp(out), None, bad.ptr()) == 1 and b"empty reference group" in L.icnv_last_error()
bad = Cfg(G, C, cs, refs, window_length=100)
assert L.icnv_smooth_chain(vp(x), vp(out), None, bad.ptr()) == 1
# fewer cells than devices
xs = np.asfortranarray(x[:, :2]); o2 = np.empty_like(xs)
check(L.icnv_smooth_chain(vp(xs), vp(o2), None, Cfg(G, 2, cs, [np.array([0], dtype=np.int32)], stage_mask=0x0F).ptr()))
check(L.icnv_set_devices(1)); o1 = np.empty_like(xs)
check(L.icnv_smooth_chain(vp(xs), vp(o1), None, Cfg(G, 2, cs, [np.array([0], dtype=np.int32)], stage_mask=0x0F).ptr()))
assert np.abs(o1 - o2).max() < 1e-12
print("MULTI_OK")
''' % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), inspect.getsource(_host_chain_and_hmm))
    env = dict(os.environ, ICNV_FAKE_DEVICES="3")
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "MULTI_OK" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]


@pytest.mark.parametrize("world,launch", [(2, "torchrun"), (3, "torchrun"), (2, "self"), (3, "self")])
def test_bench_two_ranks_equal_one_rank(dev, world, launch, tmp_path):
    """The N > 1 path of bench.py (one process per rank, torch.distributed, reference statistics all-reduced between the
    rounds) on the hardware at hand: 2 and 3 ranks on ONE GPU over gloo (ICNV_BENCH_ONE_DEVICE=1), cells dealt round-robin,
    against one rank holding all of them.  Both launch styles: under `python -m torch.distributed.run` (the driver's
    documented form) and as plain `python bench.py --gpus N` (bench.py starts its own ranks -- self_launch).  Compared
    ELEMENT BY ELEMENT per rank (bench.py --dump): every state call (0 mismatches), the per-cell sums of the HMM input
    (rounding of the rank-ordered reference sums only) and of the denoised matrix.  (RCCL on N GPUs needs a multi-GPU node:
    that is the driver's scaling run.)  At most 3 ranks and no memory-system microbenchmarks (ICNV_BENCH_NO_UBENCH: they
    only set the line's ceilings): with this process and the launcher, no more than 5 processes hold the GPU at once."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ICNV_BENCH_ONE_DEVICE="1", ICNV_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1", ICNV_BENCH_NO_UBENCH="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    per_rank = 24000 // world
    d_many, d_one = str(tmp_path / "many"), str(tmp_path / "one")
    common = ["--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--no-kernel-timing", "--checksum", str(world)]
    tail = [os.path.join(root, "bench.py"), "--gpus", str(world), "--cells", str(per_rank), "--dump", d_many] + common
    if launch == "torchrun":
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr",
               "127.0.0.1", "--master-port", str(29533 + world)] + tail
    else:
        cmd = [sys.executable] + tail                   # no launcher: bench.py re-executes itself under torch.distributed.run
    many = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=root)
    assert many.returncode == 0, many.stdout[-2000:] + many.stderr[-4000:]
    one = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--cells", str(per_rank * world), "--dump", d_one] + common,
                         env={k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")},
                         capture_output=True, text=True, timeout=900, cwd=root)
    assert one.returncode == 0, one.stdout[-2000:] + one.stderr[-4000:]
    lines = lambda r: [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines(many)) == 1, "exactly ONE JSON line from the N-rank run"
    a, b = json.loads(lines(many)[-1]), json.loads(lines(one)[-1])
    assert a["n_gpus"] == world and b["n_gpus"] == 1 and a["config"]["cells_total"] == b["config"]["cells_total"] == per_rank * world
    assert a["scaling"] == "weak" and a["config"]["cells_per_gpu"] == per_rank
    assert a["world"]["communicator_world_size"] == world and a["world"]["env_world_size"] == world
    assert a["world"]["cells_per_rank"] == [per_rank] * world and a["world"]["cells_sum"] == per_rank * world
    assert ("self_launch" in a["world"]["launcher"]) == (launch == "self")
    G = a["config"]["genes"]
    total_mismatch = 0
    for r in range(world):
        s2, s1 = np.load(os.path.join(d_many, f"states_{r}.npy")), np.load(os.path.join(d_one, f"states_{r}.npy"))
        assert s2.shape == s1.shape == (per_rank, G)
        total_mismatch += int((s2 != s1).sum())
        p2, p1 = np.load(os.path.join(d_many, f"pre_cellsums_{r}.npy")), np.load(os.path.join(d_one, f"pre_cellsums_{r}.npy"))
        # reference sums are added in rank order: rounding only (per CELL sum over 10 000 genes of values around 1)
        np.testing.assert_allclose(p2, p1, rtol=1e-12, atol=0)
        o2, o1 = np.load(os.path.join(d_many, f"out_cellsums_{r}.npy")), np.load(os.path.join(d_one, f"out_cellsums_{r}.npy"))
        # a denoise select within rounding of its bound may flip: such a cell's sum moves by at most the half width (~0.1);
        # every other cell agrees to rounding
        off = np.abs(o2 - o1) > 1e-9 * np.abs(o1)
        assert off.sum() <= 2 and (np.abs(o2 - o1)[off] < 0.5).all(), (int(off.sum()), np.abs(o2 - o1).max())
    assert total_mismatch == 0, f"{total_mismatch} state calls differ between {world} ranks and one rank"


def test_bench_collectives_over_rccl_with_one_rank(dev):
    """bench.py's N > 1 code path -- process group on the nccl (= RCCL) backend, barriers, the three all-reduces of the
    reference statistics on the library's own buffers, the all-reduce / all-gather of the timing and the checksums -- with
    ICNV_BENCH_FORCE_DIST=1 on a communicator of ONE rank: what a single-GPU box can run of it.  Same numbers as the plain
    one-rank run."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--gpus", "1", "--cells", "6000", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-kernel-timing", "--checksum", "1"]
    line = lambda r: json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    forced = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + common,
                            env=dict(os.environ, ICNV_BENCH_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29577"),
                            capture_output=True, text=True, timeout=600, cwd=root)
    assert forced.returncode == 0, forced.stdout[-2000:] + forced.stderr[-4000:]
    plain = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + common, env=dict(os.environ),
                           capture_output=True, text=True, timeout=600, cwd=root)
    assert plain.returncode == 0, plain.stdout[-2000:] + plain.stderr[-4000:]
    a, b = line(forced), line(plain)
    assert a["checksums"]["per_part"] == b["checksums"]["per_part"] and a["n_gpus"] == 1
    for c in ("4", "5"):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--config", c, "--genes", "4000"] + common[:-2],
                           env=dict(os.environ, ICNV_BENCH_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29578"),
                           capture_output=True, text=True, timeout=600, cwd=root)
        assert r.returncode == 0 and line(r)["n_gpus"] == 1, r.stdout[-2000:] + r.stderr[-4000:]


def test_bench_dump_outputs(dev, tmp_path):
    """bench.py --dump-outputs DIR: the last timed step's outputs (a fixed sample of whole cells) as float .npy files under
    64 MB -- the same files from two runs with the same arguments, the same values as the full per-cell dump (--dump) of
    those cells; `steps` and `ms_per_step` in the line.  Config 5 dumps its filtered matrix."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ICNV_BENCH_NO_UBENCH="1")
    common = ["--gpus", "1", "--cells", "3000", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-kernel-timing"]
    line = lambda r: json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    runs = []
    for i, extra in enumerate((["--checksum", "1", "--dump", str(tmp_path / "full")], [])):
        d = tmp_path / f"out{i}"
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + common + extra + ["--dump-outputs", str(d)],
                           env=env, capture_output=True, text=True, timeout=600, cwd=root)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        res = line(r)
        assert res["steps"] == 3 and res["ms_per_step"] > 0
        files = {f: np.load(d / f) for f in os.listdir(d)}
        assert sorted(files) == ["denoised.npy", "hmm_input.npy", "sample_cells.npy", "states.npy"] == res["dump_outputs"]["files"]
        assert sum(a.nbytes for a in files.values()) <= 64 << 20
        assert files["denoised.npy"].dtype == files["hmm_input.npy"].dtype == np.float64 and files["states.npy"].dtype == np.float32
        runs.append(files)
    for f in runs[0]:
        np.testing.assert_array_equal(runs[0][f], runs[1][f])
    cells = runs[0]["sample_cells.npy"].astype(np.int64)
    assert len(cells) > 0 and runs[0]["states.npy"].shape == (len(cells), res["config"]["genes"])
    full = tmp_path / "full"
    np.testing.assert_array_equal(runs[0]["states.npy"], np.load(full / "states_0.npy")[cells].astype(np.float32))
    np.testing.assert_allclose(runs[0]["hmm_input.npy"].sum(axis=1), np.load(full / "pre_cellsums_0.npy")[cells], rtol=1e-12)
    np.testing.assert_allclose(runs[0]["denoised.npy"].sum(axis=1), np.load(full / "out_cellsums_0.npy")[cells], rtol=1e-12)
    d5 = tmp_path / "out5"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--config", "5", "--genes", "4000", "--no-side-legs"] + common
                       + ["--dump-outputs", str(d5)], env=env, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    filt = np.load(d5 / "filtered.npy")
    assert filt.dtype == np.float64 and filt.shape == (len(np.load(d5 / "sample_cells.npy")), 4000) and np.isfinite(filt).all()


def test_i6_whole_samples_without_cluster_by_groups_is_one_sample_per_observation_cell(dev):
    """predict_CNV_via_HMM_on_whole_tumor_samples(cluster_by_groups = FALSE): the reference's
    `c(all_observations = unlist(obs), reference_grouped_cell_indices)` (R/inferCNV_HMM.R:532) is a list with one element
    per observation CELL (c() of a vector with a list), so each of them is decoded on its own profile with the sd the
    fit predicts for num_cells = 1, the reference groups on their mean profiles with their own sd."""
    from infercnv_amd import GeneOrder, InfercnvObject, hmm, synth
    G, C = 2000, 60
    x, cs = synth.make_matrix_np(G, C)
    refs, obs = synth.groups(C)
    _, pre, _ = oc.smooth_chain(x, cs, refs, want_pre_denoise=True)
    obj = InfercnvObject(expr_data=pre, gene_order=GeneOrder(chr=np.repeat(np.arange(22), np.diff(cs)).astype(str)),
                         reference_grouped_cell_indices={"r0": refs[0], "r1": refs[1]},
                         observation_grouped_cell_indices={f"t{q}": obs[q] for q in range(4)})
    means, _, logPi, logDelta = synth.hmm_params_i6()
    cnv = {k: {"mean": m, "sd": 0.2} for k, m in zip(hmm.CNV_LEVELS, means)}
    fit = {k: (np.log(0.3) + 0.01 * i, -0.45) for i, k in enumerate(hmm.CNV_LEVELS)}      # log(sd) = b0 + b1 log(n)
    got = hmm.predict_CNV_via_HMM_on_whole_tumor_samples(obj, False, cnv, fit).expr_data
    sd_of = lambda n: float(onp.r_median(np.array([np.exp(b0 + b1 * np.log(n)) for b0, b1 in fit.values()])))
    obs_cells = np.concatenate(obs)
    want_cells, _ = oc.viterbi_cells(pre[:, obs_cells], cs, means, sd_of(1), logPi, logDelta)
    np.testing.assert_array_equal(got[:, obs_cells], want_cells)
    want_refs, _ = oc.viterbi_groups(pre, cs, list(refs), means, [sd_of(len(r)) for r in refs], logPi, logDelta)
    ref_cells = np.concatenate(refs)
    np.testing.assert_array_equal(got[:, ref_cells], want_refs[:, ref_cells])


def test_r_shim_driven_from_c(dev):
    """The R .Call shim (rglue/src/icnv_shim.c) compiled against the mock R API and driven from C on the GPU: smooth chain
    (+ pre-denoise matrix, dimnames), per-cell and group Viterbi, median filter, proxy tables (K = 3 leaves 4..6
    untouched), average bounds -- every result identical to the direct C-ABI call, PROTECT balance zero, the library's
    error for an even window raised through Rf_error (rglue/mock/test_shim.c)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mock = os.path.join(root, "rglue", "mock")
    res = subprocess.run(["make", "-C", mock, "all"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    res = subprocess.run([os.path.join(mock, "test_shim"), "gpu"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "SHIM_GPU_OK" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]


@pytest.mark.parametrize("config", [4, 5])
def test_bench_group_configs_two_ranks_equal_one_rank(dev, config):
    """BASELINE configs 4 (i3 HMM at subcluster level) and 5 (median filter) through bench.py --config: two ranks on ONE GPU
    over gloo, whole subclusters / tiles per rank (sharded.align_to_groups), the i3 (mu, sigma) from two all-reduces of
    two doubles -- against one rank holding all the cells: the sums of the state calls / of the filtered matrix over the
    same global cells.  (RCCL on N GPUs is the driver's scaling run.)"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ICNV_BENCH_ONE_DEVICE="1", ICNV_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    common = ["--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--no-kernel-timing", "--config", str(config), "--genes", "4000"]
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                          "127.0.0.1", "--master-port", str(29541 + config), os.path.join(root, "bench.py"), "--gpus", "2", "--cells", "10000"] + common,
                         env=env, capture_output=True, text=True, timeout=900, cwd=root)
    assert two.returncode == 0, two.stdout[-2000:] + two.stderr[-4000:]
    one = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--cells", "20000"] + common,
                         env=dict(os.environ), capture_output=True, text=True, timeout=900, cwd=root)
    assert one.returncode == 0, one.stdout[-2000:] + one.stderr[-4000:]
    line = lambda r: json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    a, b = line(two), line(one)
    assert a["n_gpus"] == 2 and b["n_gpus"] == 1 and a["config"]["cells_total"] == b["config"]["cells_total"] == 20000
    s2, s1 = sum(a["checksums"]["per_rank"]), sum(b["checksums"]["per_rank"])
    assert len(a["checksums"]["per_rank"]) == 2 and min(a["checksums"]["per_rank"]) > 0
    if config == 4:
        assert abs(s2 - s1) <= 50, (s2, s1)              # state calls: identical but for a decision within 1e-16 of a tie
        assert s1 > 2 * 4000 * 20000 * 0.9               # i3 states 1..3, most of them neutral (2)
    else:
        assert abs(s2 - s1) <= 1e-9 * abs(s1), (s2, s1)  # the reference sums are added in another order: rounding only


def test_ingest_from_integer_counts_equals_the_step_functions(dev, run_inputs, golden_dir):
    """steps 2, 3, 4 of run() in ONE call from integer counts uploaded once -- dense int32 and CSC --
    against the four step functions (gene filters, depth normalisation, log2(x + 1)) on the f64 copy: kept genes, the
    normalisation factor and every value bit for bit; bytes crossing PCIe reported.  (a) the reference's golden object
    (@count.data, int32) replayed to @expr.data; (b) example/run.R's matrix rounded to counts (9 939 x 184, 59 % zeros)
    with run()'s filters (cutoff = 1, min_cells_per_gene = 3, R/inferCNV_ops.R:560-566)."""
    import scipy.sparse as sp
    from infercnv_amd import GeneOrder, InfercnvObject, ops
    # (a) golden object
    d = np.load(os.path.join(golden_dir, "infercnv_object_example.npz"))
    counts = d["count_data"].astype(np.int64)
    levels = d["chr_levels"][d["chr_codes"]]
    mk = lambda m: InfercnvObject(expr_data=m, gene_order=GeneOrder(chr=levels),
                                  reference_grouped_cell_indices={"normal": d["ref_normal"]},
                                  observation_grouped_cell_indices={"tumor": d["obs_tumor"]})
    o4, up = ops.ingest_counts(mk(counts))
    assert up == counts.size * 4 and o4.expr_data.shape == counts.shape
    want = onp.log2xplus1(onp.normalize_counts_by_seq_depth(counts.astype(np.float64)))
    assert np.abs(o4.expr_data - want).max() < 1e-12
    final = ops.hip_smooth_chain(o4)
    assert np.abs(final.expr_data - d["expr_data"]).max() < 1e-10          # @count.data -> @expr.data, the reference's own pair
    # (b) run()'s step 2-4 on a count matrix with real sparsity
    x = np.rint(run_inputs["counts"])
    obj = InfercnvObject(expr_data=x, count_data=x, gene_order=GeneOrder(chr=run_inputs["chr"]),
                         reference_grouped_cell_indices=run_inputs["refs"], observation_grouped_cell_indices=run_inputs["obs"])
    o = ops.require_above_min_mean_expr_cutoff(obj, 1)
    o = ops.require_above_min_cells_ref(o, 3)
    steps = ops.log2xplus1(ops.normalize_counts_by_seq_depth(o))
    dense, up_dense = ops.ingest_counts(obj, 1, 3)
    csc, up_csc = ops.ingest_counts(InfercnvObject(expr_data=sp.csc_matrix(x), gene_order=obj.gene_order,
                                                  reference_grouped_cell_indices=run_inputs["refs"],
                                                  observation_grouped_cell_indices=run_inputs["obs"]), 1, 3)
    for got in (dense, csc):
        assert got.expr_data.shape == steps.expr_data.shape and 3000 < got.expr_data.shape[0] < x.shape[0]
        np.testing.assert_array_equal(got.expr_data, steps.expr_data)
        np.testing.assert_array_equal(np.asarray(got.gene_order.chr), np.asarray(steps.gene_order.chr))
    nnz = int((x != 0).sum())
    assert up_dense == x.size * 4 and up_csc == (x.shape[1] + 1) * 8 + nnz * 8
    print(f"[ingest] H2D bytes: f64 matrix {x.size * 8}, int32 dense {up_dense}, CSC {up_csc} ({nnz} stored entries)")
    # every gene removed is the reference's stop(998)
    with pytest.raises(Exception, match="All genes removed"):
        ops.ingest_counts(obj, 1e9, 0)
    # a negative entry is not a count (R's NA_integer_ is INT_MIN): refused, dense and CSC
    bad = x.copy()
    bad[17, 3] = -2147483648
    for m in (bad, sp.csc_matrix(bad)):
        with pytest.raises(Exception, match="negative value in the count matrix"):
            ops.ingest_counts(InfercnvObject(expr_data=m, gene_order=obj.gene_order, reference_grouped_cell_indices=run_inputs["refs"],
                                             observation_grouped_cell_indices=run_inputs["obs"]), 1, 3)
    # a cell without a single count over the kept genes: R gives 0 / 0 * factor = NaN for every gene of it -- dense and CSC alike
    empty = x.copy()
    empty[:, 5] = 0
    mk = lambda m: InfercnvObject(expr_data=m, gene_order=obj.gene_order, reference_grouped_cell_indices=run_inputs["refs"],
                                  observation_grouped_cell_indices=run_inputs["obs"])
    e_dense, _ = ops.ingest_counts(mk(empty), 1, 3, sparse=False)
    e_csc, _ = ops.ingest_counts(mk(sp.csc_matrix(empty)), 1, 3)
    assert np.isnan(e_dense.expr_data[:, 5]).all() and np.isnan(e_csc.expr_data[:, 5]).all()
    np.testing.assert_array_equal(e_dense.expr_data, e_csc.expr_data)
    # a colptr that is not non-decreasing is refused on the host (the kernels would walk out of the arrays)
    import ctypes as ct
    from infercnv_amd import _lib
    m = sp.csc_matrix(x)
    colptr = np.ascontiguousarray(m.indptr, dtype=np.int64).copy()
    colptr[3], colptr[4] = colptr[4] + 7, colptr[3]
    rowidx, vals = np.ascontiguousarray(m.indices, dtype=np.int32), np.ascontiguousarray(m.data, dtype=np.int32)
    cnt = _lib.Counts(None, colptr.ctypes.data, rowidx.ctypes.data, vals.ctypes.data, int(vals.size))
    keep_buf = np.empty(x.shape[0], dtype=np.int32)
    n_, used_, up_ = ct.c_int64(), ct.c_double(), ct.c_int64()
    out_buf = np.empty(x.shape, dtype=np.float64, order="F")
    rc = _lib.load().icnv_ingest_counts(ct.byref(cnt), x.shape[0], x.shape[1], 1.0, 3, float("nan"), keep_buf.ctypes.data_as(ct.POINTER(ct.c_int32)),
                                        ct.byref(n_), out_buf.ctypes.data_as(ct.c_void_p), ct.byref(used_), ct.byref(up_))
    assert rc != 0 and b"colptr" in _lib.load().icnv_last_error()
    # device-resident flavour, explicit factor, no filters
    t = torch.from_numpy(np.ascontiguousarray(x.T.astype(np.int32))).cuda()
    e, keep, used = dev.ingest_counts(dev.DeviceCounts(x.shape[0], x.shape[1], dense=t), normalize_factor=1e5)
    assert used == 1e5 and keep.size == x.shape[0]
    cs = x.sum(axis=0)
    nz = cs > 0
    assert np.abs(to_host(e)[:, nz] - np.log2(x[:, nz] / cs[nz] * 1e5 + 1.0)).max() < 1e-11


def test_hspike_sd_trend_resampling_fit_vs_oracle(dev):
    """SURVEY.md 8f #3, second half: get_hspike_cnv_mean_sd_trend_by_num_cells_fit (R/inferCNV_HMM.R:154-212) -- the
    sample() draws are R's stream (set.seed(seed); tests/test_oracle.py pins it), the sampled residuals are gathered from
    the hidden-spike matrix on the device, sd / lm on the host -- against the oracle's scalar restatement: the sd of every
    (level, ncells), NA for ncells = 1, intercept and slope of the six regressions.  A hidden spike-in with the reference's
    eleven fake chromosomes (.get_hspike_chr_info), levels with one and with six chromosomes."""
    from infercnv_amd import GeneOrder, InfercnvObject, hmm
    rng = np.random.default_rng(12)
    sizes = [40, 33, 51, 37, 46, 35, 42, 39, 44, 31, 48]
    chr_names = np.concatenate([[name] * n for (name, _), n in zip(hmm.HSPIKE_CHR_INFO, sizes)])
    G, C = chr_names.size, 70
    level_of = {name: cnv for name, cnv in hmm.HSPIKE_CHR_INFO}
    x = np.stack([rng.normal(level_of[c] if level_of[c] > 0.02 else 0.05, 0.15 + 0.05 * level_of[c], size=C) for c in chr_names])
    spike = {"spike_a": np.arange(20, 45, dtype=np.int32), "spike_b": np.array([69, 3, 50, 51, 7], dtype=np.int32)}
    hs = InfercnvObject(expr_data=x, gene_order=GeneOrder(chr=chr_names),
                        reference_grouped_cell_indices={"normal": np.arange(0, 3, dtype=np.int32)},
                        observation_grouped_cell_indices=spike)
    import inspect
    sig = inspect.signature(hmm.get_hspike_cnv_mean_sd_trend_by_num_cells_fit)
    assert sig.parameters["nrounds"].default == 100 and sig.parameters["max_cells"].default == 100    # the reference's constants
    got = hmm.get_hspike_cnv_mean_sd_trend_by_num_cells_fit(hs, seed=2024, max_cells=30)
    cells = np.concatenate(list(spike.values()))
    ev = {}
    for name, cnv in hmm.HSPIKE_CHR_INFO:                       # .get_gene_expr_by_cnv (:45-68)
        key = "cnv:%g" % cnv
        block = x[np.nonzero(chr_names == name)[0]][:, cells].ravel(order="F")
        ev[key] = np.concatenate([ev[key], block]) if key in ev else block
    assert list(ev) == ["cnv:1", "cnv:0.01", "cnv:0.5", "cnv:1.5", "cnv:2", "cnv:3"]
    want = onp.hspike_sd_trend_fit(ev, 2024, max_cells=30)
    for level in ev:
        sds, (b0, b1) = want[level]
        assert np.isnan(got["_sd"][level][0]) and np.isnan(sds[0])
        assert np.abs(got["_sd"][level][1:] - sds[1:]).max() < 1e-14
        assert abs(got[level][0] - b0) < 1e-11 and abs(got[level][1] - b1) < 1e-11
        # every sd estimates sigma / sqrt(nrounds): the slope is ~0 (the reference's rowMeans runs over the rounds)
        assert abs(got[level][1]) < 0.6 and 0.4 < np.exp(got[level][0]) / (np.std(ev[level]) / 10.0) < 2.5
    # the fit feeds .get_state_emission_params (R/inferCNV_HMM.R:586-614) as before
    assert hmm._group_sd(25, {k: {"mean": 1.0, "sd": 0.2} for k in hmm.CNV_LEVELS}, {k: got[k] for k in hmm.CNV_LEVELS}) > 0
