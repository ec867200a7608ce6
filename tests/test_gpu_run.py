"""run() on the GPU (-m gpu): the reference's own run() result as a pin, the fused and the stepwise route against each other,
up_to_step, the HMM / Bayes route and both subclusterings on example/run.R's 184 cells against compositions written out by
hand here, the plots' files, and the options that must reach their step."""
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


class Hook:
    """on_step recorder: step -> (label, object); every step function returns a new object, so references suffice."""

    def __init__(self):
        self.seen = {}
        self.order = []

    def __call__(self, step, label, obj):
        assert step not in self.seen, f"step {step} reported twice"
        self.seen[step] = obj
        self.order.append(step)

    def __getitem__(self, step):
        return self.seen[step]


# ---- the reference's 20-cell example object ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def example(golden_dir):
    d = np.load(os.path.join(golden_dir, "infercnv_object_example.npz"))
    ex = {k: d[k] for k in d.files}
    log = onp.log2xplus1(onp.normalize_counts_by_seq_depth(ex["count_data"]))
    ex["oracle"] = oc.smooth_chain(log, oc.chr_starts_from_codes(ex["chr_codes"]), [ex["ref_normal"]], want_pre_denoise=True)
    return ex


def example_obj(ex):
    from infercnv_amd import GeneOrder, InfercnvObject
    chr_names = ex["chr_levels"][ex["chr_codes"] - ex["chr_codes"].min()]
    return InfercnvObject(expr_data=ex["count_data"].copy(), count_data=ex["count_data"].copy(),
                          gene_order=GeneOrder(chr_names, ex["gene_start"], ex["gene_stop"]),
                          reference_grouped_cell_indices={"normal": ex["ref_normal"]},
                          observation_grouped_cell_indices={"tumor": ex["obs_tumor"]})


EXAMPLE_CALL = dict(cutoff=1, cluster_by_groups=True, denoise=True, HMM=False, no_plot=True)
PLOT_FILES = ("infercnv.preliminary.heatmap_thresholds.txt", "infercnv.heatmap_thresholds.txt", "infercnv.observation_groupings.txt",
              "infercnv.observations.txt", "infercnv.references.txt")


@pytest.fixture(scope="module")
def fused_run(dev, example, tmp_path_factory):
    """The example call without a hook: the fused route."""
    from infercnv_amd import run
    out = tmp_path_factory.mktemp("fused")
    return run(example_obj(example), out_dir=str(out), **EXAMPLE_CALL), out


@pytest.fixture(scope="module")
def stepwise_run(dev, example, tmp_path_factory):
    """The same call with a hook: the stepwise route, every step's object recorded."""
    from infercnv_amd import run
    hook = Hook()
    out = tmp_path_factory.mktemp("stepwise")
    return run(example_obj(example), out_dir=str(out), on_step=hook, **EXAMPLE_CALL), hook, out


def test_a_reference_held_pin(example, fused_run):
    """A: data/infercnv_object_example.rda is the reference's own run() result: its @count.data through run() gives its
    @expr.data (the strict select of step 22 flips nowhere) and its tumor_subclusters' cells."""
    got, out = fused_run
    assert got.expr_data.shape == (4613, 20)            # cutoff 1 drops 0 of 4 613 genes, min_cells_per_gene = 3 keeps all
    _, ref_pre, (mu, s) = example["oracle"]
    check_denoise_flips(got.expr_data, example["expr_data"], ref_pre, mu, s, tol=1e-11, expect=0, label="run() vs @expr.data")
    subs = got.tumor_subclusters["subclusters"]
    assert set(subs) == {"tumor", "normal"} and set(got.tumor_subclusters["hc"]) == {"tumor", "normal"}
    gold = dict(zip((str(n).split("/")[0] for n in example["subcluster_names"]), (example["subcluster_0"], example["subcluster_1"])))
    for g in ("tumor", "normal"):
        assert len(subs[g]) == 1                         # 10 cells <= k_nn = 20: the single-tree branch
        cells = np.concatenate([np.asarray(v) for v in subs[g].values()])
        assert cells.size == 10 and set(cells.tolist()) == set(gold[g].tolist())
    assert got.options["cutoff"] == 1 and got.options["smooth_method"] == "pyramidinal" and got.options["denoise"] is True
    assert not any(os.path.exists(os.path.join(out, f)) for f in PLOT_FILES)       # no_plot


def test_b_both_routes_agree(example, fused_run, stepwise_run, tmp_path):
    """B: fused (no hook) against stepwise (hook) within the bound test_config1 holds for fused against stand-alone."""
    from infercnv_amd import run
    fused14 = run(example_obj(example), out_dir=str(tmp_path), up_to_step=14, **EXAMPLE_CALL)   # still the fused chain
    step_final, hook, _ = stepwise_run
    a, b = fused14.expr_data, hook[14].expr_data
    print(f"[routes] step 14: max |fused - stepwise| = {np.abs(a - b).max():.3e}, bit-equal: {np.array_equal(a, b)}")
    assert np.abs(a - b).max() <= 1e-11
    _, ref_pre, (mu, s) = example["oracle"]
    check_denoise_flips(step_final.expr_data, fused_run[0].expr_data, ref_pre, mu, s, tol=1e-11, label="stepwise vs fused run()")
    print(f"[routes] final: bit-equal: {np.array_equal(step_final.expr_data, fused_run[0].expr_data)}")
    assert hook.order == [1, 2, 3, 4, 8, 9, 10, 11, 12, 14, 15, 22]              # R's guards: 5-7, 13, 16-21 did not run


@pytest.mark.parametrize("k", [4, 12, 14, 15])
def test_c_up_to_step(example, stepwise_run, tmp_path, k):
    """C: up_to_step = k returns what the full run's hook saw at step k, and runs nothing beyond it."""
    from infercnv_amd import run
    _, full, _ = stepwise_run
    hook = Hook()
    got = run(example_obj(example), out_dir=str(tmp_path), up_to_step=k, on_step=hook, **EXAMPLE_CALL)
    assert max(hook.order) == k and hook.order == [s for s in full.order if s <= k]
    np.testing.assert_array_equal(got.expr_data, full[k].expr_data)
    assert got is hook[k]
    if k == 15:
        for g, subs in full[15].tumor_subclusters["subclusters"].items():
            for name, cells in subs.items():
                np.testing.assert_array_equal(got.tumor_subclusters["subclusters"][g][name], cells)
    else:
        assert got.tumor_subclusters is None


def test_f_plots_and_matrix_files(dev, example, tmp_path):
    """F: plot_cnv is called where R calls it: the preliminary and the final plot's files; the final plot is
    plot_cnv(returned object, x.center = 1, x.range = "auto")."""
    from infercnv_amd import heatmap, run
    out, again = tmp_path / "run", tmp_path / "again"
    got = run(example_obj(example), out_dir=str(out), **{**EXAMPLE_CALL, "no_plot": False}, write_expr_matrix=True)
    for f in PLOT_FILES:
        assert (out / f).exists(), f
    heatmap.plot_cnv(got, out_dir=str(again), title="inferCNV", output_filename="infercnv", x_center=1, x_range="auto",
                     write_expr_matrix=True, cluster_by_groups=True, cluster_references=True, k_obs_groups=1)
    assert (out / "infercnv.observations.txt").read_bytes() == (again / "infercnv.observations.txt").read_bytes()
    assert not (out / "infercnv.17_HMM_pred.hmm_mode-subclusters.heatmap_thresholds.txt").exists()    # HMM off: no HMM plot


def test_g_runmeans_reaches_step_10(dev, example, tmp_path):
    from infercnv_amd import ops, run
    step4 = run(example_obj(example), out_dir=str(tmp_path), up_to_step=4, **EXAMPLE_CALL)
    got = run(example_obj(example), out_dir=str(tmp_path), up_to_step=14, smooth_method="runmeans", **EXAMPLE_CALL)
    want = ops.hip_smooth_chain(step4, smooth_method="runmeans", denoise=False)
    np.testing.assert_array_equal(got.expr_data, want.expr_data)
    plain = ops.hip_smooth_chain(step4, denoise=False)
    assert not np.array_equal(got.expr_data, plain.expr_data)


def test_g_num_ref_groups_reaches_step_6(dev, example, tmp_path):
    from infercnv_amd import heatmap, run, tumor_subclusters
    hook = Hook()
    got = run(example_obj(example), out_dir=str(tmp_path), up_to_step=6, num_ref_groups=2, on_step=hook, **EXAMPLE_CALL)
    assert hook.order == [1, 2, 3, 4, 6]
    groups = got.reference_grouped_cell_indices
    assert list(groups) == ["refgrp-1", "refgrp-2"]
    ref = np.asarray(example["ref_normal"], dtype=np.int64)
    assert sorted(np.concatenate(list(groups.values())).tolist()) == sorted(ref.tolist())
    labels = heatmap.cutree_k(tumor_subclusters.hclust(hook[4], ref, "ward.D2").merge, 2)     # run()'s hclust_method default
    first = list(dict.fromkeys(labels.tolist()))
    for name, lab in zip(groups, first):
        np.testing.assert_array_equal(groups[name], np.sort(ref[labels == lab]))
        assert groups[name].size >= 1


def test_g_remove_genes_at_chr_ends_reaches_step_13(dev, example, tmp_path):
    from infercnv_amd import ops, run
    hook = Hook()
    got = run(example_obj(example), out_dir=str(tmp_path), remove_genes_at_chr_ends=True, window_length=11, on_step=hook,
              **EXAMPLE_CALL)
    assert hook[12].expr_data.shape[0] == 4613
    by_hand = ops.remove_genes_at_ends_of_chromosomes(hook[12], 11)
    assert hook[13].expr_data.shape[0] < hook[12].expr_data.shape[0]
    assert hook[13].expr_data.shape[0] == by_hand.expr_data.shape[0]
    assert got.expr_data.shape[0] == hook[13].expr_data.shape[0] == len(got.gene_order.chr)


# ---- example/run.R's 184 cells ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run_inputs(golden_dir):
    d = np.load(os.path.join(golden_dir, "example_run_inputs.npz"))
    x = d["mant"].astype(np.float64) / 10.0 ** d["neg_exp"].astype(np.float64)
    refs = {str(n): d[f"ref_{i}"] for i, n in enumerate(d["ref_names"])}
    obs = {str(n): d[f"obs_{i}"] for i, n in enumerate(d["obs_names"])}
    return {"counts": x, "chr": d["chr_levels"][d["chr_codes"]], "refs": refs, "obs": obs}


def inputs_obj(ri):
    from infercnv_amd import GeneOrder, InfercnvObject
    return InfercnvObject(expr_data=ri["counts"], count_data=ri["counts"], gene_order=GeneOrder(chr=ri["chr"]),
                          reference_grouped_cell_indices=ri["refs"], observation_grouped_cell_indices=ri["obs"])


D_TOKEN = "HMMi6.hmm_mode-samples"
D_REPORTS = tuple(f"17_HMM_pred{D_TOKEN}.{s}" for s in ("cell_groupings", "pred_cnv_regions.dat", "pred_cnv_genes.dat", "genes_used.dat"))
D_BAYES = tuple(f"HMM_CNV_predictions.{D_TOKEN}.Pnorm_0.5.{s}" for s in ("pred_cnv_regions.dat", "pred_cnv_genes.dat"))


@pytest.fixture(scope="module")
def hmm_run(dev, run_inputs, tmp_path_factory):
    """D's run: BASELINE configs[0] (cutoff 1, denoise, sd_amplifier 2, HMM i6) on whole samples with the Bayesian filter."""
    from infercnv_amd import run
    hook = Hook()
    out = tmp_path_factory.mktemp("hmm")
    got = run(inputs_obj(run_inputs), cutoff=1, out_dir=str(out), HMM=True, HMM_type="i6", analysis_mode="samples", denoise=True,
              sd_amplifier=2, BayesMaxPNormal=0.5, no_plot=True, seed=7, on_step=hook)
    return got, hook, out


@pytest.fixture(scope="module")
def hmm_by_hand(dev, run_inputs):
    """D's composition: the same stages called one by one, the chain through the fused entry."""
    from infercnv_amd import hidden_spike, hmm, ops, tumor_subclusters
    o = ops.require_above_min_cells_ref(ops.require_above_min_mean_expr_cutoff(inputs_obj(run_inputs), 1), 3)
    o = hidden_spike.build_and_add_hspike(ops.normalize_counts_by_seq_depth(o), seed=7)
    o = ops.log2xplus1(o)
    _, hmm_in = ops.hip_smooth_chain(o, sd_amplifier=2, return_hmm_input=True)
    # step 15 of the samples mode: one subcluster per group, which names the report's cell groups; the matrix is untouched
    hmm_in = tumor_subclusters.define_signif_tumor_subclusters(hmm_in, partition_method="none", per_chr_hmm_subclusters=False,
                                                               seed=7)[0]
    cnv_mean_sd = hmm.get_spike_dists(hmm_in.hspike)
    fit = hmm.get_hspike_cnv_mean_sd_trend_by_num_cells_fit(hmm_in.hspike, seed=7)
    states = hmm.predict_CNV_via_HMM_on_whole_tumor_samples(hmm_in, True, cnv_mean_sd, fit, 1e-6)
    return hmm_in, states


def test_d_hmm_states_and_reports(run_inputs, hmm_run, hmm_by_hand, tmp_path):
    from infercnv_amd import cnv_regions, ops
    got, hook, out = hmm_run
    st = hook[17].expr_data
    assert st.min() >= 1 and st.max() <= 6 and len(np.unique(st)) >= 4
    # the known biology of this data set: oligodendroglioma = 1p / 19q co-deletion in the malignant cells
    chr_of = np.asarray(hook[17].gene_order.chr)
    mal = np.concatenate(list(run_inputs["obs"].values()))
    ref = np.concatenate(list(run_inputs["refs"].values()))
    for arm_chr in ("chr1", "chr19"):
        rows = chr_of == arm_chr
        assert (st[np.ix_(rows, mal)] < 3).mean() > 0.3
        assert (st[np.ix_(rows, ref)] == 3).mean() > 0.9
    hmm_in, want = hmm_by_hand
    print(f"[D] step-16 object vs fused chain: max |diff| = {np.abs(hook[15].expr_data - hmm_in.expr_data).max():.3e}")
    np.testing.assert_array_equal(st, want.expr_data)
    cnv_regions.generate_cnv_region_reports(want, f"17_HMM_pred{D_TOKEN}", str(tmp_path), ignore_neutral_state=3, by="subcluster")
    for f in D_REPORTS:
        assert (out / f).exists(), f
        assert (out / f).read_bytes() == (tmp_path / f).read_bytes(), f
    # the returned object is the denoised infercnv object, not the states
    assert got is hook[22] and got.expr_data.shape == st.shape and not np.array_equal(got.expr_data, st)
    np.testing.assert_array_equal(got.expr_data, ops.clear_noise_via_ref_mean_sd(hook[15], 2).expr_data)


def test_d_bayes_filter_and_proxy(hmm_run, hmm_by_hand, tmp_path):
    from infercnv_amd import bayes_net, cnv_regions, hmm
    got, hook, out = hmm_run
    hmm_in, states = hmm_by_hand
    assert hook.order == [1, 2, 3, 4, 8, 9, 10, 11, 12, 14, 15, 17, 18, 19, 20, 22]
    cnv_regions.generate_cnv_region_reports(states, f"17_HMM_pred{D_TOKEN}", str(tmp_path), ignore_neutral_state=3, by="subcluster")
    mcmc = bayes_net.inferCNVBayesNet(hmm_in, states.expr_data, HMM_type="i6", by="subcluster", seed=7)
    assert isinstance(hook[18], bayes_net.MCMCInferCNV) and hook[18].cnv_regions == mcmc.cnv_regions and len(mcmc.cnv_regions) > 0
    np.testing.assert_array_equal(hook[18].cnv_means, mcmc.cnv_means)
    filtered, kept = bayes_net.filterHighPNormals(mcmc, states.expr_data, 0.5)
    np.testing.assert_array_equal(hook[19].expr_data, kept)
    cnv_regions.adjust_genes_regions_report(filtered, f"17_HMM_pred{D_TOKEN}", f"HMM_CNV_predictions.{D_TOKEN}.Pnorm_0.5", str(tmp_path))
    for f in D_BAYES:
        assert (out / f).exists(), f
        assert (out / f).read_bytes() == (tmp_path / f).read_bytes(), f
    proxy = states.copy()
    proxy.expr_data = kept
    np.testing.assert_array_equal(hook[20].expr_data, hmm.assign_HMM_states_to_proxy_expr_vals(proxy).expr_data)


@pytest.mark.parametrize("method", ["leiden", "random_trees"])
def test_e_subcluster_routes(dev, run_inputs, tmp_path, method):
    """E: the i3 HMM on tumor subclusters, by Leiden (step 15) and by random trees (step 7); no Bayesian filter."""
    from infercnv_amd import pipeline, run
    hook = Hook()
    obj = inputs_obj(run_inputs)
    run(obj, cutoff=1, out_dir=str(tmp_path), HMM=True, HMM_type="i3", analysis_mode="subclusters",
        tumor_subcluster_partition_method=method, leiden_method="simple", k_nn=10, BayesMaxPNormal=0, no_plot=True, seed=7,
        on_step=hook)
    at, other = (15, 7) if method == "leiden" else (7, 15)
    assert at in hook.order and other not in hook.order
    assert hook[at].tumor_subclusters is not None and (at == 7 or hook[14].tumor_subclusters is None)
    assert 18 not in hook.order and 19 not in hook.order and 17 in hook.order and 20 in hook.order
    subs = hook[17].tumor_subclusters["subclusters"]
    st = hook[17].expr_data
    assert st.min() >= 1 and st.max() <= 3
    for g, cells in run_inputs["obs"].items():
        got = np.concatenate([np.asarray(v).ravel() for v in subs[g].values()])
        assert got.size == len(cells) and sorted(got.tolist()) == sorted(np.asarray(cells).tolist())     # a partition
    for g in subs:
        for name, cells in subs[g].items():
            cells = np.asarray(cells).ravel()
            assert (st[:, cells] == st[:, cells[:1]]).all(), (g, name)
    if method == "random_trees":                          # .redo_hierarchical_clustering: one tree over each group's sorted cells
        names = hook[17].cells()
        for g in subs:
            cells = np.sort(np.concatenate([np.asarray(v).ravel() for v in subs[g].values()]))
            hc = hook[17].tumor_subclusters["hc"][g]
            assert sorted(hc.order.tolist()) == list(range(1, cells.size + 1)) and hc.merge.shape == (cells.size - 1, 2)
            assert list(hc.labels) == list(names[cells])
    token = {"leiden": "HMMi3.leiden.hmm_mode-subclusters", "random_trees": "HMMi3.rand_trees.hmm_mode-subclusters"}[method]
    assert pipeline.file_tokens(True, "i3", "subclusters", method, 0)["hmm_resume_file_token"] == token
    for s in ("cell_groupings", "pred_cnv_regions.dat", "pred_cnv_genes.dat", "genes_used.dat"):
        assert (tmp_path / f"17_HMM_pred{token}.{s}").exists(), s
    assert not [f for f in os.listdir(tmp_path) if f.startswith("BayesNetOutput") or f.startswith("HMM_CNV_predictions")]
