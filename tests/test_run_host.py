"""run() without a GPU: its signature against R's formals, the argument checks (they come before the library is loaded and
before anything is written), the file-name tokens of steps 17-20 and the gate of steps 18-19 against a restatement of R's
`length(unique(apply(states, 2, unique))) != 1`."""
import inspect
import itertools
import json
import logging
import os

import numpy as np
import pytest

import infercnv_amd
from infercnv_amd import GeneOrder, InfercnvObject, _lib, pipeline, run


@pytest.fixture
def tiny():
    return InfercnvObject(expr_data=np.ones((4, 3)), gene_order=GeneOrder(chr=np.array(["chr1"] * 4)),
                          reference_grouped_cell_indices={"n": np.array([0])}, observation_grouped_cell_indices={"t": np.array([1, 2])})


@pytest.fixture
def no_library(monkeypatch):
    """The argument checks must not reach the library."""
    def refuse():
        raise AssertionError("run() loaded the library before its argument checks were through")
    monkeypatch.setattr(_lib, "load", refuse)


def test_run_is_the_function_and_is_exported():
    assert infercnv_amd.run is pipeline.run and inspect.isfunction(infercnv_amd.run)
    assert "run" in infercnv_amd.__all__


def test_signature_matches_r_formals(golden_dir):
    want = json.load(open(os.path.join(golden_dir, "run_formals.json")))["run"]
    params = list(inspect.signature(run).parameters.values())
    positional = [p for p in params if p.kind == p.POSITIONAL_OR_KEYWORD]
    assert [p.name for p in positional] == [n.replace(".", "_") for n in want["formals"]]
    assert [p.default is not p.empty for p in positional] == want["has_default"]
    rest = params[len(positional):]
    assert [(p.name, p.kind) for p in rest] == [("seed", inspect.Parameter.KEYWORD_ONLY), ("on_step", inspect.Parameter.KEYWORD_ONLY)]
    assert rest[0].default == 0 and rest[1].default is None
    # R's defaults where a user meets them first; a match.arg vector defaults to its first element
    d = {p.name: p.default for p in positional}
    assert (d["cutoff"], d["min_cells_per_gene"], d["window_length"], d["sd_amplifier"], d["BayesMaxPNormal"]) == (1, 3, 101, 1.5, 0.5)
    assert (d["smooth_method"], d["HMM_type"], d["HMM_report_by"], d["analysis_mode"]) == ("pyramidinal", "i6", "subcluster", "subclusters")
    assert (d["tumor_subcluster_partition_method"], d["leiden_method"], d["leiden_function"]) == ("leiden", "PCA", "CPM")
    assert (d["leiden_method_per_chr"], d["leiden_function_per_chr"], d["up_to_step"]) == ("simple", "modularity", 100)
    assert d["out_dir"] is None and d["noise_filter"] is None and d["num_ref_groups"] is None and d["HMM_i3_use_KS"] is False


@pytest.mark.parametrize("kwargs,message", [
    (dict(out_dir=None), "out_dir is NULL"),                                                             # R/inferCNV_ops.R:389-392
    (dict(HMM=True, HMM_type="i6", smooth_method="coordinates"), "Incompatible HMM mode and smoothing method."),   # :353-356
])
def test_r_stops_raise_value_error(tiny, no_library, tmp_path, kwargs, message):
    out = tmp_path / "out"
    with pytest.raises(ValueError, match=message):
        run(tiny, **{"out_dir": str(out), **kwargs})
    assert not out.exists()


@pytest.mark.parametrize("kwargs,names", [
    (dict(tumor_subcluster_partition_method="qnorm"), "tumor_subcluster_partition_method"),
    (dict(tumor_subcluster_partition_method="pheight"), "tumor_subcluster_partition_method"),
    (dict(tumor_subcluster_partition_method="qgamma"), "tumor_subcluster_partition_method"),
    (dict(tumor_subcluster_partition_method="shc"), "tumor_subcluster_partition_method"),
    (dict(sim_method="simple"), "sim_method"),
    (dict(sim_method="splatter"), "sim_method"),
    (dict(sim_foreground=True), "sim_foreground"),
    (dict(plot_chr_scale=True), "plot_chr_scale"),
    (dict(write_phylo=True), "write_phylo"),
    (dict(output_format="pdf"), "output_format"),
    (dict(test_use="perm", mask_nonDE_genes=True), "test_use"),
])
def test_unsupported_options_raise_not_implemented(tiny, no_library, tmp_path, kwargs, names):
    out = tmp_path / "out"
    with pytest.raises(NotImplementedError, match=names):
        run(tiny, out_dir=str(out), **kwargs)
    assert not out.exists()


def test_perm_without_the_mask_is_not_refused(tiny, tmp_path, monkeypatch):
    """test_use = "perm" is only read by step 21: without mask_nonDE_genes the checks pass and run() goes on to the library."""
    class Reached(Exception):
        pass

    def reached():
        raise Reached()
    monkeypatch.setattr(_lib, "load", reached)
    with pytest.raises(Reached):
        run(tiny, out_dir=str(tmp_path / "out"), test_use="perm")
    assert not (tmp_path / "out").exists()


def _defaults(**over):
    a = {p.name: p.default for p in inspect.signature(run).parameters.values()
         if p.kind == p.POSITIONAL_OR_KEYWORD and p.name != "infercnv_obj"}
    a["out_dir"] = "out"
    a.update(over)
    return a


def test_r_adjustments(caplog):
    caplog.set_level(logging.INFO, logger="infercnv_amd")
    a = pipeline.check_arguments(_defaults(smooth_method="coordinates", window_length=101))           # :357-362
    assert a["window_length"] == 10000000 and "window_length" in caplog.text
    assert pipeline.check_arguments(_defaults(smooth_method="coordinates", window_length=20000))["window_length"] == 20000
    caplog.clear()
    a = pipeline.check_arguments(_defaults(analysis_mode="cells"))                                     # :368-372
    assert a["HMM_report_by"] == "cell" and "HMM_report_by" in caplog.text
    a = pipeline.check_arguments(_defaults(per_chr_hmm_subclusters=True, tumor_subcluster_partition_method="random_trees"))   # :376-378
    assert a["per_chr_hmm_subclusters"] is False
    assert pipeline.check_arguments(_defaults(per_chr_hmm_subclusters=True))["per_chr_hmm_subclusters"] is True
    a = pipeline.check_arguments(_defaults(max_centered_threshold=float("nan"), noise_filter=float("nan")))   # NA is None
    assert a["max_centered_threshold"] is None and a["noise_filter"] is None
    with pytest.raises(ValueError, match="should be one of"):                                          # match.arg
        pipeline.check_arguments(_defaults(smooth_method="median"))


def test_ignored_options_log_one_line_each(caplog):
    caplog.set_level(logging.INFO, logger="infercnv_amd")
    pipeline.check_arguments(_defaults())
    assert "ignored" not in caplog.text
    over = dict(num_threads=8, debug=True, useRaster=False, diagnostics=True, plot_probabilities=False, save_rds=False,
                save_final_rds=False, resume_mode=False)
    pipeline.check_arguments(_defaults(**over))
    lines = [r.getMessage() for r in caplog.records if "ignored" in r.getMessage()]
    assert len(lines) == len(over)
    for name in over:
        assert sum(name + " =" in ln for ln in lines) == 1


def test_file_tokens_on_r_literal_cases():
    tok = pipeline.file_tokens
    assert tok(False, "i6", "subclusters", "leiden")["resume_file_token"] == ".leiden"      # ifelse(HMM, ..., "") (:583), then :1069
    assert tok(False, "i6", "samples", "leiden")["resume_file_token"] == ""                  # no HMM: ""
    assert tok(True, "i6", "samples", "leiden")["hmm_resume_file_token"] == "HMMi6.hmm_mode-samples"
    assert tok(True, "i6", "subclusters", "leiden")["hmm_resume_file_token"] == "HMMi6.leiden.hmm_mode-subclusters"
    # random_trees: step 7's condition (:716, `== 'random_trees'`) appends ".rand_trees" (:720); step 15's condition
    # (:1067, `!= 'random_trees'`) excludes it, so :1069 appends nothing
    assert tok(True, "i3", "subclusters", "random_trees")["hmm_resume_file_token"] == "HMMi3.rand_trees.hmm_mode-subclusters"
    # modes other than subclusters append neither
    assert tok(True, "i3", "cells", "random_trees")["hmm_resume_file_token"] == "HMMi3.hmm_mode-cells"
    t = tok(True, "i6", "samples", "leiden", 0.5)
    assert t["hmm_prefix"] == "17_HMM_predHMMi6.hmm_mode-samples"                            # :1314
    assert t["bayes_prefix"] == "HMM_CNV_predictions.HMMi6.hmm_mode-samples.Pnorm_0.5"       # :1451
    assert t["bayes_dir"] == "BayesNetOutput.HMMi6.hmm_mode-samples"                         # :1374
    assert tok(True, "i6", "samples", "leiden", 0.25)["bayes_prefix"].endswith(".Pnorm_0.25")
    assert tok(True, "i6", "samples", "leiden", 1)["bayes_prefix"].endswith(".Pnorm_1")      # C's %g


# ---- the gate of steps 18-19, restated from R's semantics -------------------------------------------------------------
def _r_unique(values):
    """unique(): the distinct elements in order of first appearance."""
    out = []
    for v in values:
        if v not in out:
            out.append(v)
    return out


def _r_apply_cols_unique(m):
    """apply(m, 2, unique): a vector when every call returns one value, a matrix (one column per call) when all calls return
    the same number > 1 of values, a list otherwise."""
    cols = [_r_unique(m[:, j].tolist()) for j in range(m.shape[1])]
    lens = {len(c) for c in cols}
    if lens == {1}:
        return "vector", [c[0] for c in cols]
    if len(lens) == 1:
        return "matrix", [[c[i] for c in cols] for i in range(lens.pop())]          # rows of the k x ncol matrix
    return "list", cols


def _r_length_unique(kind, v):
    """length(unique(v)): distinct entries of a vector; for a matrix unique() drops duplicated rows and length() counts the
    elements of what is left; for a list the distinct elements."""
    if kind == "vector":
        return len(_r_unique(v))
    if kind == "matrix":
        rows = _r_unique([tuple(r) for r in v])
        return len(rows) * len(rows[0])
    return len(_r_unique([tuple(c) for c in v]))


def _r_gate(m):
    return _r_length_unique(*_r_apply_cols_unique(m)) != 1


@pytest.mark.parametrize("shape", [(3, 2), (2, 3), (1, 1), (2, 1), (3, 1)])
def test_gate_against_restatement_exhaustively(shape):
    n = shape[0] * shape[1]
    kinds = set()
    for values in itertools.product((1, 2, 3), repeat=n):
        m = np.array(values, dtype=np.float64).reshape(shape)
        kinds.add(_r_apply_cols_unique(m)[0])
        assert pipeline.states_not_constant(m) == _r_gate(m), m
    assert "vector" in kinds and (shape[0] == 1 or "matrix" in kinds)
    if shape == (3, 2):
        assert "list" in kinds


# ---- the order of the steps and their guards, with every stage replaced by a recorder ----------------------------------
@pytest.fixture
def stages(monkeypatch):
    """Every stage run() calls, replaced by a stub that records its name (and keyword arguments) and passes the object on:
    what is left is run()'s own logic -- order, guards, up_to_step, which object goes where."""
    from infercnv_amd import bayes_net, cnv_regions, heatmap, hidden_spike, hmm, mask_non_de, ops, tumor_subclusters
    calls = []

    def stub(module, name, result=lambda o, a, k: o.copy()):
        def fn(obj, *args, **kwargs):
            calls.append((name, args, kwargs))
            return result(obj, args, kwargs)
        monkeypatch.setattr(module, name, fn)

    monkeypatch.setattr(_lib, "load", lambda: None)
    for name in ("require_above_min_mean_expr_cutoff", "require_above_min_cells_ref", "normalize_counts_by_seq_depth", "log2xplus1",
                 "scale_infercnv_expr", "split_references", "subtract_ref_expr_from_obs", "apply_max_threshold_bounds",
                 "smooth_by_chromosome", "smooth_by_chromosome_runmeans", "smooth_by_chromosome_coordinates",
                 "center_cell_expr_across_chromosome", "remove_genes_at_ends_of_chromosomes", "invert_log2", "remove_outliers_norm",
                 "clear_noise", "clear_noise_via_ref_mean_sd", "hip_smooth_chain"):
        stub(ops, name)
    stub(ops, "ingest_counts", lambda o, a, k: (o.copy(), 0))

    def with_hspike(o, a, k):
        o = o.copy()
        o.hspike = o.copy()
        return o
    stub(hidden_spike, "build_and_add_hspike", with_hspike)

    def with_subclusters(o):
        o = o.copy()
        o.tumor_subclusters = {"hc": {}, "subclusters": {}}
        return o
    stub(tumor_subclusters, "define_signif_tumor_subclusters_via_random_smooothed_trees", lambda o, a, k: with_subclusters(o))
    stub(tumor_subclusters, "define_signif_tumor_subclusters", lambda o, a, k: (with_subclusters(o), {"chr1": {}}))
    stub(tumor_subclusters, "redo_hierarchical_clustering")
    stub(hmm, "get_spike_dists", lambda o, a, k: {"cnv:1": {"mean": 1.0, "sd": 0.1}})
    stub(hmm, "get_hspike_cnv_mean_sd_trend_by_num_cells_fit", lambda o, a, k: {"fit": True})

    def states(o, a, k):
        o = o.copy()
        o.expr_data = np.array([[3.0, 3.0, 4.0]] * 4)
        return o
    for name in ("predict_CNV_via_HMM_on_indiv_cells", "predict_CNV_via_HMM_on_tumor_subclusters",
                 "predict_CNV_via_HMM_on_tumor_subclusters_per_chr", "predict_CNV_via_HMM_on_whole_tumor_samples",
                 "i3HMM_predict_CNV_via_HMM_on_indiv_cells", "i3HMM_predict_CNV_via_HMM_on_tumor_subclusters",
                 "i3HMM_predict_CNV_via_HMM_on_whole_tumor_samples"):
        stub(hmm, name, states)
    stub(hmm, "assign_HMM_states_to_proxy_expr_vals")
    stub(hmm, "i3HMM_assign_HMM_states_to_proxy_expr_vals")
    stub(cnv_regions, "generate_cnv_region_reports", lambda o, a, k: [])
    stub(cnv_regions, "adjust_genes_regions_report", lambda o, a, k: None)
    stub(bayes_net, "inferCNVBayesNet", lambda o, a, k: "mcmc")
    stub(bayes_net, "filterHighPNormals", lambda o, a, k: ("filtered", np.full((4, 3), 3.0)))
    stub(mask_non_de, "mask_non_DE_genes_basic")
    stub(heatmap, "plot_cnv", lambda o, a, k: {})
    return calls


def _names(calls):
    return [c[0] for c in calls]


CHAIN_STEPWISE = ["subtract_ref_expr_from_obs", "apply_max_threshold_bounds", "smooth_by_chromosome", "center_cell_expr_across_chromosome",
                  "subtract_ref_expr_from_obs", "invert_log2"]


def test_default_run_takes_the_fused_entries(tiny, stages, tmp_path):
    tiny.expr_data = np.ones((4, 3), dtype=np.int32)
    got = run(tiny, out_dir=str(tmp_path / "out"))
    assert (tmp_path / "out").is_dir()
    assert _names(stages) == ["ingest_counts", "hip_smooth_chain", "define_signif_tumor_subclusters", "plot_cnv", "plot_cnv"]
    assert stages[1][2]["denoise"] is False and stages[1][2]["smooth_method"] == "pyramidinal"
    assert stages[2][2]["partition_method"] == "leiden" and stages[2][2]["leiden_method"] == "PCA" and stages[2][2]["seed"] == 0
    prelim, final = stages[3][2], stages[4][2]
    assert (prelim["title"], prelim["output_filename"]) == ("Preliminary infercnv (pre-noise filtering)", "infercnv.preliminary")
    assert (final["title"], final["output_filename"], final["x_center"], final["x_range"]) == ("inferCNV", "infercnv", 1, "auto")
    assert got.options["window_length"] == 101 and got.options["HMM_type"] == "i6" and tiny.options == {}


def test_non_integer_counts_and_observers_take_the_step_functions(tiny, stages, tmp_path):
    tiny.expr_data = np.full((4, 3), 0.5)
    run(tiny, out_dir=str(tmp_path), no_plot=True, up_to_step=14)                    # the fused ingest wants integer counts
    ingest = ["require_above_min_mean_expr_cutoff", "require_above_min_cells_ref", "normalize_counts_by_seq_depth", "log2xplus1"]
    assert _names(stages) == ingest + ["hip_smooth_chain"]
    del stages[:]
    seen = []
    tiny.expr_data = np.ones((4, 3), dtype=np.int32)
    run(tiny, out_dir=str(tmp_path), no_plot=True, up_to_step=14, on_step=lambda s, label, o: seen.append(s))
    assert _names(stages) == ingest + CHAIN_STEPWISE
    assert seen == [1, 2, 3, 4, 8, 9, 10, 11, 12, 14]
    del stages[:]
    run(tiny, out_dir=str(tmp_path), no_plot=True, up_to_step=12)                    # up_to_step inside the block: stepwise
    assert _names(stages) == ["ingest_counts"] + CHAIN_STEPWISE[:5]
    del stages[:]
    run(tiny, out_dir=str(tmp_path), no_plot=True, up_to_step=14, remove_genes_at_chr_ends=True, max_centered_threshold=None)
    assert _names(stages) == ["ingest_counts"] + CHAIN_STEPWISE[:1] + CHAIN_STEPWISE[2:5] + ["remove_genes_at_ends_of_chromosomes", "invert_log2"]


@pytest.mark.parametrize("k,last", [(0, None), (1, None), (2, "require_above_min_cells_ref"), (3, "normalize_counts_by_seq_depth"),
                                    (4, "log2xplus1"), (7, "log2xplus1"), (8, "subtract_ref_expr_from_obs"), (10, "smooth_by_chromosome"),
                                    (13, "subtract_ref_expr_from_obs"), (15, "define_signif_tumor_subclusters"),
                                    (21, "define_signif_tumor_subclusters"), (22, "clear_noise_via_ref_mean_sd")])
def test_up_to_step_returns_where_r_returns(tiny, stages, tmp_path, k, last):
    seen = []
    run(tiny, out_dir=str(tmp_path), no_plot=True, denoise=True, up_to_step=k, on_step=lambda s, label, o: seen.append(s))
    assert (_names(stages)[-1] if stages else None) == last
    assert seen == [s for s in (1, 2, 3, 4, 8, 9, 10, 11, 12, 14, 15, 22) if s <= k]


def test_hmm_route_i6_samples_with_the_bayesian_filter(tiny, stages, tmp_path):
    seen = {}
    got = run(tiny, out_dir=str(tmp_path), HMM=True, analysis_mode="samples", denoise=True, sd_amplifier=2, no_plot=True, seed=7,
              on_step=lambda s, label, o: seen.__setitem__(s, o))
    names = _names(stages)
    assert names.index("build_and_add_hspike") == names.index("normalize_counts_by_seq_depth") + 1          # step 3, before the log
    tail = names[names.index("define_signif_tumor_subclusters"):]
    assert tail == ["define_signif_tumor_subclusters", "get_spike_dists", "get_hspike_cnv_mean_sd_trend_by_num_cells_fit",
                    "predict_CNV_via_HMM_on_whole_tumor_samples", "generate_cnv_region_reports", "inferCNVBayesNet",
                    "filterHighPNormals", "adjust_genes_regions_report", "assign_HMM_states_to_proxy_expr_vals",
                    "clear_noise_via_ref_mean_sd"]
    by = {c[0]: c for c in stages}
    assert by["define_signif_tumor_subclusters"][2]["partition_method"] == "none"
    assert by["build_and_add_hspike"][2]["seed"] == 7 and by["get_hspike_cnv_mean_sd_trend_by_num_cells_fit"][2]["seed"] == 7
    assert by["inferCNVBayesNet"][2]["seed"] == 7 and by["inferCNVBayesNet"][2]["by"] == "subcluster"
    assert by["inferCNVBayesNet"][2]["out_dir"] == os.path.join(str(tmp_path), "BayesNetOutput.HMMi6.hmm_mode-samples")
    assert by["generate_cnv_region_reports"][1][:2] == ("17_HMM_predHMMi6.hmm_mode-samples", str(tmp_path))
    assert by["generate_cnv_region_reports"][2] == {"ignore_neutral_state": 3, "by": "subcluster"}
    assert by["adjust_genes_regions_report"][2]["input_filename_prefix"] == "17_HMM_predHMMi6.hmm_mode-samples"
    assert by["adjust_genes_regions_report"][2]["output_filename_prefix"] == "HMM_CNV_predictions.HMMi6.hmm_mode-samples.Pnorm_0.5"
    assert by["clear_noise_via_ref_mean_sd"][2]["sd_amplifier"] == 2
    # what on_step receives: the infercnv object, the HMM object for 17, 19, 20, the MCMC object for 18; run() returns R's
    assert seen[18] == "mcmc" and seen[17].expr_data[0, 2] == 4 and (seen[19].expr_data == 3).all() and got is seen[22]
    assert got.expr_data is not seen[20].expr_data and (got.expr_data == 1).all()


def test_constant_states_close_the_gate(tiny, stages, tmp_path, monkeypatch):
    from infercnv_amd import hmm

    def flat(obj, *a, **k):
        o = obj.copy()
        o.expr_data = np.full((4, 3), 3.0)
        return o
    monkeypatch.setattr(hmm, "predict_CNV_via_HMM_on_whole_tumor_samples", flat)
    seen = []
    run(tiny, out_dir=str(tmp_path), HMM=True, analysis_mode="samples", no_plot=True, on_step=lambda s, label, o: seen.append(s))
    assert "inferCNVBayesNet" not in _names(stages) and "filterHighPNormals" not in _names(stages)
    assert 17 in seen and 20 in seen and 18 not in seen and 19 not in seen


@pytest.mark.parametrize("mode,method,hmm_type,per_chr,predictor", [
    ("subclusters", "leiden", "i6", False, "predict_CNV_via_HMM_on_tumor_subclusters"),
    ("subclusters", "leiden", "i6", True, "predict_CNV_via_HMM_on_tumor_subclusters_per_chr"),
    ("subclusters", "random_trees", "i6", True, "predict_CNV_via_HMM_on_tumor_subclusters"),     # per_chr switched off (:376-378)
    ("subclusters", "random_trees", "i3", False, "i3HMM_predict_CNV_via_HMM_on_tumor_subclusters"),
    ("cells", "leiden", "i6", False, "predict_CNV_via_HMM_on_indiv_cells"),
    ("cells", "leiden", "i3", False, "i3HMM_predict_CNV_via_HMM_on_indiv_cells"),
    ("samples", "leiden", "i6", False, "predict_CNV_via_HMM_on_whole_tumor_samples"),
    ("samples", "leiden", "i3", False, "i3HMM_predict_CNV_via_HMM_on_whole_tumor_samples"),
    ("subclusters", "leiden", "i3", False, "i3HMM_predict_CNV_via_HMM_on_tumor_subclusters"),
])
def test_the_nine_predictors_of_step_17(tiny, stages, tmp_path, mode, method, hmm_type, per_chr, predictor):
    seen = []
    run(tiny, out_dir=str(tmp_path), HMM=True, HMM_type=hmm_type, analysis_mode=mode, tumor_subcluster_partition_method=method,
        per_chr_hmm_subclusters=per_chr, BayesMaxPNormal=0, no_plot=True, on_step=lambda s, label, o: seen.append(s))
    names = _names(stages)
    predictors = [n for n in names if "predict_CNV" in n]
    assert predictors == [predictor]
    fits = names.count("get_hspike_cnv_mean_sd_trend_by_num_cells_fit")
    assert fits == (1 if hmm_type == "i6" and mode != "cells" else 0)                # once, only for a group-level i6 predictor
    assert ("redo_hierarchical_clustering" in names) == (mode == "subclusters" and method == "random_trees")
    assert (7 in seen) == (mode == "subclusters" and method == "random_trees")
    assert (15 in seen) == (not (mode == "subclusters" and method == "random_trees"))
    assert 18 not in seen and 19 not in seen and "inferCNVBayesNet" not in names     # BayesMaxPNormal = 0
    by = {c[0]: c for c in stages}
    token = pipeline.file_tokens(True, hmm_type, mode, method, 0)["hmm_prefix"]
    assert by["generate_cnv_region_reports"][1][0] == token
    assert by["generate_cnv_region_reports"][2]["by"] == ("cell" if mode == "cells" else "subcluster")
    assert by["generate_cnv_region_reports"][2]["ignore_neutral_state"] == (3 if hmm_type == "i6" else 2)
    if predictor.endswith("per_chr"):
        assert by[predictor][1][0] == {"chr1": {}}                                   # step 15's subclusters_per_chr, kept


def test_optional_steps_and_plots(tiny, stages, tmp_path):
    seen = []
    run(tiny, out_dir=str(tmp_path), scale_data=True, num_ref_groups=2, prune_outliers=True, mask_nonDE_genes=True, denoise=True,
        noise_filter=0.2, smooth_method="runmeans", plot_steps=True, HMM=True, HMM_type="i3", analysis_mode="samples",
        BayesMaxPNormal=0, on_step=lambda s, label, o: seen.append(s))
    assert seen == [1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 14, 15, 16, 17, 20, 21, 22]
    names = _names(stages)
    assert "smooth_by_chromosome_runmeans" in names and "smooth_by_chromosome" not in names
    assert "clear_noise" in names and "clear_noise_via_ref_mean_sd" not in names
    by = {c[0]: c for c in stages}
    assert by["split_references"][2] == {"num_groups": 2, "hclust_method": "ward.D2"}
    plots = [(c[2]["title"], c[2]["output_filename"], c[2].get("x_center"), c[2].get("x_range")) for c in stages if c[0] == "plot_cnv"]
    assert plots == [
        ("04_log_transformed_data", "infercnv.04_log_transformed", None, None),
        ("05_scaled", "infercnv.05_scaled", None, None),
        ("08_remove_average", "infercnv.08_remove_average", None, None),
        ("09_apply_max_centered_expr_threshold", "infercnv.09_apply_max_centred_expr_threshold", None, None),
        ("10_smoothed_by_chr", "infercnv.10_smoothed_by_chr", None, None),
        ("11_centering_of_smoothed", "infercnv.11_centering_of_smoothed", None, None),
        ("12_remove_average", "infercnv.12_remove_average", None, None),
        ("14_invert_log_transform log(FC)->FC", "infercnv.14_invert_log_FC", None, None),
        ("Preliminary infercnv (pre-noise filtering)", "infercnv.preliminary", None, None),
        ("16_removed_outliers", "infercnv.16_removed_outliers", None, None),
        ("17_HMM_preds", "infercnv.17_HMM_predHMMi3.hmm_mode-samples", 2, (1, 3)),
        ("20_HMM_preds.repr_intensities", "infercnv.20_HMM_predHMMi3.hmm_mode-samples.Pnorm_0.repr_intensities", 1, (-1, 3)),
        ("21_mask_nonDE", "infercnv.21_mask_nonDE", None, None),
        ("22_denoised", "infercnv.22_denoised", None, None),
        ("inferCNV", "infercnv", 1, "auto"),
    ]
    del stages[:]
    run(tiny, out_dir=str(tmp_path), no_prelim_plot=True, final_scale_limits=(0.5, 1.5), final_center_val=1.0)
    plots = [(c[2]["output_filename"], c[2]["x_center"], c[2]["x_range"]) for c in stages if c[0] == "plot_cnv"]
    assert plots == [("infercnv", 1.0, (0.5, 1.5))]


def test_sparse_counts(tiny, stages, tmp_path, caplog):
    sp = pytest.importorskip("scipy.sparse")
    caplog.set_level(logging.INFO, logger="infercnv_amd")
    tiny.expr_data = sp.csc_matrix(np.ones((4, 3), dtype=np.int32))
    run(tiny, out_dir=str(tmp_path), no_plot=True, up_to_step=4)
    assert _names(stages) == ["ingest_counts"] and "densifies" not in caplog.text    # the fused ingest takes it as it is
    del stages[:]
    first = []
    run(tiny, out_dir=str(tmp_path), no_plot=True, up_to_step=2, on_step=lambda s, label, o: first.append(o))
    assert "densifies" in caplog.text and isinstance(first[0].expr_data, np.ndarray) and sp.issparse(tiny.expr_data)
