"""run(): the whole pipeline from an infercnv object to CNV calls -- the mirror of `infercnv::run`
(R/inferCNV_ops.R:242-1652), exported as `infercnv_amd.run`.

run() adds no arithmetic of its own: every one of R's 22 steps calls the step function that mirrors it (ops, hidden_spike,
tumor_subclusters, hmm, cnv_regions, bayes_net, mask_non_de, heatmap), each a thin call into libicnv_hip.so.  What lives here
is what R's run() alone wrote down: the order, the guards, `up_to_step`, which object each stage reads, and the file-name
tokens through which steps 17-20 find each other's files (`file_tokens`, `states_not_constant`).

Not mirrored: resume (`resume_mode`), `plot_subclusters`, and the options the library does not build (they raise
NotImplementedError before anything runs).  run() itself draws none of the Bayes plots (`plot_probabilities` and `diagnostics`
are accepted and ignored) and serialises nothing (`save_rds`, `save_final_rds` likewise); `on_step` is the hook for all three:
`bayes_probabilities_hook` writes the probability heatmaps and the tables under plotProbabilities' PDFs (DESIGN K33),
`mcmc_diagnostics_hook` the table under the diagnostic plots (DESIGN K31), and `rds_checkpoints` R's serialised step objects
under R's file names (DESIGN K27).
"""
from __future__ import annotations

import logging
import math
import os

import numpy as np

from .infercnv_object import DeviceMatrix, InfercnvObject

log = logging.getLogger("infercnv_amd")

SMOOTH_METHODS = ("pyramidinal", "runmeans", "coordinates")
HMM_REPORT_BY = ("subcluster", "consensus", "cell")
HMM_TYPES = ("i6", "i3")
ANALYSIS_MODES = ("subclusters", "samples", "cells")
PARTITION_METHODS = ("leiden", "random_trees", "qnorm", "pheight", "qgamma", "shc")
LEIDEN_METHODS = ("PCA", "simple")
LEIDEN_FUNCTIONS = ("CPM", "modularity")

# accepted for signature parity and otherwise ignored: name -> R's default
IGNORED_OPTIONS = {"num_threads": 4, "debug": False, "useRaster": True, "diagnostics": False, "plot_probabilities": True,
                   "save_rds": True, "save_final_rds": True, "resume_mode": True}


def _is_na(v):
    return v is None or (isinstance(v, float) and math.isnan(v))


def _match_arg(name, value, choices):
    """match.arg: the whole vector (R's default) or None selects the first element; else one of the choices."""
    if value is None or (isinstance(value, (tuple, list)) and tuple(value) == tuple(choices)):
        return choices[0]
    if value not in choices:
        raise ValueError(f"{name}: 'arg' should be one of " + ", ".join(f"'{c}'" for c in choices))
    return value


def file_tokens(HMM=False, HMM_type="i6", analysis_mode="subclusters", tumor_subcluster_partition_method="leiden",
                BayesMaxPNormal=0.5):
    """The file-name tokens of run()'s steps 17-20, a pure function of five arguments:

      resume_file_token      "HMM" + HMM_type if HMM else ""                                        (R/inferCNV_ops.R:583)
                             + ".rand_trees" where step 7 runs: subclusters and random_trees         (:716-720)
                             + "." + partition method where step 15's first branch runs: subclusters
                               and NOT random_trees                                                  (:1067-1069)
      hmm_resume_file_token  resume_file_token + ".hmm_mode-" + analysis_mode                        (:1236)
      hmm_prefix             "%02d_HMM_pred%s" % (17, hmm_resume_file_token)                         (:1314, :1450)
      bayes_dir              "BayesNetOutput." + hmm_resume_file_token                               (:1374)
      bayes_prefix           "HMM_CNV_predictions.%s.Pnorm_%g"                                       (:1451; C's %g)
    """
    token = "HMM" + HMM_type if HMM else ""
    if analysis_mode == "subclusters" and tumor_subcluster_partition_method == "random_trees":
        token += ".rand_trees"
    if analysis_mode == "subclusters" and tumor_subcluster_partition_method != "random_trees":
        token += "." + tumor_subcluster_partition_method
    hmm_token = token + ".hmm_mode-" + analysis_mode
    return {"resume_file_token": token, "hmm_resume_file_token": hmm_token, "hmm_prefix": "%02d_HMM_pred%s" % (17, hmm_token),
            "bayes_dir": "BayesNetOutput.%s" % hmm_token,
            "bayes_prefix": "HMM_CNV_predictions.%s.Pnorm_%g" % (hmm_token, BayesMaxPNormal)}


def states_not_constant(states) -> bool:
    """The gate of steps 18 and 19, `length(unique(apply(states, 2, unique))) != 1` (R/inferCNV_ops.R:1364, :1407).

    `apply(states, 2, unique)` takes the distinct values of every cell's column, and what it returns depends on their counts:
      - every cell has ONE state: a vector with one entry per cell; `unique` of it holds the distinct states, so its length is
        1 exactly when all cells share that state;
      - all cells have the same number k > 1 of states: a k x cells matrix; `unique` drops duplicated ROWS and keeps a matrix
        of at least one row and `cells` columns whose `length` is rows * cells -- with one cell its k rows are distinct
        (length k > 1), with more cells the length is at least 2;
      - otherwise: a list with one entry per cell; the entries differ in length, so `unique` keeps at least two.
    Only the first case can give 1, and it does when the whole matrix holds a single value: the gate is "the state matrix is
    not constant"."""
    if isinstance(states, DeviceMatrix):   # a resident state matrix (DESIGN K32): one comparison on the device, one flag back
        t = states.tensor.reshape(-1)
        return True if t.numel() == 0 else bool((t != t[0]).any())
    s = np.asarray(states)
    if s.size == 0:
        return True           # length(unique(list())) is 0, and 0 != 1
    return bool((s != s.ravel()[0]).any())


def _r_chr(v):
    """sprintf("%s", v) of a scalar run() argument: NA for None, TRUE / FALSE, a number as as.character prints it."""
    if v is None or (isinstance(v, float) and math.isnan(v)):
        return "NA"
    if isinstance(v, (bool, np.bool_)):
        return "TRUE" if v else "FALSE"
    if isinstance(v, (float, np.floating)):
        return "%.15g" % v
    return str(v)


def checkpoint_file_names(**run_args):
    """{step: file name} of the objects infercnv::run saves with save_rds (expected_file_names of .get_relevant_args_list,
    R/inferCNV_ops.R:3316-3492, with R's own sprintf patterns), for the run() arguments given (the others at their defaults).
    Steps R gives no file for these arguments are absent; step 18 is R's .mcmc_obj."""
    a = {"HMM": False, "HMM_type": "i6", "analysis_mode": "subclusters", "tumor_subcluster_partition_method": "leiden",
         "BayesMaxPNormal": 0.5, "num_ref_groups": None, "max_centered_threshold": 3, "remove_genes_at_chr_ends": False,
         "prune_outliers": False, "mask_nonDE_genes": False, "denoise": False, "noise_filter": None, "sd_amplifier": 1.5,
         "noise_logistic": False}
    a.update({k: v for k, v in run_args.items() if k in a})
    for k, choices in (("HMM_type", HMM_TYPES), ("analysis_mode", ANALYSIS_MODES), ("tumor_subcluster_partition_method", PARTITION_METHODS)):
        a[k] = _match_arg(k, a[k], choices)
    method, mode = a["tumor_subcluster_partition_method"], a["analysis_mode"]
    token = "HMM" + a["HMM_type"] if a["HMM"] else ""
    names = {1: "%02d_incoming_data.infercnv_obj" % 1, 2: "%02d_reduced_by_cutoff.infercnv_obj" % 2,
             3: "%02d_normalized_by_depth%s.infercnv_obj" % (3, token), 4: "%02d_logtransformed%s.infercnv_obj" % (4, token),
             5: "%02d_scaled%s.infercnv_obj" % (5, token)}
    if a["num_ref_groups"] is not None:
        names[6] = "%02d_split_%sf_refs%s.infercnv_obj" % (6, token, _r_chr(a["num_ref_groups"]))
    if mode == "subclusters" and method == "random_trees":
        token += ".rand_trees"
        names[7] = "%02d_tumor_subclusters%s.%s.infercnv_obj" % (7, token, method)
    names[8] = "%02d_remove_ref_avg_from_obs_logFC%s.infercnv_obj" % (8, token)
    if not _is_na(a["max_centered_threshold"]):
        names[9] = "%02d_apply_max_centered_expr_threshold%s.infercnv_obj" % (9, token)
    names[10] = "%02d_smoothed_by_chr%s.infercnv_obj" % (10, token)
    names[11] = "%02d_recentered_cells_by_chr%s.infercnv_obj" % (11, token)
    names[12] = "%02d_remove_ref_avg_from_obs_adjust%s.infercnv_obj" % (12, token)
    if a["remove_genes_at_chr_ends"]:
        names[13] = "%02d_remove_gene_at_chr_ends%s.infercnv_obj" % (13, token)
    names[14] = "%02d_invert_log_transform%s.infercnv_obj" % (14, token)
    if mode == "subclusters" and method != "random_trees":
        token += "." + method
        names[15] = "%02d_tumor_subclusters%s.infercnv_obj" % (15, token)
    elif mode != "subclusters":
        names[15] = "%02d_no_subclustering%s.infercnv_obj" % (15, token)
    if a["prune_outliers"]:
        names[16] = "%02d_remove_outlier%s.infercnv_obj" % (16, token)
    tokens = file_tokens(a["HMM"], a["HMM_type"], mode, method, a["BayesMaxPNormal"])
    assert tokens["resume_file_token"] == token
    hmm_token = tokens["hmm_resume_file_token"]
    if a["HMM"]:
        names[17] = "%02d_HMM_pred%s.infercnv_obj" % (17, hmm_token)
        if a["BayesMaxPNormal"] > 0:
            names[18] = "%02d_HMM_pred.Bayes_Net%s.mcmc_obj" % (18, hmm_token)
            names[19] = "%02d_HMM_pred.Bayes_Net%s.Pnorm_%g.infercnv_obj" % (19, hmm_token, a["BayesMaxPNormal"])
        names[20] = "%02d_HMM_pred.repr_intensities%s.Pnorm_%g.infercnv_obj" % (20, hmm_token, a["BayesMaxPNormal"])
    if a["mask_nonDE_genes"]:
        names[21] = "%02d_mask_nonDE%s.infercnv_obj" % (21, token)
    if a["denoise"]:
        names[22] = "%02d_denoise%s.NF_%s.SD_%g.NL_%s.infercnv_obj" % (22, token, _r_chr(a["noise_filter"]), a["sd_amplifier"],
                                                                      _r_chr(a["noise_logistic"]))
    return names


def rds_checkpoints(out_dir, which="all", *, saver=None, compress=False, **run_args):
    """An on_step(step, label, obj) callable for run() that saves what infercnv::run saves with save_rds = TRUE and
    save_final_rds = TRUE (DESIGN K27), as .rds files R reads (rds.save_infercnv_obj), under R's own names:

      which="all"    every infercnv / HMM object under checkpoint_file_names(**run_args)[step], plus `preliminary.infercnv_obj`
                     (R/inferCNV_ops.R:1156: the object after step 15 -- after step 14 when step 15 does not run) and
                     `run.final.infercnv_obj` (:1618: the infercnv object after the last step that ran).  The two are hard
                     links to the step file that holds the same object (a copy where the file system has no links): no second
                     encode.
      which="final"  only those two: the object is written at step 14, again at step 15 if it runs, and `run.final` follows
                     the steps 16, 21 and 22 that run.
    run_args: the arguments run() is called with (the ones the names depend on are read, the others ignored); pass the same
    dict to both.  The step-18 MCMCInferCNV object has no R form here and is skipped with one log line.  A run that stops
    early (up_to_step) leaves `run.final.infercnv_obj` naming the last object it reached, which R would not have written.
    saver(obj, path): what writes a file (default rds.save_infercnv_obj); files are written under a temporary name and
    renamed.  compress: handed to the default saver (gzip files, as saveRDS writes by default; compressed on the device where
    the payloads go through it, DESIGN K28); ignored when `saver` is given.  Resuming from these files is not built."""
    if which not in ("all", "final"):
        raise ValueError("which: 'all' or 'final'")
    names = checkpoint_file_names(**run_args)
    if saver is None:
        from . import rds

        def saver(obj, path):
            return rds.save_infercnv_obj(obj, path, compress=compress)

    def write(obj, name):
        path = os.path.join(out_dir, name)
        saver(obj, path + ".tmp")
        os.replace(path + ".tmp", path)
        return path

    def alias(path, name):
        target = os.path.join(out_dir, name)
        if os.path.lexists(target + ".tmp"):
            os.remove(target + ".tmp")
        try:
            os.link(path, target + ".tmp")
        except OSError:
            import shutil
            shutil.copyfile(path, target + ".tmp")
        os.replace(target + ".tmp", target)

    def on_step(step, label, obj):
        if step == 18:
            log.info("rds_checkpoints: the step-18 MCMCInferCNV object (%s) is not written", names.get(18, "no file in R either"))
            return
        is_hmm_obj = step in (17, 19, 20)
        path = None
        if which == "all" and step in names:
            path = write(obj, names[step])
        if is_hmm_obj:
            return
        if step in (14, 15):
            path = path or write(obj, "preliminary.infercnv_obj")
            if which == "all":
                alias(path, "preliminary.infercnv_obj")
            alias(path, "run.final.infercnv_obj")
        elif which == "all" and path is not None:
            alias(path, "run.final.infercnv_obj")
        elif which == "final" and step > 15:
            write(obj, "run.final.infercnv_obj")

    on_step.file_names = names
    return on_step


def mcmc_diagnostics_hook(out_dir, *, max_sample_bytes=2 << 30, **run_args):
    """An on_step(step, label, obj) callable for run() that does what `diagnostics = TRUE` stands for in infercnv::run, as
    data (DESIGN K31): at step 18, where run() passes the MCMC object, bayes_net.mcmc_diagnostics writes
    CNV_MCMC_Diagnostics.dat into R's `BayesNetOutput.<token>` directory under out_dir (file_tokens); every other step is
    ignored.  run_args: the arguments run() is called with (the ones the directory depends on are read, the others ignored).
    The record of the last call is kept as on_step.diagnostics.  run()'s own `diagnostics` argument stays accepted and ignored:
    the plots are R's."""
    a = {"HMM": False, "HMM_type": "i6", "analysis_mode": "subclusters", "tumor_subcluster_partition_method": "leiden",
         "BayesMaxPNormal": 0.5}
    a.update({k: v for k, v in run_args.items() if k in a})
    for k, choices in (("HMM_type", HMM_TYPES), ("analysis_mode", ANALYSIS_MODES), ("tumor_subcluster_partition_method", PARTITION_METHODS)):
        a[k] = _match_arg(k, a[k], choices)
    target = os.path.join(out_dir, file_tokens(a["HMM"], a["HMM_type"], a["analysis_mode"], a["tumor_subcluster_partition_method"],
                                               a["BayesMaxPNormal"])["bayes_dir"])

    def on_step(step, label, obj):
        if step != 18:
            return
        from . import bayes_net
        on_step.diagnostics = bayes_net.mcmc_diagnostics(obj, max_sample_bytes=max_sample_bytes, out_dir=target)

    on_step.diagnostics = None
    on_step.out_dir = target
    return on_step


def bayes_probabilities_hook(out_dir, *, max_sample_bytes=2 << 30, **run_args):
    """An on_step(step, label, obj) callable for run() that does what `plot_probabilities = TRUE` stands for in infercnv::run
    (DESIGN K33).  At step 18, where run() passes the MCMC object, it writes into R's `BayesNetOutput.<token>` directory under
    out_dir (file_tokens), in R's order (R/inferCNV_BayesNet.R:1350-1361, 1429-1437):

      infercnv.NormalProbabilities.PreFiltering    bayes_net.postProbNormal of the object, " (1 - Probabilities of Normal)
                                                   Before Filtering": whatever heatmap.plot_cnv writes under that name
      cnvProbs.<p>.dat, cellProbs.<p>.dat          bayes_net.plotProbabilities of kept = bayes_net.kept_regions(obj,
                                                   BayesMaxPNormal), the object step 19's filter will return (<p>: the threshold)
      infercnv.NormalProbabilities.PostFiltering   postProbNormal of kept, " (1 - Probabilities of Normal) With Threshold <p>"

    Every other step is ignored.  run_args: the arguments run() is called with; the ones the directory depends on,
    BayesMaxPNormal, k_obs_groups, cluster_by_groups, useRaster, no_plot and plot_probabilities are read, the others ignored.
    With no_plot = True or plot_probabilities = False nothing is written and one line is logged.  The record of the last call
    is kept as on_step.probabilities.  run()'s own `plot_probabilities` argument stays accepted and ignored: the PDFs are R's.
    The regions are sampled again for the box statistics (as mcmc_diagnostics_hook samples them for its own table)."""
    a = {"HMM": False, "HMM_type": "i6", "analysis_mode": "subclusters", "tumor_subcluster_partition_method": "leiden",
         "BayesMaxPNormal": 0.5, "k_obs_groups": 1, "cluster_by_groups": True, "useRaster": True, "no_plot": False,
         "plot_probabilities": True}
    a.update({k: v for k, v in run_args.items() if k in a})
    for k, choices in (("HMM_type", HMM_TYPES), ("analysis_mode", ANALYSIS_MODES), ("tumor_subcluster_partition_method", PARTITION_METHODS)):
        a[k] = _match_arg(k, a[k], choices)
    target = os.path.join(out_dir, file_tokens(a["HMM"], a["HMM_type"], a["analysis_mode"], a["tumor_subcluster_partition_method"],
                                               a["BayesMaxPNormal"])["bayes_dir"])
    off = bool(a["no_plot"]) or not a["plot_probabilities"]

    def on_step(step, label, obj):
        if step != 18:
            return
        if off:
            log.info("bayes_probabilities_hook: no_plot / plot_probabilities = FALSE, nothing is written")
            return
        import copy
        from . import bayes_net
        obj = copy.copy(obj)                     # the plots' arguments ride in args, as in R's MCMC_inferCNV object
        obj.args = dict(obj.args, k_obs_groups=a["k_obs_groups"], cluster_by_groups=a["cluster_by_groups"], no_plot=False)
        thr = a["BayesMaxPNormal"]
        bayes_net.postProbNormal(obj, " (1 - Probabilities of Normal) Before Filtering", "infercnv.NormalProbabilities.PreFiltering",
                                 out_dir=target, useRaster=a["useRaster"])
        kept = bayes_net.kept_regions(obj, thr)
        on_step.probabilities = bayes_net.plotProbabilities(kept, target, max_sample_bytes=max_sample_bytes)
        bayes_net.postProbNormal(kept, " (1 - Probabilities of Normal) With Threshold %s" % bayes_net._r_threshold(thr),
                                 "infercnv.NormalProbabilities.PostFiltering", out_dir=target, useRaster=a["useRaster"])

    on_step.probabilities = None
    on_step.out_dir = target
    return on_step


def chain_hooks(*hooks):
    """One on_step(step, label, obj) that calls every hook given, in order (None entries are skipped): rds_checkpoints next to
    mcmc_diagnostics_hook and bayes_probabilities_hook, for instance."""
    hooks = [h for h in hooks if h is not None]

    def on_step(step, label, obj):
        for h in hooks:
            h(step, label, obj)

    return on_step


def check_arguments(a):
    """R's own stops and adjustments (R/inferCNV_ops.R:351-392) and the refusals of what the library does not build, on the
    dict of evaluated arguments `a` (adjusted in place).  Needs no GPU and writes nothing."""
    a["smooth_method"] = _match_arg("smooth_method", a["smooth_method"], SMOOTH_METHODS)
    a["HMM_type"] = _match_arg("HMM_type", a["HMM_type"], HMM_TYPES)
    if a["HMM"] and a["HMM_type"] == "i6" and a["smooth_method"] == "coordinates":
        log.error("Cannot use 'coordinate' smoothing method with i6 HMM model at this time.")
        raise ValueError("Incompatible HMM mode and smoothing method.")
    if a["smooth_method"] == "coordinates" and a["window_length"] < 10000:
        a["window_length"] = 10000000
        log.warning("smooth_method set to 'coordinates', but window_length is less than 10.000, setting it to 10.000.000. "
                    "Please set a different value > 10.000 if this default does not seem suitable.")
    a["leiden_function"] = _match_arg("leiden_function", a["leiden_function"], LEIDEN_FUNCTIONS)
    a["leiden_function_per_chr"] = _match_arg("leiden_function_per_chr", a["leiden_function_per_chr"], LEIDEN_FUNCTIONS[::-1])
    a["HMM_report_by"] = _match_arg("HMM_report_by", a["HMM_report_by"], HMM_REPORT_BY)
    a["analysis_mode"] = _match_arg("analysis_mode", a["analysis_mode"], ANALYSIS_MODES)
    if a["analysis_mode"] == "cells" and a["HMM_report_by"] != "cell":
        log.warning('analysis_mode is "cells" but HMM_report_by is not, changing HMM_report_by to "cells".')
        a["HMM_report_by"] = "cell"
    a["tumor_subcluster_partition_method"] = _match_arg("tumor_subcluster_partition_method",
                                                        a["tumor_subcluster_partition_method"], PARTITION_METHODS)
    a["leiden_method"] = _match_arg("leiden_method", a["leiden_method"], LEIDEN_METHODS)
    a["leiden_method_per_chr"] = _match_arg("leiden_method_per_chr", a["leiden_method_per_chr"], LEIDEN_METHODS[::-1])
    if a["tumor_subcluster_partition_method"] != "leiden":
        a["per_chr_hmm_subclusters"] = False
    if a["out_dir"] is None:
        log.error("Error, out_dir is NULL, please provide a path.")
        raise ValueError("out_dir is NULL")

    for name in ("noise_filter", "outlier_lower_bound", "outlier_upper_bound", "max_centered_threshold"):
        if _is_na(a[name]):
            a[name] = None
    # what the library does not build: refused here, before anything runs
    if a["tumor_subcluster_partition_method"] in ("qnorm", "pheight", "qgamma", "shc"):
        raise NotImplementedError(f'tumor_subcluster_partition_method = "{a["tumor_subcluster_partition_method"]}" is not built: '
                                  '"leiden" and "random_trees" are')
    if a["sim_method"] != "meanvar":
        raise NotImplementedError(f"sim_method {a['sim_method']!r} is not built: only 'meanvar' is")
    if a["sim_foreground"]:
        raise NotImplementedError("sim_foreground = TRUE (.sim_foreground) is not built")
    if a["plot_chr_scale"]:
        raise NotImplementedError("plot_chr_scale = TRUE is not built (plot_cnv)")
    if a["write_phylo"]:
        raise NotImplementedError("write_phylo = TRUE is not built (plot_cnv)")
    if a["output_format"] == "pdf":
        raise NotImplementedError("output_format 'pdf' is not built: plot_cnv produces the PNG panels only")
    if a["mask_nonDE_genes"] and a["test_use"] == "perm":
        raise NotImplementedError("test_use = 'perm' (coin::oneway_test) with mask_nonDE_genes is not built")
    for name, default in IGNORED_OPTIONS.items():
        if a[name] != default:
            log.info("run(): %s = %r is accepted for signature parity and ignored", name, a[name])
    return a


def _integral(x):
    if isinstance(x, DeviceMatrix):
        import torch
        return bool(torch.equal(x.tensor, torch.round(x.tensor)))
    if hasattr(x, "tocsc"):
        x = x.data
    x = np.asarray(x)
    return bool(np.issubdtype(x.dtype, np.integer) or np.array_equal(x, np.rint(x)))


def run(infercnv_obj: InfercnvObject,
        # gene filtering settings
        cutoff=1,
        min_cells_per_gene=3,
        out_dir=None,
        # smoothing params
        window_length=101,
        smooth_method="pyramidinal",
        num_ref_groups=None,
        ref_subtract_use_mean_bounds=True,
        # observation cell clustering settings
        cluster_by_groups=True,
        cluster_references=True,
        k_obs_groups=1,
        hclust_method="ward.D2",
        max_centered_threshold=3,
        scale_data=False,
        # HMM opts
        HMM=False,
        HMM_transition_prob=1e-6,
        HMM_report_by="subcluster",
        HMM_type="i6",
        HMM_i3_pval=0.05,
        HMM_i3_use_KS=False,
        BayesMaxPNormal=0.5,
        sim_method="meanvar",
        sim_foreground=False,
        reassignCNVs=True,
        # tumor subclustering options
        analysis_mode="subclusters",
        tumor_subcluster_partition_method="leiden",
        tumor_subcluster_pval=0.1,
        k_nn=20,
        leiden_method="PCA",
        leiden_function="CPM",
        leiden_resolution="auto",
        leiden_method_per_chr="simple",
        leiden_function_per_chr="modularity",
        leiden_resolution_per_chr=1,
        per_chr_hmm_subclusters=False,
        per_chr_hmm_subclusters_references=False,
        z_score_filter=0.8,
        # noise settings
        denoise=False,
        noise_filter=None,
        sd_amplifier=1.5,
        noise_logistic=False,
        # outlier adjustment settings
        outlier_method_bound="average_bound",
        outlier_lower_bound=None,
        outlier_upper_bound=None,
        # misc options
        final_scale_limits=None,
        final_center_val=None,
        debug=False,
        num_threads=4,
        plot_steps=False,
        inspect_subclusters=True,
        resume_mode=True,
        png_res=300,
        plot_probabilities=True,
        save_rds=True,
        save_final_rds=True,
        diagnostics=False,
        # experimental options
        remove_genes_at_chr_ends=False,
        prune_outliers=False,
        mask_nonDE_genes=False,
        mask_nonDE_pval=0.05,
        test_use="wilcoxon",
        require_DE_all_normals="any",
        hspike_aggregate_normals=False,
        no_plot=False,
        no_prelim_plot=False,
        write_expr_matrix=False,
        write_phylo=False,
        output_format="png",
        plot_chr_scale=False,
        chr_lengths=None,
        useRaster=True,
        up_to_step=100,
        *, seed=0, on_step=None) -> InfercnvObject:
    """infercnv::run (R/inferCNV_ops.R:242-1652): R's formals in R's order with R's defaults (`.` spelt `_`, NA / NULL are
    None, a match.arg vector selects its first element), R's 22 steps in R's order, each behind R's own condition, and
    `up_to_step` returning where R returns.  Returns the infercnv object after step 22 (not the HMM object).

    seed: handed unchanged to every stage that draws -- the hidden spike-in, the sd trend fit, the KS delta of the i3 HMM,
    both subclusterings, the Bayesian network and the rank-sum jitter.  Each keys its own documented stream; R draws unseeded.
    on_step(step_count, label, obj): called after every step that ran, with the object R would saveRDS there -- the infercnv
    object for steps 1-16, 21 and 22, the HMM object for steps 17, 19 and 20, the MCMCInferCNV for step 18.  It is the hook
    for checkpoints and the replacement of save_rds.

    Raises before anything is loaded or written: ValueError for R's own stops (out_dir None; the i6 HMM with smooth_method
    "coordinates"), NotImplementedError for tumor_subcluster_partition_method qnorm / pheight / qgamma / shc, a sim_method
    other than "meanvar", sim_foreground, plot_chr_scale, write_phylo, output_format "pdf", and test_use "perm" with
    mask_nonDE_genes.

    Accepted for signature parity and otherwise ignored (one log line each when set away from R's default): num_threads,
    debug, useRaster, diagnostics, plot_probabilities, save_rds, save_final_rds, resume_mode.  Nothing is serialised and
    nothing is resumed; the Bayes plots stay in R; inspect_subclusters (plot_subclusters) is logged as not built and skipped.

    Two routes through steps 2-4 and 8-14, both on the device: when nobody looks at the intermediate objects (on_step is
    None, plot_steps off, up_to_step not inside the block) ops.ingest_counts serves steps 2-4 (integer counts and no hidden
    spike-in, which is built from step 3's matrix) and ops.hip_smooth_chain steps 8-12 and 14 (step 13 not requested);
    otherwise the step functions run one by one (also with ref_subtract_use_mean_bounds off,
    which the fused chain does not offer).  An expr_data that is a scipy sparse matrix goes into the fused ingest as it
    is; the stepwise route densifies it once on the host and logs that.

    infercnv_obj.options receives the evaluated arguments (:446); they take precedence over entries already there."""
    a = dict(locals())
    for k in ("infercnv_obj", "seed", "on_step"):
        del a[k]
    check_arguments(a)                              # everything below reads the evaluated arguments
    smooth_method, HMM_type, window_length = a["smooth_method"], a["HMM_type"], a["window_length"]
    HMM_report_by, analysis_mode = a["HMM_report_by"], a["analysis_mode"]
    partition_method = a["tumor_subcluster_partition_method"]
    per_chr_hmm_subclusters = a["per_chr_hmm_subclusters"]
    noise_filter, max_centered_threshold = a["noise_filter"], a["max_centered_threshold"]

    from . import _lib, bayes_net, cnv_regions, heatmap, hidden_spike, hmm, mask_non_de, ops, tumor_subclusters
    _lib.load()
    log.info("::process_data:Start")
    if out_dir != "." and not os.path.exists(out_dir):
        log.info("Creating output path %s", out_dir)
        os.mkdir(out_dir)

    obj = infercnv_obj.copy()
    obj.options = {**a, **{k: v for k, v in (infercnv_obj.options or {}).items() if k not in a}}
    tokens = file_tokens(HMM, HMM_type, analysis_mode, partition_method, BayesMaxPNormal)
    hmm_token = tokens["hmm_resume_file_token"]

    def done(step, label, o):
        if on_step is not None:
            on_step(step, label, o)

    def plot(o, title, output_filename, **extra):
        heatmap.plot_cnv(o, out_dir=out_dir, title=title, output_filename=output_filename, k_obs_groups=k_obs_groups,
                         cluster_by_groups=cluster_by_groups, cluster_references=cluster_references, plot_chr_scale=plot_chr_scale,
                         chr_lengths=chr_lengths, output_format=output_format, write_expr_matrix=write_expr_matrix,
                         write_phylo=write_phylo, png_res=png_res, useRaster=useRaster, **extra)

    def step_plot(o, step, title, filename):
        if plot_steps:
            plot(o, "%02d_%s" % (step, title), "infercnv.%02d_%s" % (step, filename))

    def skip_inspect():
        if inspect_subclusters:
            log.info("inspect_subclusters: plot_subclusters is not built, skipped")

    need_hspike = bool(HMM) and HMM_type == "i6"
    unobserved = on_step is None and not plot_steps
    fused_ingest = (unobserved and up_to_step >= 4 and not need_hspike and obj.hspike is None and _integral(obj.expr_data))
    fused_chain = (unobserved and up_to_step >= 14 and ref_subtract_use_mean_bounds
                   and not (remove_genes_at_chr_ends and smooth_method != "coordinates"))

    step = 0
    if up_to_step == step:
        return obj
    step = 1                                                                               # incoming data
    if not fused_ingest and hasattr(obj.expr_data, "tocsc"):
        log.info("run(): the stepwise route densifies the sparse expr_data once on the host (%d x %d)", *obj.expr_data.shape)
        obj.expr_data = np.asarray(obj.expr_data.todense())
    done(step, "incoming data", obj)

    if fused_ingest:                                                                       # steps 2, 3, 4 in one call
        log.info("STEP 02-04: gene filters, normalization by sequencing depth, log transformation (fused ingest)")
        obj, _ = ops.ingest_counts(obj, min_mean_expr_cutoff=cutoff, min_cells_per_gene=min_cells_per_gene)
        step = 4
    else:
        if up_to_step == step:
            return obj
        step = 2
        log.info("STEP %02d: Removing lowly expressed genes", step)
        obj = ops.require_above_min_mean_expr_cutoff(obj, cutoff)
        obj = ops.require_above_min_cells_ref(obj, min_cells_per_gene)
        done(step, "Removing lowly expressed genes", obj)

        if up_to_step == step:
            return obj
        step = 3
        log.info("STEP %02d: normalization by sequencing depth", step)
        obj = ops.normalize_counts_by_seq_depth(obj)
        if need_hspike:                                                                    # the hidden spike needed by the HMM
            obj = hidden_spike.build_and_add_hspike(obj, sim_method=sim_method, aggregate_normals=hspike_aggregate_normals, seed=seed)
        done(step, "normalization by sequencing depth", obj)

        if up_to_step == step:
            return obj
        step = 4
        log.info("STEP %02d: log transformation of data", step)
        obj = ops.log2xplus1(obj)
        done(step, "log transformation of data", obj)
        step_plot(obj, step, "log_transformed_data", "log_transformed")

    if up_to_step == step:
        return obj
    step = 5
    if scale_data:
        log.info("STEP %02d: scaling all expression data", step)
        obj = ops.scale_infercnv_expr(obj)
        done(step, "scaling all expression data", obj)
        step_plot(obj, step, "scaled", "scaled")

    if up_to_step == step:
        return obj
    step = 6
    if num_ref_groups is not None:
        if not obj.has_reference_cells():
            raise ValueError("Error, no reference cells defined. Cannot split them into groups as requested")
        log.info("STEP %02d: splitting reference data into %d clusters", step, num_ref_groups)
        obj = ops.split_references(obj, num_groups=num_ref_groups, hclust_method=hclust_method)
        done(step, "splitting reference data", obj)

    if up_to_step == step:
        return obj
    step = 7
    if analysis_mode == "subclusters" and partition_method == "random_trees":
        log.info("STEP %02d: computing tumor subclusters via %s", step, partition_method)
        obj = tumor_subclusters.define_signif_tumor_subclusters_via_random_smooothed_trees(
            obj, p_val=tumor_subcluster_pval, hclust_method=hclust_method, cluster_by_groups=cluster_by_groups, seed=seed)
        done(step, "computing tumor subclusters via %s" % partition_method, obj)
        step_plot(obj, step, "tumor_subclusters.%s" % partition_method, "tumor_subclusters.%s" % partition_method)
        skip_inspect()

    if fused_chain:                                                                        # steps 8-12 and 14 in one pass
        if up_to_step == step:
            return obj
        log.info("STEP 08-14: reference subtraction, threshold, smoothing, centering, reference subtraction, invert log (fused chain)")
        obj = ops.hip_smooth_chain(obj, window_length=window_length, max_centered_threshold=max_centered_threshold, denoise=False,
                                   smooth_method=smooth_method)
        step = 14
    else:
        if up_to_step == step:
            return obj
        step = 8
        log.info("STEP %02d: removing average of reference data (before smoothing)", step)
        obj = ops.subtract_ref_expr_from_obs(obj, inv_log=False, use_bounds=ref_subtract_use_mean_bounds)
        done(step, "removing average of reference data (before smoothing)", obj)
        step_plot(obj, step, "remove_average", "remove_average")

        if up_to_step == step:
            return obj
        step = 9
        if max_centered_threshold is not None:
            log.info("STEP %02d: apply max centered expression threshold: %s", step, max_centered_threshold)
            obj = ops.apply_max_threshold_bounds(obj, threshold=max_centered_threshold)   # "auto": mean(abs(get_average_bounds()))
            done(step, "apply max centered expression threshold", obj)
            step_plot(obj, step, "apply_max_centered_expr_threshold", "apply_max_centred_expr_threshold")

        if up_to_step == step:
            return obj
        step = 10
        log.info("STEP %02d: Smoothing data per cell by chromosome", step)
        if smooth_method == "runmeans":
            obj = ops.smooth_by_chromosome_runmeans(obj, window_length)
        elif smooth_method == "pyramidinal":
            obj = ops.smooth_by_chromosome(obj, window_length=window_length, smooth_ends=True)
        else:
            obj = ops.smooth_by_chromosome_coordinates(obj, window_length=window_length)
        done(step, "Smoothing data per cell by chromosome", obj)
        step_plot(obj, step, "smoothed_by_chr", "smoothed_by_chr")

        if up_to_step == step:
            return obj
        step = 11
        log.info("STEP %02d: re-centering data across chromosome after smoothing", step)
        obj = ops.center_cell_expr_across_chromosome(obj, method="median")
        done(step, "re-centering data across chromosome after smoothing", obj)
        step_plot(obj, step, "centering_of_smoothed", "centering_of_smoothed")

        if up_to_step == step:
            return obj
        step = 12
        log.info("STEP %02d: removing average of reference data (after smoothing)", step)
        obj = ops.subtract_ref_expr_from_obs(obj, inv_log=False, use_bounds=ref_subtract_use_mean_bounds)
        done(step, "removing average of reference data (after smoothing)", obj)
        step_plot(obj, step, "remove_average", "remove_average")

        if up_to_step == step:
            return obj
        step = 13
        if remove_genes_at_chr_ends and smooth_method != "coordinates":
            log.info("STEP %02d: removing genes at chr ends", step)
            obj = ops.remove_genes_at_ends_of_chromosomes(obj, window_length)
            done(step, "removing genes at chr ends", obj)
            step_plot(obj, step, "remove_genes_at_chr_ends", "remove_genes_at_chr_ends")

        if up_to_step == step:
            return obj
        step = 14
        log.info("STEP %02d: invert log2(FC) to FC", step)
        obj = ops.invert_log2(obj)
        done(step, "invert log2(FC) to FC", obj)
        step_plot(obj, step, "invert_log_transform log(FC)->FC", "invert_log_FC")

    if up_to_step == step:
        return obj
    step = 15
    subclusters_per_chr = None
    if analysis_mode == "subclusters" and partition_method != "random_trees":
        log.info("STEP %02d: computing tumor subclusters via %s", step, partition_method)
        obj, subclusters_per_chr = tumor_subclusters.define_signif_tumor_subclusters(
            obj, p_val=tumor_subcluster_pval, k_nn=k_nn, leiden_resolution=leiden_resolution, leiden_method=a["leiden_method"],
            leiden_function=a["leiden_function"], leiden_method_per_chr=a["leiden_method_per_chr"],
            leiden_function_per_chr=a["leiden_function_per_chr"], leiden_resolution_per_chr=leiden_resolution_per_chr,
            hclust_method=hclust_method, cluster_by_groups=cluster_by_groups, partition_method=partition_method,
            per_chr_hmm_subclusters=per_chr_hmm_subclusters, per_chr_hmm_subclusters_references=per_chr_hmm_subclusters_references,
            z_score_filter=z_score_filter, seed=seed)
        done(step, "computing tumor subclusters via %s" % partition_method, obj)
        step_plot(obj, step, "tumor_subclusters", "tumor_subclusters")
        skip_inspect()
    elif analysis_mode != "subclusters":
        log.info("STEP %02d: Clustering samples (not defining tumor subclusters)", step)
        obj = tumor_subclusters.define_signif_tumor_subclusters(
            obj, p_val=tumor_subcluster_pval, hclust_method=hclust_method, cluster_by_groups=cluster_by_groups,
            partition_method="none", per_chr_hmm_subclusters=False, z_score_filter=z_score_filter, seed=seed)[0]
        done(step, "Clustering samples (not defining tumor subclusters)", obj)

    # "This is a milestone step and results should always be examined here."
    if not (no_prelim_plot or no_plot):
        plot(obj, "Preliminary infercnv (pre-noise filtering)", "infercnv.preliminary")

    if up_to_step == step:
        return obj
    step = 16
    if prune_outliers:
        log.info("STEP %02d: Removing outliers", step)
        obj = ops.remove_outliers_norm(obj, out_method=outlier_method_bound, lower_bound=a["outlier_lower_bound"],
                                       upper_bound=a["outlier_upper_bound"])
        done(step, "Removing outliers", obj)
        step_plot(obj, step, "removed_outliers", "removed_outliers")

    if up_to_step == step:
        return obj
    step = 17
    hmm_obj = None
    hmm_center, hmm_state_range = (3, (0, 6)) if HMM_type == "i6" else (2, (1, 3))
    if HMM:
        log.info("STEP %02d: HMM-based CNV prediction", step)
        t = HMM_transition_prob
        if HMM_type == "i6":
            cnv_mean_sd = hmm.get_spike_dists(obj.hspike)
            if analysis_mode == "cells":
                hmm_obj = hmm.predict_CNV_via_HMM_on_indiv_cells(obj, cnv_mean_sd, t=t)
            else:                                    # the group-level predictors scale the sd by the group's size: one fit
                fit = hmm.get_hspike_cnv_mean_sd_trend_by_num_cells_fit(obj.hspike, seed=seed)
                if analysis_mode == "subclusters" and partition_method == "leiden" and per_chr_hmm_subclusters:
                    hmm_obj = hmm.predict_CNV_via_HMM_on_tumor_subclusters_per_chr(obj, subclusters_per_chr, cnv_mean_sd, fit, t=t)
                elif analysis_mode == "subclusters":
                    hmm_obj = hmm.predict_CNV_via_HMM_on_tumor_subclusters(obj, cnv_mean_sd, fit, t=t)
                else:
                    hmm_obj = hmm.predict_CNV_via_HMM_on_whole_tumor_samples(obj, cluster_by_groups, cnv_mean_sd, fit, t=t)
        else:
            i3 = dict(i3_p_val=HMM_i3_pval, t=t, use_KS=HMM_i3_use_KS, seed=seed)
            if analysis_mode == "subclusters":
                hmm_obj = hmm.i3HMM_predict_CNV_via_HMM_on_tumor_subclusters(obj, **i3)
            elif analysis_mode == "cells":
                hmm_obj = hmm.i3HMM_predict_CNV_via_HMM_on_indiv_cells(obj, **i3)
            else:
                hmm_obj = hmm.i3HMM_predict_CNV_via_HMM_on_whole_tumor_samples(obj, cluster_by_groups, **i3)
        if analysis_mode == "subclusters" and partition_method == "random_trees":
            # the subcluster assignments do not always line up with the top-level dendrogram
            hmm_obj = tumor_subclusters.redo_hierarchical_clustering(hmm_obj, hclust_method=hclust_method)
        cnv_regions.generate_cnv_region_reports(hmm_obj, tokens["hmm_prefix"], out_dir, ignore_neutral_state=hmm_center,
                                                by=HMM_report_by)
        done(step, "HMM-based CNV prediction", hmm_obj)
        if not no_plot:
            plot(hmm_obj, "%02d_HMM_preds" % step, "infercnv.%02d_HMM_pred%s" % (step, hmm_token), x_center=hmm_center,
                 x_range=hmm_state_range)

    if up_to_step == step:
        return obj
    step = 18
    bayes = bool(HMM) and BayesMaxPNormal > 0 and states_not_constant(hmm_obj.expr_data)
    mcmc_obj = None
    if bayes:
        log.info("STEP %02d: Run Bayesian Network Model on HMM predicted CNVs", step)
        mcmc_obj = bayes_net.inferCNVBayesNet(obj, hmm_obj.expr_data, HMM_type=HMM_type, by=HMM_report_by,
                                              postMcmcMethod="removeCNV", reassignCNVs=reassignCNVs,
                                              out_dir=os.path.join(out_dir, tokens["bayes_dir"]), seed=seed,
                                              route="table" if HMM_report_by == "cell" else "dict")
        done(step, "Run Bayesian Network Model on HMM predicted CNVs", mcmc_obj)

    if up_to_step == step:
        return obj
    step = 19
    if bayes:
        log.info("STEP %02d: Filter HMM predicted CNVs based on the Bayesian Network Model results and BayesMaxPNormal", step)
        filtered, states = bayes_net.filterHighPNormals(mcmc_obj, hmm_obj.expr_data, BayesMaxPNormal)
        hmm_obj = hmm_obj.copy()
        hmm_obj.expr_data = states
        done(step, "Filter HMM predicted CNVs", hmm_obj)
        if not no_plot:
            plot(hmm_obj, "%02d_HMM_preds_Bayes_Net" % step, "infercnv.%02d_HMM_pred.Bayes_Net.Pnorm_%g" % (step, BayesMaxPNormal),
                 x_center=hmm_center, x_range=hmm_state_range)
        cnv_regions.adjust_genes_regions_report(filtered, input_filename_prefix=tokens["hmm_prefix"],
                                                output_filename_prefix=tokens["bayes_prefix"], out_dir=out_dir)

    if up_to_step == step:
        return obj
    step = 20
    if HMM:
        log.info("STEP %02d: Converting HMM-based CNV states to repr expr vals", step)
        if HMM_type == "i6":
            hmm_obj = hmm.assign_HMM_states_to_proxy_expr_vals(hmm_obj)
        else:
            hmm_obj = hmm.i3HMM_assign_HMM_states_to_proxy_expr_vals(hmm_obj)
        done(step, "Converting HMM-based CNV states to repr expr vals", hmm_obj)
        if not no_plot:
            plot(hmm_obj, "%02d_HMM_preds.repr_intensities" % step,
                 "infercnv.%02d_HMM_pred%s.Pnorm_%g.repr_intensities" % (step, hmm_token, BayesMaxPNormal), x_center=1, x_range=(-1, 3))

    if up_to_step == step:
        return obj
    step = 21
    if mask_nonDE_genes:
        if not obj.has_reference_cells():
            raise ValueError("Error, cannot mask non-DE genes when there are no normal references set")
        log.info("STEP %02d: Identify and mask non-DE genes", step)
        obj = mask_non_de.mask_non_DE_genes_basic(obj, p_val_thresh=mask_nonDE_pval, test_use=test_use, center_val=None,
                                                  require_DE_all_normals=require_DE_all_normals, seed=seed)   # None: mean(expr.data)
        done(step, "Identify and mask non-DE genes", obj)
        step_plot(obj, step, "mask_nonDE", "mask_nonDE")

    if up_to_step == step:
        return obj
    step = 22
    if denoise:
        log.info("STEP %02d: Denoising", step)
        if noise_filter is not None:
            if noise_filter > 0:
                log.info("::process_data:Remove noise, noise threshold at: %s", noise_filter)
                obj = ops.clear_noise(obj, threshold=noise_filter, noise_logistic=noise_logistic)
            # noise_filter == 0 or negative: don't remove noise
        else:
            log.info("::process_data:Remove noise, noise threshold defined via ref mean sd_amplifier: %s", sd_amplifier)
            obj = ops.clear_noise_via_ref_mean_sd(obj, sd_amplifier=sd_amplifier, noise_logistic=noise_logistic)
        done(step, "Denoising", obj)
        if plot_steps:
            plot(obj, "%02d_denoised" % step, "infercnv.%02d_denoised" % step, color_safe_pal=False)

    if not no_plot:
        log.info("## Making the final infercnv heatmap ##")
        plot(obj, "inferCNV", "infercnv", x_center=1 if final_center_val is None else final_center_val,
             x_range="auto" if final_scale_limits is None else final_scale_limits)
    return obj

