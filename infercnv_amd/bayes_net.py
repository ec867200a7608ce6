"""The Bayesian filter of the HMM-predicted CNV regions (steps 18-19 of run(), R/inferCNV_ops.R:1363-1453): mirror of
inferCNVBayesNet / filterHighPNormals (R/inferCNV_BayesNet.R) on the GPU sampler of DESIGN K13.

The reference fits one JAGS mixture model per region; here every region of a run goes through ONE likelihood pass and ONE
sampler launch (device.bayes_loglik / device.bayes_sample, contract in include/icnv.h).  The posterior is the same, the random
stream is this library's own (seeded, per draw), so probabilities agree with JAGS up to Monte-Carlo error, not bit for bit.
Plotting (postProbNormal, plotProbabilities, mcmcDiagnosticPlots) stays out.  Index vectors are 0-based (R: 1-based);
states keep R's numbering 1..K."""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from . import cnv_regions, device, hmm
from .infercnv_object import InfercnvObject
from .tumor_subclusters import fnv1a64

NA_INTEGER = np.iinfo(np.int32).min


def _normal_state(HMM_type):
    return 3 if HMM_type == "i6" else 2


@dataclass
class MCMCInferCNV:
    """The slots of MCMC_inferCNV (R/inferCNV_BayesNet.R:31-40) that steps 18-19 use.  cnv_regions: region names;
    cell_gene: per region {"cnv_regions": name, "Genes": gene rows, "Cells": columns (ascending), "State": HMM state};
    mu / sig: state means and PRECISIONS (1 / sd^2, MeanSD :148-198); group_id: per cell the 1-based number of its cell
    group (NA_INTEGER elsewhere); cnv_probabilities: per region the kept theta samples (K n_keep x K) when they were asked
    for, else None; cnv_means: K x regions, their column means (what the reference takes from them); cell_probabilities:
    per region the K x |Cells| state frequencies of eps; args: the arguments of the call."""
    infercnv_obj: InfercnvObject
    cnv_regions: List[str] = field(default_factory=list)
    cell_gene: List[dict] = field(default_factory=list)
    mu: Optional[np.ndarray] = None
    sig: Optional[np.ndarray] = None
    group_id: Optional[np.ndarray] = None
    cnv_probabilities: List[Optional[np.ndarray]] = field(default_factory=list)
    cnv_means: Optional[np.ndarray] = None
    cell_probabilities: List[np.ndarray] = field(default_factory=list)
    args: dict = field(default_factory=dict)
    x_dev: object = None                      # the (C, G) CUDA matrix the sampler reads


def mean_sd(infercnv_obj: InfercnvObject, HMM_type, i3_p_val=0.05):
    """MeanSD (R/inferCNV_BayesNet.R:148-198) -> (mu, sig = 1 / sd^2)."""
    if HMM_type == "i6":
        d = hmm.get_spike_dists(infercnv_obj.hspike)
        keys = sorted(d)
        mu = np.array([d[k]["mean"] for k in keys], dtype=np.float64)
        sd = np.array([d[k]["sd"] for k in keys], dtype=np.float64)
        return mu, 1.0 / (sd * sd)
    t = hmm.i3HMM_get_sd_trend(infercnv_obj, i3_p_val)
    mu = np.array([t["mu"] - t["mean_delta"], t["mu"], t["mu"] + t["mean_delta"]], dtype=np.float64)
    return mu, np.full(3, 1.0 / (t["sigma"] * t["sigma"]))


def _gene_run(genes, name):
    genes = np.asarray(genes, dtype=np.int64)
    if genes.size == 0 or (genes.size > 1 and not np.all(np.diff(genes) == 1)):
        raise ValueError(f"region {name}: its genes must be one contiguous run of rows (order the object by chromosome)")
    return int(genes[0]), int(genes.size)


def run_mcmc(obj: MCMCInferCNV) -> MCMCInferCNV:
    """runMCMC + getProbabilities (R/inferCNV_BayesNet.R:709-731, 362-388): every region in one call."""
    a = obj.args
    K = len(obj.mu)
    if not obj.cell_gene:
        obj.cnv_probabilities, obj.cell_probabilities, obj.cnv_means = [], [], np.zeros((K, 0))
        return obj
    regions = [_gene_run(cg["Genes"], cg["cnv_regions"]) + (np.asarray(cg["Cells"], dtype=np.int32),) for cg in obj.cell_gene]
    tokens = [fnv1a64(cg["cnv_regions"]) for cg in obj.cell_gene]
    _, L, off = device.bayes_loglik(obj.x_dev, regions, obj.mu, obj.sig)
    theta_sum, samples, freq = device.bayes_sample(L, off, tokens, a["n_adapt"], a["n_burn"], a["n_keep"], a["seed"],
                                                   want_samples=a["keep_samples"])
    theta_sum = theta_sum.cpu().numpy()
    freq = freq.cpu().numpy()
    n = float(K * a["n_keep"])
    tot = np.zeros((len(regions), K))
    for ch in range(K):                        # the chain sums in chain order, one division
        tot = tot + theta_sum[:, ch, :]
    obj.cnv_means = (tot / n).T.copy()
    samples = samples.cpu().numpy() if samples is not None else None
    obj.cnv_probabilities = [samples[r].reshape(-1, K) if samples is not None else None for r in range(len(regions))]
    obj.cell_probabilities = [(freq[off[r]:off[r + 1]].astype(np.float64) / n).T.copy() for r in range(len(regions))]
    return obj


def inferCNVBayesNet(infercnv_obj: InfercnvObject, HMM_states, HMM_type="i6", by="subcluster", postMcmcMethod="removeCNV",
                     reassignCNVs=True, out_dir=None, seed=0, n_adapt=500, n_burn=200, n_keep=1000, keep_samples=False,
                     i3_p_val=0.05, mu=None, sig=None, x=None) -> MCMCInferCNV:
    """inferCNVBayesNet (R/inferCNV_BayesNet.R:1237-1364).  infercnv_obj: the object the HMM ran on (its expr_data are the
    values the mixture model sees); HMM_states: the genes x cells state matrix of step 17 (1..K).  The regions are those of
    cnv_regions.get_predicted_CNV_regions(states, by) without the neutral state -- what initializeObject / getGenesCells
    (:245-338) read back from the step-17 report files.  mu / sig default to mean_sd(); x: the (C, G) CUDA matrix when it is
    already on the device.  keep_samples: also keep every theta sample (K n_keep x K per region)."""
    import torch
    if HMM_type not in ("i6", "i3"):
        raise ValueError("HMM_type must be i6 or i3")
    normal = _normal_state(HMM_type)
    states = np.asarray(HMM_states)
    st_obj = infercnv_obj.copy()
    st_obj.expr_data = states.astype(np.float64)
    groups = cnv_regions.get_predicted_CNV_regions(st_obj, by)
    cells_all = infercnv_obj.cells()
    col_of = {str(c): i for i, c in enumerate(cells_all)}
    obj = MCMCInferCNV(infercnv_obj=infercnv_obj)
    obj.args = {"HMM_type": HMM_type, "postMcmcMethod": postMcmcMethod, "reassignCNVs": bool(reassignCNVs), "out_dir": out_dir,
                "BayesMaxPNormal": 0, "seed": int(seed), "n_adapt": int(n_adapt), "n_burn": int(n_burn), "n_keep": int(n_keep),
                "keep_samples": bool(keep_samples), "by": by}
    n_obs = max((int(np.max(v)) + 1 for v in infercnv_obj.observation_grouped_cell_indices.values() if len(v)), default=0)
    group_id = np.full(n_obs, NA_INTEGER, dtype=np.int64)
    gid = 0
    for grp in groups:
        cols = np.sort(np.array([col_of[str(c)] for c in grp["cells"]], dtype=np.int64))
        kept = [(rn, r) for rn, r in grp["gene_regions"] if r["state"] != normal]
        if not kept:
            continue
        gid += 1                                # unique(pred_cnv_genes_df$cell_group_name): groups with a region, in file order
        group_id[cols[cols < n_obs]] = gid
        for rn, r in kept:
            obj.cnv_regions.append(rn)
            obj.cell_gene.append({"cnv_regions": rn, "Genes": np.asarray(r["gene"], dtype=np.int64), "Cells": cols.copy(),
                                  "State": int(r["state"])})
    obj.group_id = group_id
    if mu is None or sig is None:
        mu, sig = mean_sd(infercnv_obj, HMM_type, i3_p_val)
    obj.mu, obj.sig = np.asarray(mu, dtype=np.float64), np.asarray(sig, dtype=np.float64)
    if obj.mu.size != (6 if HMM_type == "i6" else 3) or obj.sig.size != obj.mu.size:
        raise ValueError("mu and sig must have one entry per state")
    obj.x_dev = x if x is not None else torch.from_numpy(
        np.ascontiguousarray(np.asarray(infercnv_obj.expr_data, dtype=np.float64).T)).cuda()
    return run_mcmc(obj)


# ---- step 19 ----------------------------------------------------------------------------------------------------------
class _States:
    """The state matrix where the caller holds it: a (cells, genes) CUDA tensor stays on the device and its rectangles are
    rewritten there; a genes x cells host array is rewritten on the host.  Either way the input itself is left alone."""

    def __init__(self, HMM_states):
        import torch
        self.on_device = isinstance(HMM_states, torch.Tensor)
        if self.on_device:
            if not HMM_states.is_cuda or HMM_states.dim() != 2:
                raise TypeError("HMM_states: a genes x cells array or a (cells, genes) CUDA tensor")
            self.m = HMM_states.clone()
        else:
            self.m = np.array(HMM_states)

    def fill(self, genes, cells, value):
        if len(cells) == 0:
            return
        g0, ng = _gene_run(genes, "")
        if self.on_device:
            import torch
            self.m[torch.as_tensor(np.asarray(cells, dtype=np.int64), device=self.m.device), g0:g0 + ng] = value
        else:
            self.m[g0:g0 + ng, np.asarray(cells, dtype=np.int64)] = value

    def result(self):
        return self.m


def _remove_cnv(obj: MCMCInferCNV, st: _States):
    """removeCNV (R/inferCNV_BayesNet.R:562-630): strictly above the threshold; a region without cells (NaN) stays."""
    normal = _normal_state(obj.args["HMM_type"])
    thr = obj.args["BayesMaxPNormal"]
    p_normal = obj.cnv_means[normal - 1] if obj.cnv_means.size else np.zeros(0)
    remove = np.nonzero(p_normal > thr)[0]
    if remove.size == 0:
        return obj
    for i in remove:
        st.fill(obj.cell_gene[i]["Genes"], obj.cell_gene[i]["Cells"], normal)
    keep = [i for i in range(len(obj.cell_gene)) if i not in set(remove.tolist())]
    obj.cell_gene = [obj.cell_gene[i] for i in keep]
    obj.cnv_regions = [obj.cnv_regions[i] for i in keep]
    obj.cell_probabilities = [obj.cell_probabilities[i] for i in keep]
    obj.cnv_probabilities = [obj.cnv_probabilities[i] for i in keep]
    obj.cnv_means = obj.cnv_means[:, keep]
    out_dir = obj.args.get("out_dir")
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "CNV_State_Probabilities.dat"), "w") as fh:   # write.table(row.names = TRUE): no corner cell
            fh.write("\t".join(cg["cnv_regions"] for cg in obj.cell_gene) + "\n")
            for k in range(obj.cnv_means.shape[0]):
                fh.write("\t".join([f"State:{k + 1}"] + [cnv_regions._fmt(float(v)) if v == v else "NaN" for v in obj.cnv_means[k]]) + "\n")
    return obj


def _remove_cells(obj: MCMCInferCNV, st: _States):
    """removeCells (R/inferCNV_BayesNet.R:650-685): the cells whose own P(normal) is above the threshold leave their region
    and are set to the normal state; then the sampler runs once more on the shrunken regions.  (The reference computes the
    rewrite of those cells' states and returns only the object, :683, so its caller never sees it; here it is kept.)"""
    normal = _normal_state(obj.args["HMM_type"])
    thr = obj.args["BayesMaxPNormal"]
    hit = False
    for i, cp in enumerate(obj.cell_probabilities):
        idx = np.nonzero(cp[normal - 1] > thr)[0] if cp.size else np.zeros(0, dtype=np.int64)
        if idx.size:
            hit = True
            cells = obj.cell_gene[i]["Cells"]
            st.fill(obj.cell_gene[i]["Genes"], cells[idx], normal)
            obj.cell_gene[i]["Cells"] = np.delete(cells, idx)
    return run_mcmc(obj) if hit else obj


def _reassign_cnv(obj: MCMCInferCNV, st: _States):
    """reassignCNV (R/inferCNV_BayesNet.R:491-540): every region takes its most probable state.  On a tie of the maximum
    R's which(i == max(i)) yields two values and the assignment fails; the first is taken here.  A region without cells
    (NaN probabilities) keeps its HMM state."""
    for i, cg in enumerate(obj.cell_gene):
        col = obj.cnv_means[:, i]
        if np.isnan(col).any():
            continue
        cg["State"] = int(np.argmax(col)) + 1
        st.fill(cg["Genes"], cg["Cells"], cg["State"])
    return obj


def filterHighPNormals(mcmc_obj: MCMCInferCNV, HMM_states, BayesMaxPNormal):
    """filterHighPNormals (R/inferCNV_BayesNet.R:1394-1440) -> (mcmc_obj, HMM_states).  HMM_states: genes x cells array, or a
    (cells, genes) CUDA tensor, which stays on the device and is rewritten there; a new array / tensor of the same kind comes
    back.  The object passed in is not modified."""
    import copy
    obj = copy.copy(mcmc_obj)
    obj.cell_gene = [dict(cg) for cg in mcmc_obj.cell_gene]
    obj.cnv_regions = list(mcmc_obj.cnv_regions)
    obj.args = dict(mcmc_obj.args, BayesMaxPNormal=BayesMaxPNormal)
    st = _States(HMM_states)
    method = obj.args.get("postMcmcMethod")
    if method is not None:
        obj = _remove_cnv(obj, st) if method == "removeCNV" else _remove_cells(obj, st)
        if obj.args.get("reassignCNVs"):
            obj = _reassign_cnv(obj, st)
    return obj, st.result()
