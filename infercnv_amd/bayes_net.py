"""The Bayesian filter of the HMM-predicted CNV regions (steps 18-19 of run(), R/inferCNV_ops.R:1363-1453): mirror of
inferCNVBayesNet / filterHighPNormals (R/inferCNV_BayesNet.R) on the GPU sampler of DESIGN K13.

The reference fits one JAGS mixture model per region; here every region of a run goes through ONE likelihood pass and ONE
sampler launch (device.bayes_loglik / device.bayes_sample, contract in include/icnv.h).  The posterior is the same, the random
stream is this library's own (seeded, per draw), so probabilities agree with JAGS up to Monte-Carlo error, not bit for bit.
The pages R draws stay in R; what is under them is built here: postProbNormal's heatmaps go through heatmap.plot_cnv and
plotProbabilities' stacked bars and box plots are written as tables (DESIGN K33); the numbers under mcmcDiagnosticPlots' plots
and table are mcmc_diagnostics (DESIGN K31).  Index vectors are 0-based (R: 1-based); states keep R's numbering 1..K."""
from __future__ import annotations

import logging
import operator
import os
from collections.abc import Sequence
from dataclasses import dataclass, field, replace
from typing import List, Optional

import numpy as np

from . import cnv_regions, device, hmm
from .infercnv_object import DeviceMatrix, InfercnvObject
from .tumor_subclusters import fnv1a64

NA_INTEGER = np.iinfo(np.int32).min
log = logging.getLogger("infercnv_amd")


def _normal_state(HMM_type):
    return 3 if HMM_type == "i6" else 2


@dataclass
class MCMCInferCNV:
    """The slots of MCMC_inferCNV (R/inferCNV_BayesNet.R:31-40) that steps 18-19 use.  cnv_regions: region names;
    cell_gene: per region {"cnv_regions": name, "Genes": gene rows, "Cells": columns (ascending), "State": HMM state};
    mu / sig: state means and PRECISIONS (1 / sd^2, MeanSD :148-198); group_id: per cell the 1-based number of its cell
    group (NA_INTEGER elsewhere); cnv_probabilities: per region the kept theta samples (K n_keep x K) when they were asked
    for, else None; cnv_means: K x regions, their column means (what the reference takes from them); cell_probabilities:
    per region the K x |Cells| state frequencies of eps; args: the arguments of the call.  cell_prob_rows (table route):
    every region's cell_probabilities transposed and stacked, (cell_off[-1], K), the rows of region r at table.cell_off[r]."""
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
    table: object = None                      # route="table": the RegionTable behind the four per-region sequences
    cell_prob_rows: Optional[np.ndarray] = None


# ---- the table route (DESIGN K25) ---------------------------------------------------------------------------------------
_FNV_OFFSET, _FNV_PRIME = 0xCBF29CE484222325, 0x100000001B3


def region_tokens(chr_names, chr_i, ordinal):
    """fnv1a64("<chr>-region_<ordinal>") of every region as a uint64 array: the prefix is hashed once per chromosome, the
    ordinal's decimal digits (at most ten: ordinals below 10^10) take one step each over the whole array."""
    chr_i, ordinal = np.asarray(chr_i, dtype=np.int64), np.asarray(ordinal, dtype=np.int64)
    if ordinal.size and (int(ordinal.min()) < 0 or int(ordinal.max()) >= 10 ** 10):
        raise ValueError("region ordinals must be in 0 .. 10^10 - 1")
    prefix = np.array([fnv1a64(f"{c}-region_") for c in chr_names], dtype=np.uint64)
    h = prefix[chr_i] if ordinal.size else np.zeros(0, dtype=np.uint64)
    n_digits = np.searchsorted(10 ** np.arange(1, 10, dtype=np.int64), ordinal, side="right") + 1
    prime = np.uint64(_FNV_PRIME)
    with np.errstate(over="ignore"):
        for step in range(int(n_digits.max()) if ordinal.size else 0):
            live = n_digits > step
            digit = (ordinal // 10 ** np.maximum(n_digits - 1 - step, 0)) % 10
            h = np.where(live, (h ^ (digit + 48).astype(np.uint64)) * prime, h)
    return h


def _ranges(start, count):
    """concatenate([arange(s, s + c) for s, c in zip(start, count)]) without the loop."""
    start, count = np.asarray(start, dtype=np.int64), np.asarray(count, dtype=np.int64)
    end = np.cumsum(count)
    return np.arange(int(end[-1]) if end.size else 0, dtype=np.int64) + np.repeat(start - (end - count), count)


@dataclass
class RegionTable:
    """The predicted CNV regions of a run as arrays, one entry per region in report order (cell group, then gene).  groups:
    [(name, 0-based cell indices)] in report order; chr_names: chromosomes in order of first appearance; perm: the gene gather
    of chr_layout(), or None; col: index into groups; chr: index into chr_names; gene_first / gene_count: the run in the
    gathered gene order; row_first: its first row in the object's own gene order (the run is contiguous there too); state: the
    HMM state, -1 for the invalid state; ordinal: the counter of the region's name "<chr>-region_<ordinal>"; token: fnv1a64 of
    that name; cell_idx[cell_off[r] : cell_off[r + 1]]: the region's cells, ascending.  source: the table this one was
    taken from by take() (the regions the step-17 reports hold), else None."""
    groups: list
    chr_names: np.ndarray
    perm: Optional[np.ndarray]
    col: np.ndarray
    chr: np.ndarray
    gene_first: np.ndarray
    gene_count: np.ndarray
    row_first: np.ndarray
    state: np.ndarray
    ordinal: np.ndarray
    token: np.ndarray
    cell_off: np.ndarray
    cell_idx: np.ndarray
    source: object = None

    def __len__(self):
        return int(self.col.size)

    @staticmethod
    def from_records(groups, chr_names, perm, rec):
        """rec: the six int64 record arrays of device.cnv_runs (col, chr, gene_first, gene_last, state with 255 for the
        invalid state, ordinal)."""
        col, chr_i, first, last, state, ordinal = (np.asarray(r, dtype=np.int64) for r in rec)
        count = last - first + 1
        if perm is None:
            row_first = first.copy()
        else:                                   # a run must stay one run of rows in the object's own order
            perm = np.asarray(perm, dtype=np.int64)
            breaks = np.concatenate([[0], np.cumsum(np.diff(perm) != 1)])
            bad = np.nonzero(breaks[last] != breaks[first])[0]
            if bad.size:
                name = f"{chr_names[chr_i[bad[0]]]}-region_{ordinal[bad[0]]}"
                raise ValueError(f"region {name}: its genes must be one contiguous run of rows (order the object by chromosome)")
            row_first = perm[first]
        sizes = np.fromiter((len(g) for _, g in groups), dtype=np.int64, count=len(groups))
        members = (np.concatenate([np.asarray(g, dtype=np.int64).ravel() for _, g in groups]) if len(groups)
                   else np.zeros(0, dtype=np.int64))
        owner = np.repeat(np.arange(len(groups), dtype=np.int64), sizes)
        members = members[np.lexsort((members, owner))]          # every group's cells ascending
        g_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        n_cells = sizes[col] if col.size else np.zeros(0, dtype=np.int64)
        cell_off = np.concatenate([[0], np.cumsum(n_cells)]).astype(np.int64)
        cell_idx = members[_ranges(g_off[col], n_cells)].astype(np.int32) if col.size else np.zeros(0, dtype=np.int32)
        return RegionTable(groups=groups, chr_names=np.asarray(chr_names), perm=perm, col=col, chr=chr_i, gene_first=first,
                           gene_count=count, row_first=row_first, state=np.where(state == 255, -1, state), ordinal=ordinal,
                           token=region_tokens(chr_names, chr_i, ordinal), cell_off=cell_off, cell_idx=cell_idx)

    @staticmethod
    def from_states(infercnv_obj, HMM_states, by, normal):
        """The regions inferCNVBayesNet samples: the runs of get_predicted_CNV_regions(states, by) whose state is not `normal`.
        The states go to the device once as uint8 (as generate_cnv_region_reports sends them); group modes segment the groups'
        consensus columns, by = "cell" the cells' own columns with every byte outside 1 .. 6 as the invalid state."""
        import torch
        groups = cnv_regions._cell_groups(infercnv_obj, by)
        by_cell = by == "cell" and infercnv_obj.tumor_subclusters is not None
        perm, chr_start = infercnv_obj.chr_layout()
        chrs = np.asarray(infercnv_obj.gene_order.chr)
        resident = isinstance(HMM_states, DeviceMatrix)     # (DESIGN K32: the states are on the device already)
        if resident:
            n_cells = HMM_states.shape[1]
            if perm is not None:
                chrs = chrs[perm]
        else:
            st = np.asarray(HMM_states)
            st = np.asfortranarray(np.where(st < 0, 255, st).astype(np.uint8))
            if perm is not None:                    # the kernels see contiguous chromosomes only
                st, chrs = np.asfortranarray(st[perm]), chrs[perm]
            if by_cell:
                st = np.asfortranarray(np.where((st >= 1) & (st <= 6), st, 255).astype(np.uint8))
            n_cells = st.shape[1]
        rec = np.zeros((6, 0), dtype=np.int64)
        if n_cells and groups:
            dev_states = cnv_regions._states_dev(HMM_states, perm, by_cell) if resident else torch.from_numpy(st.T).cuda()
            if by_cell:
                mat, col_idx = dev_states, np.concatenate([g for _, g in groups]).astype(np.int32)
            else:
                mat, col_idx = device.state_consensus(dev_states, [g for _, g in groups]), None
            rec = device.cnv_runs(mat, chr_start, neutral=int(normal), K=0, col_idx=col_idx)[0].cpu().numpy()
        return RegionTable.from_records(groups, chrs[chr_start[:-1]], perm, rec)

    def take(self, keep, state=None):
        """The regions `keep` (a boolean mask or ascending indices), optionally with new states."""
        idx = np.nonzero(keep)[0] if np.asarray(keep).dtype == bool else np.asarray(keep, dtype=np.int64)
        n_cells = np.diff(self.cell_off)[idx]
        cells = self.cell_idx[_ranges(self.cell_off[:-1][idx], n_cells)] if idx.size else self.cell_idx[:0]
        return replace(self, col=self.col[idx], chr=self.chr[idx], gene_first=self.gene_first[idx], gene_count=self.gene_count[idx],
                       row_first=self.row_first[idx], state=(self.state if state is None else np.asarray(state, dtype=np.int64))[idx],
                       ordinal=self.ordinal[idx], token=self.token[idx],
                       cell_off=np.concatenate([[0], np.cumsum(n_cells)]).astype(np.int64), cell_idx=cells,
                       source=self if self.source is None else self.source)

    def name(self, r):
        return f"{self.chr_names[self.chr[r]]}-region_{self.ordinal[r]}"

    def cell_gene(self, r):
        rows = np.arange(self.gene_first[r], self.gene_first[r] + self.gene_count[r], dtype=np.int64)
        if self.perm is not None:
            rows = self.perm[rows]
        return {"cnv_regions": self.name(r), "Genes": rows, "Cells": self.cell_idx[self.cell_off[r]:self.cell_off[r + 1]].astype(np.int64),
                "State": int(self.state[r])}

    def group_id(self, n_obs):
        """Per cell below n_obs the 1-based number of its cell group among the groups that have a region (NA_INTEGER elsewhere)."""
        has = np.zeros(len(self.groups), dtype=bool)
        has[self.col] = True
        number = np.cumsum(has)
        out = np.full(n_obs, NA_INTEGER, dtype=np.int64)
        which = np.nonzero(has)[0]
        if which.size:
            sizes = np.fromiter((len(self.groups[g][1]) for g in which), dtype=np.int64, count=which.size)
            cells = np.concatenate([np.asarray(self.groups[g][1], dtype=np.int64).ravel() for g in which])
            gid = np.repeat(number[which], sizes)
            sel = cells < n_obs
            out[cells[sel]] = gid[sel]          # groups in report order: where two share a cell the later one stays
        return out


class _LazySeq(Sequence):
    """A read-only sequence whose element i is make(i), built when it is asked for (cnv_regions._RegionList is the precedent)."""

    def __init__(self, n, make):
        self._n, self._make = int(n), make

    def __len__(self):
        return self._n

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self._make(k) for k in range(*i.indices(self._n))]
        i = operator.index(i)
        if i < 0:
            i += self._n
        if not 0 <= i < self._n:
            raise IndexError("region index out of range")
        return self._make(i)


def _attach_table(obj: "MCMCInferCNV", table: RegionTable):
    obj.table = table
    obj.cnv_regions = _LazySeq(len(table), table.name)
    obj.cell_gene = _LazySeq(len(table), table.cell_gene)


def run_mcmc_table(obj: "MCMCInferCNV") -> "MCMCInferCNV":
    """run_mcmc on obj.table: the same two device calls, fed from the table's arrays."""
    a, t = obj.args, obj.table
    K = len(obj.mu)
    R = len(t)
    if R == 0:
        obj.cnv_probabilities, obj.cell_probabilities, obj.cnv_means = _LazySeq(0, None), _LazySeq(0, None), np.zeros((K, 0))
        obj.cell_prob_rows = np.zeros((0, K))
        return obj
    _, L, off = device.bayes_loglik_arrays(obj.x_dev, t.row_first, t.gene_count, t.cell_idx, t.cell_off, obj.mu, obj.sig)
    theta_sum, samples, freq = device.bayes_sample(L, off, t.token, a["n_adapt"], a["n_burn"], a["n_keep"], a["seed"],
                                                   want_samples=a["keep_samples"])
    theta_sum = theta_sum.cpu().numpy()
    freq = freq.cpu().numpy()
    n = float(K * a["n_keep"])
    tot = np.zeros((R, K))
    for ch in range(K):                        # the chain sums in chain order, one division
        tot = tot + theta_sum[:, ch, :]
    obj.cnv_means = (tot / n).T.copy()
    samples = samples.cpu().numpy() if samples is not None else None
    obj.cnv_probabilities = _LazySeq(R, (lambda r: samples[r].reshape(-1, K)) if samples is not None else (lambda r: None))
    rows = freq.astype(np.float64) / n
    obj.cell_prob_rows = rows
    obj.cell_probabilities = _LazySeq(R, lambda r: rows[off[r]:off[r + 1]].T.copy())
    return obj


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
                     i3_p_val=0.05, mu=None, sig=None, x=None, *, route="dict") -> MCMCInferCNV:
    """inferCNVBayesNet (R/inferCNV_BayesNet.R:1237-1364).  infercnv_obj: the object the HMM ran on (its expr_data are the
    values the mixture model sees); HMM_states: the genes x cells state matrix of step 17 (1..K).  The regions are those of
    cnv_regions.get_predicted_CNV_regions(states, by) without the neutral state -- what initializeObject / getGenesCells
    (:245-338) read back from the step-17 report files.  mu / sig default to mean_sd(); x: the (C, G) CUDA matrix when it is
    already on the device.  keep_samples: also keep every theta sample (K n_keep x K per region).
    route: "dict" builds one Python object per region; "table" (DESIGN K25) keeps the regions as the arrays of a RegionTable
    (obj.table) -- cnv_regions, cell_gene, cell_probabilities and cnv_probabilities are then read-only sequences whose
    elements, equal to the dict route's, are built when they are indexed.  postMcmcMethod = "removeCells" needs the dict route."""
    import torch
    if HMM_type not in ("i6", "i3"):
        raise ValueError("HMM_type must be i6 or i3")
    if route not in ("dict", "table"):
        raise ValueError("route must be dict or table")
    normal = _normal_state(HMM_type)
    if route == "table" and postMcmcMethod == "removeCells":
        raise ValueError('postMcmcMethod = "removeCells" is not built on the table route: use route="dict"')
    obj = MCMCInferCNV(infercnv_obj=infercnv_obj)
    obj.args = {"HMM_type": HMM_type, "postMcmcMethod": postMcmcMethod, "reassignCNVs": bool(reassignCNVs), "out_dir": out_dir,
                "BayesMaxPNormal": 0, "seed": int(seed), "n_adapt": int(n_adapt), "n_burn": int(n_burn), "n_keep": int(n_keep),
                "keep_samples": bool(keep_samples), "by": by}
    n_obs = max((int(np.max(v)) + 1 for v in infercnv_obj.observation_grouped_cell_indices.values() if len(v)), default=0)
    if route == "table":
        _attach_table(obj, RegionTable.from_states(infercnv_obj, HMM_states, by, normal))
        obj.group_id = obj.table.group_id(n_obs)
    else:
        st_obj = infercnv_obj.copy()
        st_obj.expr_data = HMM_states if isinstance(HMM_states, DeviceMatrix) else np.asarray(HMM_states).astype(np.float64)
        groups = cnv_regions.get_predicted_CNV_regions(st_obj, by)
        cells_all = infercnv_obj.cells()
        col_of = {str(c): i for i, c in enumerate(cells_all)}
        group_id = np.full(n_obs, NA_INTEGER, dtype=np.int64)
        gid = 0
        for grp in groups:
            cols = np.sort(np.array([col_of[str(c)] for c in grp["cells"]], dtype=np.int64))
            kept = [(rn, r) for rn, r in grp["gene_regions"] if r["state"] != normal]
            if not kept:
                continue
            gid += 1                            # unique(pred_cnv_genes_df$cell_group_name): groups with a region, in file order
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
    if x is not None:
        obj.x_dev = x
    elif isinstance(infercnv_obj.expr_data, DeviceMatrix):
        obj.x_dev = infercnv_obj.expr_data.tensor
    else:
        obj.x_dev = torch.from_numpy(np.ascontiguousarray(np.asarray(infercnv_obj.expr_data, dtype=np.float64).T)).cuda()
    return run_mcmc_table(obj) if route == "table" else run_mcmc(obj)


# ---- step 19 ----------------------------------------------------------------------------------------------------------
class _NoStates:
    """kept_regions' stand-in for _States: the filter's decisions are taken and no matrix is rewritten."""

    def fill(self, genes, cells, value):
        pass

    def result(self):
        return None


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


def _remove_cnv(obj: MCMCInferCNV, st: _States, write=True):
    """removeCNV (R/inferCNV_BayesNet.R:562-630): strictly above the threshold; a region without cells (NaN) stays.
    write: also rewrite CNV_State_Probabilities.dat (kept_regions leaves the file to the filter)."""
    normal = _normal_state(obj.args["HMM_type"])
    thr = obj.args["BayesMaxPNormal"]
    p_normal = obj.cnv_means[normal - 1] if obj.cnv_means.size else np.zeros(0)
    remove = np.nonzero(p_normal > thr)[0]
    if remove.size == 0:
        return obj
    for i in remove:
        st.fill(obj.cell_gene[i]["Genes"], obj.cell_gene[i]["Cells"], normal)
    mask = np.ones(len(obj.cell_gene), dtype=bool)
    mask[remove] = False
    keep = np.nonzero(mask)[0].tolist()
    obj.cell_gene = [obj.cell_gene[i] for i in keep]
    obj.cnv_regions = [obj.cnv_regions[i] for i in keep]
    obj.cell_probabilities = [obj.cell_probabilities[i] for i in keep]
    obj.cnv_probabilities = [obj.cnv_probabilities[i] for i in keep]
    obj.cnv_means = obj.cnv_means[:, keep]
    if write:
        _write_state_probabilities(obj.args.get("out_dir"), [cg["cnv_regions"] for cg in obj.cell_gene], obj.cnv_means)
    return obj


def _write_state_probabilities(out_dir, names, cnv_means):
    if out_dir is None:
        return
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "CNV_State_Probabilities.dat"), "w") as fh:   # write.table(row.names = TRUE): no corner cell
        fh.write("\t".join(names) + "\n")
        for k in range(cnv_means.shape[0]):
            fh.write("\t".join([f"State:{k + 1}"] + [cnv_regions._fmt(float(v)) if v == v else "NaN" for v in cnv_means[k]]) + "\n")


def _decide_table(mcmc_obj: MCMCInferCNV, BayesMaxPNormal, write=True):
    """The decisions of filterHighPNormals on the table route, as array expressions: removeCNV's -- strictly above the
    threshold, a NaN column stays and keeps its HMM state -- and reassignCNV's -- the first maximum is the new state.
    -> (the filtered object, value): value[r] is the byte device.fill_regions writes over region r of mcmc_obj.table -- the
    normal state for the removed regions, the new state for the kept ones when reassignCNVs is set, 0 (leave alone) otherwise;
    None when there is no postMcmcMethod.  write: also rewrite CNV_State_Probabilities.dat when a region was removed."""
    import copy
    obj = copy.copy(mcmc_obj)
    obj.args = dict(mcmc_obj.args, BayesMaxPNormal=BayesMaxPNormal)
    t = mcmc_obj.table
    method = obj.args.get("postMcmcMethod")
    if method is None:
        return obj, None
    if method != "removeCNV":
        raise ValueError('postMcmcMethod = "removeCells" is not built on the table route')
    normal = _normal_state(obj.args["HMM_type"])
    means = mcmc_obj.cnv_means
    R = len(t)
    remove = (means[normal - 1] > BayesMaxPNormal) if R else np.zeros(0, dtype=bool)   # NaN compares false: it stays
    value = np.where(remove, normal, 0).astype(np.uint8)
    state = t.state.copy()
    if obj.args.get("reassignCNVs") and R:
        moved = ~remove & ~np.isnan(means).any(axis=0)
        best = np.argmax(means, axis=0) + 1                      # the first maximum
        state[moved] = best[moved]
        value[moved] = best[moved]
    kept = np.nonzero(~remove)[0]
    _attach_table(obj, t.take(kept, state))
    obj.cnv_means = means[:, kept]
    cell_p, cnv_p = mcmc_obj.cell_probabilities, mcmc_obj.cnv_probabilities
    obj.cell_probabilities = _LazySeq(kept.size, lambda i: cell_p[int(kept[i])])
    obj.cnv_probabilities = _LazySeq(kept.size, lambda i: cnv_p[int(kept[i])])
    if mcmc_obj.cell_prob_rows is not None:
        obj.cell_prob_rows = mcmc_obj.cell_prob_rows[_ranges(t.cell_off[:-1][kept], np.diff(t.cell_off)[kept])]
    if write and remove.any():
        _write_state_probabilities(obj.args.get("out_dir"), list(obj.cnv_regions), obj.cnv_means)
    return obj, value


def _filter_table(mcmc_obj: MCMCInferCNV, HMM_states, BayesMaxPNormal):
    """filterHighPNormals on the table route: the decisions of _decide_table and ONE device.fill_regions call for every
    rectangle."""
    import torch
    t = mcmc_obj.table
    on_device = isinstance(HMM_states, torch.Tensor)
    if on_device and (not HMM_states.is_cuda or HMM_states.dim() != 2):
        raise TypeError("HMM_states: a genes x cells array or a (cells, genes) CUDA tensor")
    host = None if on_device else np.asarray(HMM_states)
    obj, value = _decide_table(mcmc_obj, BayesMaxPNormal)
    if value is None:
        return obj, (HMM_states.clone() if on_device else np.array(host))

    def fill(m):
        if value.any():
            device.fill_regions(m, t.row_first, t.gene_count, t.cell_off, t.cell_idx, value)
        return m

    if on_device and HMM_states.dtype == torch.uint8:
        return obj, fill(HMM_states.clone(memory_format=torch.contiguous_format))
    # any other element type: the rectangles are drawn on a zero uint8 matrix and laid over the input
    C, G = HMM_states.shape if on_device else host.shape[::-1]
    over = fill(torch.zeros((C, G), dtype=torch.uint8, device=HMM_states.device if on_device else "cuda"))
    if on_device:
        return obj, torch.where(over != 0, over.to(HMM_states.dtype), HMM_states)
    over = over.cpu().numpy().T
    out = np.array(host)
    hit = over != 0
    out[hit] = over[hit]
    return obj, out


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
    back.  The object passed in is not modified.  A DeviceMatrix of states (DESIGN K32) is a uint8 CUDA tensor in a wrapper:
    it is filtered as one and comes back wrapped."""
    if isinstance(HMM_states, DeviceMatrix):
        t = HMM_states.tensor if HMM_states.kind == "states" else cnv_regions._states_dev(HMM_states)
        obj, out = filterHighPNormals(mcmc_obj, t, BayesMaxPNormal)
        return obj, DeviceMatrix(out.contiguous(), "states")
    if mcmc_obj.table is not None:
        return _filter_table(mcmc_obj, HMM_states, BayesMaxPNormal)
    st = _States(HMM_states)
    return _filter_dict(mcmc_obj, st, BayesMaxPNormal), st.result()


def _filter_dict(mcmc_obj: MCMCInferCNV, st, BayesMaxPNormal, write=True):
    """filterHighPNormals' decisions on the dict route; the rectangles go to st (a _States, or _NoStates)."""
    import copy
    obj = copy.copy(mcmc_obj)
    obj.cell_gene = [dict(cg) for cg in mcmc_obj.cell_gene]
    obj.cnv_regions = list(mcmc_obj.cnv_regions)
    obj.args = dict(mcmc_obj.args, BayesMaxPNormal=BayesMaxPNormal)
    method = obj.args.get("postMcmcMethod")
    if method is not None:
        obj = _remove_cnv(obj, st, write) if method == "removeCNV" else _remove_cells(obj, st)
        if obj.args.get("reassignCNVs"):
            obj = _reassign_cnv(obj, st)
    return obj


def kept_regions(mcmc_obj: MCMCInferCNV, BayesMaxPNormal) -> MCMCInferCNV:
    """The MCMC object filterHighPNormals(mcmc_obj, states, BayesMaxPNormal)[0] returns -- the regions that stay, cell_gene with
    the reassigned State, their means and cell probabilities, args with the threshold -- derived without a state matrix
    (DESIGN K33): run() hands an on_step hook the MCMC object at step 18 and only the filtered HMM object at step 19.  Nothing
    is written; the object passed in is not modified."""
    if mcmc_obj.table is not None:
        return _decide_table(mcmc_obj, BayesMaxPNormal, write=False)[0]
    return _filter_dict(mcmc_obj, _NoStates(), BayesMaxPNormal, write=False)


# ---- convergence diagnostics of the chains (DESIGN K31) -----------------------------------------------------------------
MCMC_TABLE_FILE = "CNV_MCMC_Diagnostics.dat"
MCMC_TABLE_COLUMNS = ("Mean", "St.Dev", "2.5%", "50%", "97.5%", "Rhat", "ESS", "Geweke", "acf1", "acf5", "acf10", "acf50")
MCMC_DEVICE_TABLE_ROWS = 1 << 16          # a table of at least this many rows is formatted on the device (K20)


@dataclass
class McmcDiagnostics:
    """What mcmcDiagnosticPlots (R/inferCNV_BayesNet.R:866-990) takes from coda, as numbers (device.mcmc_diag; the library's
    own contract, modelled on coda: believed, not verified against it).  regions: the region names; chain_stats: (regions, K,
    n_chains, 9) host array, chain_fields per region, state and chain; pooled: (regions, K, 7), pooled_fields per region and
    state.  States keep R's numbering: index k is state k + 1."""
    regions: Sequence
    chain_stats: np.ndarray
    pooled: np.ndarray
    chain_fields: tuple = device.MCMC_CHAIN_FIELDS
    pooled_fields: tuple = device.MCMC_POOLED_FIELDS

    def table(self):
        """The (regions * K, 12) matrix of CNV_MCMC_Diagnostics.dat: MCMC_TABLE_COLUMNS per (region, state) -- R's
        CNVSummaryTablels columns, then Rhat and ESS, then Geweke and the autocorrelations of chain 0."""
        R, K = self.pooled.shape[:2]
        return np.concatenate([self.pooled.reshape(R * K, -1), self.chain_stats[:, :, 0, 4:].reshape(R * K, -1)], axis=1)

    def row_names(self):
        K = self.pooled.shape[1]
        return [f"{name}:State:{k + 1}" for name in self.regions for k in range(K)]


def write_mcmc_diagnostics(diag: McmcDiagnostics, out_dir, device_rows=MCMC_DEVICE_TABLE_ROWS):
    """CNV_MCMC_Diagnostics.dat in out_dir: write.table(sep = "\\t", quote = FALSE) of diag.table() with R's number formatting.
    A small table goes through heatmap.write_table; from device_rows rows on the numbers are formatted on the device and
    streamed (heatmap.write_matrix, DESIGN K20): the bytes are the same."""
    os.makedirs(out_dir, exist_ok=True)
    return _write_tsv(os.path.join(out_dir, MCMC_TABLE_FILE), diag.table(), diag.row_names(), MCMC_TABLE_COLUMNS, device_rows)


def _write_tsv(path, tab, names, columns, device_rows):
    """write.table(sep = "\\t", quote = FALSE) of the matrix tab with R's number formatting: through heatmap.write_table, and
    from device_rows rows on formatted on the device and streamed (heatmap.write_matrix, DESIGN K20).  The bytes are the same."""
    import torch
    from . import heatmap
    if 0 < device_rows <= tab.shape[0]:
        x = torch.from_numpy(np.ascontiguousarray(tab)).cuda()
        heatmap.write_matrix(path, x, np.arange(tab.shape[0], dtype=np.int32), "cell_rows", row_names=names,
                             col_names=columns, quote=False, sep="\t")
    else:
        heatmap.write_table(path, tab.tolist(), row_names=names, col_names=columns, quote=False, sep="\t")
    return path


def _resample(obj: MCMCInferCNV, lo, hi):
    """The kept theta samples of the regions lo .. hi - 1, (hi - lo, K, n_keep, K) on the device: the likelihoods again from
    obj.x_dev, the sampler again with the object's schedule, seed and tokens.  Every draw has its own counter and a region's
    chains do not depend on the other regions of a call, so these are the samples of the run itself."""
    a = obj.args
    if obj.table is not None:
        t = obj.table
        c0, c1 = int(t.cell_off[lo]), int(t.cell_off[hi])
        _, L, off = device.bayes_loglik_arrays(obj.x_dev, t.row_first[lo:hi], t.gene_count[lo:hi], t.cell_idx[c0:c1],
                                               t.cell_off[lo:hi + 1] - c0, obj.mu, obj.sig)
        tokens = t.token[lo:hi]
    else:
        cgs = [obj.cell_gene[r] for r in range(lo, hi)]
        regions = [_gene_run(cg["Genes"], cg["cnv_regions"]) + (np.asarray(cg["Cells"], dtype=np.int32),) for cg in cgs]
        _, L, off = device.bayes_loglik(obj.x_dev, regions, obj.mu, obj.sig)
        tokens = [fnv1a64(cg["cnv_regions"]) for cg in cgs]
    return device.bayes_sample(L, off, tokens, a["n_adapt"], a["n_burn"], a["n_keep"], a["seed"], want_samples=True)[1]


def _sample_batches(mcmc_obj: MCMCInferCNV, max_sample_bytes):
    """(lo, hi, samples) over the object's regions in order: the kept theta samples of the regions lo .. hi - 1 as a
    (hi - lo, K, n_keep, K) CUDA tensor, in batches that fit max_sample_bytes (K n_keep K doubles per region; at least one
    region per batch).  The held samples of a keep_samples = True object are uploaded; else the regions are sampled again
    (_resample).  The caller drops a batch before it asks for the next."""
    import torch
    K, n_keep, R = len(mcmc_obj.mu), int(mcmc_obj.args["n_keep"]), len(mcmc_obj.cnv_regions)
    batch = max(1, int(max_sample_bytes) // (K * n_keep * K * 8))
    held = R > 0 and mcmc_obj.cnv_probabilities[0] is not None
    for lo in range(0, R, batch):
        hi = min(R, lo + batch)
        if held:
            host = np.stack([np.asarray(mcmc_obj.cnv_probabilities[r], dtype=np.float64).reshape(K, n_keep, K) for r in range(lo, hi)])
            yield lo, hi, torch.from_numpy(host).to(mcmc_obj.x_dev.device)
        else:
            yield lo, hi, _resample(mcmc_obj, lo, hi)


def mcmc_diagnostics(mcmc_obj: MCMCInferCNV, *, max_sample_bytes=2 << 30, out_dir=None) -> McmcDiagnostics:
    """Convergence diagnostics of every region's chains (DESIGN K31): R-hat, effective sample size, Geweke scores,
    autocorrelations and the pooled quantiles, as a table one can filter -- the data under mcmcDiagnosticPlots' PDFs.
    mcmc_obj: what inferCNVBayesNet returned (either route), or filterHighPNormals' object.  keep_samples is not needed: the
    regions are sampled again in batches whose kept samples fit max_sample_bytes (K n_keep K doubles per region; at least one
    region per batch), and device.mcmc_diag runs on each batch; the result does not depend on the batching.  An object that
    holds its samples (keep_samples = True) is not sampled again.  out_dir: also write CNV_MCMC_Diagnostics.dat there."""
    K, R = len(mcmc_obj.mu), len(mcmc_obj.cnv_regions)
    cs = np.empty((R, K, K, len(device.MCMC_CHAIN_FIELDS)))
    po = np.empty((R, K, len(device.MCMC_POOLED_FIELDS)))
    for lo, hi, samples in _sample_batches(mcmc_obj, max_sample_bytes):
        c, p = device.mcmc_diag(samples)
        cs[lo:hi], po[lo:hi] = c.cpu().numpy(), p.cpu().numpy()
        del samples
    diag = McmcDiagnostics(regions=list(mcmc_obj.cnv_regions) if R <= MCMC_DEVICE_TABLE_ROWS else mcmc_obj.cnv_regions,
                           chain_stats=cs, pooled=po)
    rhat, ess = po[:, :, 5], po[:, :, 6]
    with np.errstate(invalid="ignore"):
        n_bad = int((rhat >= 1.1).any(axis=1).sum()) if R else 0
    min_ess = float(np.nanmin(ess)) if R and not np.isnan(ess).all() else float("nan")
    log.info("MCMC diagnostics: %d regions, %d with a state of Rhat >= 1.1, smallest ESS %.6g", R, n_bad, min_ess)
    if out_dir is not None:
        write_mcmc_diagnostics(diag, out_dir)
    return diag


# ---- the probability heatmaps and tables (DESIGN K33) -------------------------------------------------------------------
def _region_arrays(obj: MCMCInferCNV):
    """(first row, row count, cell_off, cell_idx) of the object's regions in the object's own gene order, as arrays."""
    if obj.table is not None:
        t = obj.table
        return t.row_first, t.gene_count, t.cell_off, t.cell_idx
    runs = [_gene_run(cg["Genes"], cg["cnv_regions"]) for cg in obj.cell_gene]
    cells = [np.asarray(cg["Cells"], dtype=np.int32).ravel() for cg in obj.cell_gene]
    off = np.concatenate([[0], np.cumsum([c.size for c in cells])]).astype(np.int64)
    return (np.array([r[0] for r in runs], dtype=np.int32), np.array([r[1] for r in runs], dtype=np.int32), off,
            np.concatenate(cells) if cells else np.zeros(0, dtype=np.int32))


def _region_names(obj: MCMCInferCNV):
    """The region names as one array of strings (the table route's are put together chromosome-wise, not one by one)."""
    if obj.table is not None:
        t = obj.table
        if len(t) == 0:
            return np.zeros(0, dtype=str)
        return np.char.add(np.char.add(np.asarray(t.chr_names).astype(str)[t.chr], "-region_"), t.ordinal.astype(str))
    return np.array([str(n) for n in obj.cnv_regions], dtype=str)


def normal_probability_matrix(mcmc_obj: MCMCInferCNV):
    """postProbNormal's matrix (R/inferCNV_BayesNet.R:763-774) as a (C, G) CUDA float64 tensor: 0 everywhere, then
    1 - cnv_means[normal state, r] (one rounded subtraction) over region r's genes x cells, regions in order -- where two
    overlap the later one stays -- in one device.paint_regions call (DESIGN K33)."""
    import torch
    normal = _normal_state(mcmc_obj.args["HMM_type"])
    means = np.asarray(mcmc_obj.cnv_means, dtype=np.float64)
    value = 1.0 - means[normal - 1] if means.size else np.zeros(0)
    G, C = mcmc_obj.infercnv_obj.expr_data.shape
    dev = mcmc_obj.x_dev.device if mcmc_obj.x_dev is not None else "cuda"
    out = torch.empty((C, G), dtype=torch.float64, device=dev)
    g0, ng, off, idx = _region_arrays(mcmc_obj)
    return device.paint_regions(out, g0, ng, off, idx, value)


def _plots_off(args):
    return bool(args.get("no_plot")) or args.get("plotingProbs") is False


def postProbNormal(mcmc_obj: MCMCInferCNV, title, output_filename, out_dir=None, useRaster=True):
    """postProbNormal (R/inferCNV_BayesNet.R:757-788): the heatmap of 1 - P(normal) of every region, through heatmap.plot_cnv
    on a copy of the object's infercnv object whose expr_data is normal_probability_matrix() as a DeviceMatrix, with R's
    arguments (k_obs_groups and cluster_by_groups from the object's args, write_expr_matrix = FALSE, x.center = 0,
    x.range = c(0, 1)).  out_dir defaults to the object's args["out_dir"].  Writes what plot_cnv writes for them and returns
    its settings; writes nothing and returns None when the object's args hold no_plot (or plotingProbs = False)."""
    from . import heatmap
    a = mcmc_obj.args
    if _plots_off(a):
        return None
    out_dir = a.get("out_dir") if out_dir is None else out_dir
    if out_dir is None:
        raise ValueError("postProbNormal: no out_dir, neither given nor in the object's args")
    plot_obj = mcmc_obj.infercnv_obj.copy()
    plot_obj.expr_data = DeviceMatrix(normal_probability_matrix(mcmc_obj), "expr")
    return heatmap.plot_cnv(plot_obj, out_dir=out_dir, k_obs_groups=a.get("k_obs_groups", 1),
                            cluster_by_groups=a.get("cluster_by_groups", True), title=title, output_filename=output_filename,
                            write_expr_matrix=False, x_center=0, x_range=(0, 1), useRaster=useRaster)


BOX_TABLE_COLUMNS = device.BOX_FIELDS


def _r_threshold(v):
    """sprintf("%s", BayesMaxPNormal)."""
    if isinstance(v, (bool, np.bool_)):
        return "TRUE" if v else "FALSE"
    if isinstance(v, (float, np.floating)):
        return "%.15g" % v
    return str(v)


@dataclass
class CnvProbabilities:
    """What plotProbabilities (R/inferCNV_BayesNet.R:808-844) draws, as numbers.  regions: the region names; box: (regions, K,
    7) host array, device.BOX_FIELDS of the pooled kept theta draws per region and state (plot_cnv_prob's box plot;
    device.theta_box: the library's own contract, modelled on ggplot2's stat_boxplot: believed, not verified against it);
    cell_off / cell_idx: region r's cells are cell_idx[cell_off[r] : cell_off[r + 1]] in the region's order; cell_probs:
    (cell_off[-1], K), per (region, cell) its state frequencies over all chains' kept draws (plot_cell_prob's stacked bar);
    cell_names: the names of all cells of the object; threshold: the object's BayesMaxPNormal (None: unset).  States keep R's
    numbering: index k is state k + 1."""
    regions: Sequence
    box: np.ndarray
    cell_off: np.ndarray
    cell_idx: np.ndarray
    cell_probs: np.ndarray
    cell_names: np.ndarray
    threshold: object = None
    box_fields: tuple = device.BOX_FIELDS

    def file_names(self):
        """(cnvProbs.<p>.dat, cellProbs.<p>.dat): R's PDF names (:819-836) with the tables' extension."""
        p = "" if self.threshold is None else "." + _r_threshold(self.threshold)
        return f"cnvProbs{p}.dat", f"cellProbs{p}.dat"

    def cnv_table(self):
        R, K = self.box.shape[:2]
        return self.box.reshape(R * K, -1)

    def cnv_row_names(self):
        K = self.box.shape[1]
        state = np.char.add(":State:", np.arange(1, K + 1).astype(str))
        return np.char.add(np.repeat(np.asarray(self.regions, dtype=str), K), np.tile(state, len(self.regions)))

    def cell_columns(self):
        return tuple(f"State:{k + 1}" for k in range(self.cell_probs.shape[1]))

    def cell_row_names(self):
        region = np.repeat(np.asarray(self.regions, dtype=str), np.diff(self.cell_off))
        return np.char.add(np.char.add(region, ":"), np.asarray(self.cell_names).astype(str)[self.cell_idx])


def write_cnv_probabilities(probs: CnvProbabilities, out_dir, device_rows=MCMC_DEVICE_TABLE_ROWS):
    """cnvProbs.<p>.dat -- one row <region>:State:<k> per (region, state), columns device.BOX_FIELDS -- and cellProbs.<p>.dat --
    one row <region>:<cell name> per (region, cell), columns State:1 .. State:K -- in out_dir, tab-separated with R's number
    formatting, through the writers of write_mcmc_diagnostics.  Returns the two paths."""
    os.makedirs(out_dir, exist_ok=True)
    cnv_name, cell_name = probs.file_names()
    return (_write_tsv(os.path.join(out_dir, cnv_name), probs.cnv_table(), probs.cnv_row_names(), BOX_TABLE_COLUMNS, device_rows),
            _write_tsv(os.path.join(out_dir, cell_name), probs.cell_probs, probs.cell_row_names(), probs.cell_columns(), device_rows))


def plotProbabilities(mcmc_obj: MCMCInferCNV, out_dir=None, *, max_sample_bytes=2 << 30,
                      device_rows=MCMC_DEVICE_TABLE_ROWS) -> CnvProbabilities:
    """plotProbabilities (R/inferCNV_BayesNet.R:808-844) as data (DESIGN K33): per region the box statistics of every state's
    pooled kept theta draws (device.theta_box) and every cell's state probabilities.  mcmc_obj: what inferCNVBayesNet returned
    (either route), or a filtered object (kept_regions, filterHighPNormals) -- R plots the filtered one.  The samples come as
    mcmc_diagnostics gets them: the held ones of a keep_samples = True object, else the regions are sampled again in batches
    that fit max_sample_bytes; the result does not depend on the batching.  out_dir: also write cnvProbs.<p>.dat and
    cellProbs.<p>.dat there (write_cnv_probabilities; nothing is written when the object's args hold no_plot).  The PDFs stay
    in R."""
    K, R = len(mcmc_obj.mu), len(mcmc_obj.cnv_regions)
    box = np.empty((R, K, len(device.BOX_FIELDS)))
    for lo, hi, samples in _sample_batches(mcmc_obj, max_sample_bytes):
        box[lo:hi] = device.theta_box(samples).cpu().numpy()
        del samples
    _, _, off, idx = _region_arrays(mcmc_obj)
    if mcmc_obj.table is not None and mcmc_obj.cell_prob_rows is not None:
        cell_probs = mcmc_obj.cell_prob_rows
    else:
        parts = [np.asarray(mcmc_obj.cell_probabilities[r], dtype=np.float64).T for r in range(R)]
        cell_probs = np.concatenate(parts) if parts else np.zeros((0, K))
    probs = CnvProbabilities(regions=_region_names(mcmc_obj), box=box, cell_off=np.asarray(off, dtype=np.int64),
                             cell_idx=np.asarray(idx, dtype=np.int64), cell_probs=np.ascontiguousarray(cell_probs),
                             cell_names=np.asarray(mcmc_obj.infercnv_obj.cells()), threshold=mcmc_obj.args.get("BayesMaxPNormal"))
    log.info("CNV and cell probabilities: %d regions, %d (region, cell) rows", R, probs.cell_probs.shape[0])
    if out_dir is not None and not _plots_off(mcmc_obj.args):
        write_cnv_probabilities(probs, out_dir, device_rows)
    return probs
