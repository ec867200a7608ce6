"""The hidden spike-in of the i6 HMM (DESIGN K15): .build_and_add_hspike of R/inferCNV_hidden_spike.R:3-165 with
sim_method = "meanvar", step 3 of run() (R/inferCNV_ops.R:586-590).  The hspike is a small simulated data set of normal and
CNV-spiked cells over eleven fake chromosomes; get_spike_dists and get_hspike_cnv_mean_sd_trend_by_num_cells_fit (hmm.py)
and the Bayesian filter (bayes_net.py) read their emission parameters from it.

The group gene tables (icnv_group_gene_tables_dev) and the simulation (icnv_hspike_simulate_dev) run on the device; the two
smoothing splines between them are fitted on the host (smooth_spline.py).  The object must hold the depth-normalised,
not yet log-transformed matrix, as in run() (step 3 precedes the log2(x + 1) of step 4).

Where R draws unseeded the library has its own documented stream (restated in tests/hspike_restate.py):
  genes_means_use_idx[j] = floor(G u_j), u_j the first .random() draw of NumPy's
      Generator(Philox(key = [seed, ICNV_HSPIKE_GENES_TOKEN], counter = [2, j, 0, 0]))   (R: sample(, replace = TRUE));
  the token of a matrix = fnv1a64("simnorm_cell_<type>") for the normal cells and fnv1a64("spike_tumor_cell_<type>") for
      the spiked ones -- the name prefixes of its cells, the way K10 derives a token from a clade's name.
Deviations from R, all documented in include/icnv.h: an all-zero simulated row stays as it is (R divides by zero), and the
nls logistic fit of .get_logistic_params is not built (R computes it and never reads it on this route).
"""
from __future__ import annotations

import numpy as np

from . import _lib, device, ops
from .hmm import HSPIKE_CHR_INFO
from .infercnv_object import DeviceMatrix, GeneOrder, InfercnvObject
from .smooth_spline import smooth_spline
from .tumor_subclusters import fnv1a64

NUM_CELLS = 100            # cells per simulated matrix (R/inferCNV_hidden_spike.R:32)
NUM_GENES_PER_CHR = 400    # :33


def get_hspike_chr_info(num_genes_each, num_total):
    """.get_hspike_chr_info (R/inferCNV_hidden_spike.R:170-215): [(name, cnv, ngenes)] of the eleven fake chromosomes; the last
    one receives max(num_total - 10 num_genes_each, num_genes_each) genes."""
    remaining = max(int(num_total) - 10 * int(num_genes_each), int(num_genes_each))
    last = len(HSPIKE_CHR_INFO) - 1
    return [(name, cnv, remaining if k == last else int(num_genes_each)) for k, (name, cnv) in enumerate(HSPIKE_CHR_INFO)]


def _table_groups(infercnv_obj):
    """c(observation groups, reference groups) (.get_mean_var_table, R/inferCNV_meanVarSim.R:180); without references the
    one 'normalsToUse' group of all observation cells (infercnv_obj_tmp, R/inferCNV_hidden_spike.R:20-25)."""
    obs = [np.asarray(v, dtype=np.int32) for v in infercnv_obj.observation_grouped_cell_indices.values()]
    if not infercnv_obj.has_reference_cells():
        return [np.concatenate(obs)]
    return obs + [np.asarray(v, dtype=np.int32) for v in infercnv_obj.reference_grouped_cell_indices.values()]


def _device_matrix(expr):
    """genes x cells host matrix -> the (C, G) CUDA tensor of the same bytes; a DeviceMatrix is there already."""
    import torch
    if isinstance(expr, DeviceMatrix):
        return expr.tensor
    return torch.from_numpy(np.ascontiguousarray(np.asarray(expr, dtype=np.float64).T)).cuda()


def _group_tables(infercnv_obj, x=None):
    """(m, v, p0) host arrays (n_groups, G) over _table_groups, one device call."""
    groups = _table_groups(infercnv_obj)
    x = _device_matrix(infercnv_obj.expr_data) if x is None else x
    m, v, nzero = device.group_gene_tables(x, groups)
    n = np.array([len(g) for g in groups], dtype=np.float64)[:, None]
    return m.cpu().numpy(), v.cpu().numpy(), nzero.cpu().numpy().astype(np.float64) / n


def get_mean_var_table(infercnv_obj, x=None):
    """.get_mean_var_table (R/inferCNV_meanVarSim.R:178-211): (m, v), each (n_groups, G), rows in c(observation, reference)
    order.  x: the matrix already on the device, (C, G)."""
    m, v, _ = _group_tables(infercnv_obj, x)
    return m, v


def get_mean_vs_p0_table(infercnv_obj, x=None):
    """.get_mean_vs_p0_table (R/inferCNV_simple_sim.R:100-154): (m, p0), p0 = the fraction of zeros."""
    m, _, p0 = _group_tables(infercnv_obj, x)
    return m, p0


def fit_splines(m, v, p0):
    """The two smoothing splines of a build: log(v + 1) over log(m + 1) on every (group, gene) row
    (R/inferCNV_meanVarSim.R:27-30) and p0 over log(m) on the rows with m > 0 (.get_logistic_params,
    R/inferCNV_simple_sim.R:190-218).  A non-finite value -- the NaN variance of a one-cell group -- raises ValueError, as R
    stops in smooth.spline."""
    m, v, p0 = (np.asarray(a, dtype=np.float64).ravel() for a in (m, v, p0))
    with np.errstate(invalid="ignore", divide="ignore"):
        var_spline = smooth_spline(np.log(m + 1.0), np.log(v + 1.0))
        pos = m > 0
        p0_spline = smooth_spline(np.log(m[pos]), p0[pos])
    return var_spline, p0_spline


def get_simulated_cell_matrix_using_meanvar_trend(infercnv_obj, gene_means, num_cells, seed=0, token=0, splines=None):
    """.get_simulated_cell_matrix_using_meanvar_trend(include.dropout = TRUE) (R/inferCNV_meanVarSim.R:1-19): a genes x
    num_cells host matrix simulated from gene_means with the object's mean-variance and dropout trends.  splines: the
    (variance, p0) pair of fit_splines when the caller has it already."""
    if splines is None:
        splines = fit_splines(*_group_tables(infercnv_obj))
    out = device.hspike_simulate(np.asarray(gene_means, dtype=np.float64)[None, :], num_cells, splines[0], splines[1], seed, [token])
    return np.asfortranarray(out[0].cpu().numpy().T)


def genes_means_use_idx(num_genes_orig, num_genes, seed=0):
    """The library's sample(seq_len(G), size = num_genes, replace = TRUE), 0-based (module docstring)."""
    out = np.empty(int(num_genes), dtype=np.int64)
    key = np.array([int(seed) & (2**64 - 1), _lib.HSPIKE_GENES_TOKEN], dtype=np.uint64)
    for j in range(int(num_genes)):
        bg = np.random.Philox(key=key, counter=np.array([2, j, 0, 0], dtype=np.uint64))
        out[j] = int(np.floor(float(num_genes_orig) * float(np.random.Generator(bg).random())))
    return out


def build_and_add_hspike(infercnv_obj: InfercnvObject, sim_method="meanvar", aggregate_normals=False, seed=0) -> InfercnvObject:
    """.build_and_add_hspike (R/inferCNV_hidden_spike.R:3-165): returns the object with `hspike` set.  Per normal cell type
    100 simulated normal cells (reference group "simnorm_cell_<type>") and 100 cells simulated from the gene means times
    the fake chromosomes' CNV factors (observation group "spike_tumor_cell_<type>"), all 2 n_types matrices in one launch;
    then normalize_counts_by_seq_depth to median(colSums) of the LAST normal type's cells (R's loop variable leaks, :160)."""
    if sim_method not in ("meanvar", "simple", "splatter"):
        raise ValueError("'arg' should be one of 'meanvar', 'simple', 'splatter'")
    if sim_method != "meanvar":
        raise NotImplementedError(f"sim_method {sim_method!r} is not built: only 'meanvar' (run()'s choice) is")
    if infercnv_obj.has_reference_cells():
        if aggregate_normals:
            normals = {"normalsToUse": infercnv_obj.get_reference_grouped_cell_indices()}
        else:
            normals = {k: np.asarray(v, dtype=np.int32) for k, v in infercnv_obj.reference_grouped_cell_indices.items()}
    else:
        normals = {"normalsToUse": np.concatenate([np.asarray(v, dtype=np.int32)
                                                   for v in infercnv_obj.observation_grouped_cell_indices.values()])}
    G = infercnv_obj.expr_data.shape[0]
    chr_info = get_hspike_chr_info(NUM_GENES_PER_CHR, G)
    chrs = np.concatenate([np.repeat(name, n) for name, _, n in chr_info])
    pos = np.concatenate([np.arange(1, n + 1) for _, _, n in chr_info])
    cnv = np.concatenate([np.repeat(float(c), n) for _, c, n in chr_info])
    num_genes = chrs.size
    use_idx = genes_means_use_idx(G, num_genes, seed)

    x = _device_matrix(infercnv_obj.expr_data)
    # the tables and the splines are the same for every simulated matrix of a build: once
    m, v, p0 = _group_tables(infercnv_obj, x)
    var_spline, p0_spline = fit_splines(m, v, p0)
    normal_means = device.group_means(x, list(normals.values())).cpu().numpy()   # rowMeans per normal type, (n_types, G)

    means, tokens, cell_names, ref_idx, obs_idx = [], [], [], {}, {}
    counter = 0
    for k, normal_type in enumerate(normals):
        gene_means = normal_means[k][use_idx].copy()
        gene_means[gene_means == 0] = 1e-3                       # "just make small nonzero values" (:65)
        for prefix, mu, dest in (("simnorm_cell_", gene_means, ref_idx), ("spike_tumor_cell_", np.where(cnv != 1, gene_means * cnv, gene_means), obs_idx)):
            name = prefix + str(normal_type)
            means.append(mu)
            tokens.append(fnv1a64(name))
            cell_names += [f"{name}{i}" for i in range(1, NUM_CELLS + 1)]
            dest[name] = np.arange(counter, counter + NUM_CELLS, dtype=np.int32)
            counter += NUM_CELLS
    sim = device.hspike_simulate(np.vstack(means), NUM_CELLS, var_spline, p0_spline, seed, tokens, device=x.device)
    if isinstance(infercnv_obj.expr_data, DeviceMatrix):
        # a resident object gets a resident spike-in: the simulated counts stay where the launch wrote them (DESIGN K32)
        counts = DeviceMatrix(sim.reshape(-1, num_genes).contiguous())
    else:
        counts = np.asfortranarray(sim.reshape(-1, num_genes).cpu().numpy().T)    # genes x (2 n_types 100) cells

    hspike = InfercnvObject(expr_data=counts, count_data=counts, gene_order=GeneOrder(chrs, pos.copy(), pos.copy()),
                            reference_grouped_cell_indices=ref_idx, observation_grouped_cell_indices=obs_idx,
                            gene_names=np.array([f"gene_{j}" for j in range(1, num_genes + 1)]), cell_names=np.array(cell_names))
    hspike.validate()
    last = _rows(x, list(normals.values())[-1])
    target = float(np.median(device.col_sums(last).cpu().numpy()))               # median(colSums(normal_cells_expr)) (:160)
    hspike = ops.normalize_counts_by_seq_depth(hspike, target)
    out = infercnv_obj.copy()
    out.hspike = hspike
    return out


def _rows(x, cells):
    """The rows `cells` of the (C, G) device matrix as a contiguous tensor."""
    import torch
    return x[torch.as_tensor(np.asarray(cells, dtype=np.int64), device=x.device)].contiguous()
