"""Host-side mirror of the distance step of the reference's subclustering
(R/inferCNV_tumor_subclusters.R:180-194: `hclust(parallelDist(t(tumor_expr_data)))`): the Euclidean distances
between the cells of one tumor group, computed on the GPU (icnv_cell_distances_dev) bit-equal to R's sequential dist:
per pair the fp64 sum over the genes in order of the rounded squares of the rounded differences of the raw values, then
sqrt.  Identical cells (step 22 makes many) are at distance exactly 0, so tied merges resolve as R's do.

The Leiden route's neighbour search (R/inferCNV_tumor_subclusters.R:646-741, RANN::nn2) is the exact kNN of
icnv_knn_dev (DESIGN K8): `nn2`, `snn_adjacency`, `knn_per_chr`, with the reference-based gene filter of :45-71.

The hierarchical clustering itself, `hclust(parallelDist(t(x)), method = hclust_method)` (:191, 582, 609 and the other
call sites of DESIGN K9), runs on the GPU too, on the same exact distances: `hclust` returns R's hclust object without the
distance matrix ever leaving the device.

The random-trees subclustering (R/inferCNV_tumor_subclusters.random_smoothed_trees.R, DESIGN K10) runs its permutation
statistic on the GPU (icnv_random_trees_dev), one call per recursion level: `define_signif_tumor_subclusters_via_random_smooothed_trees`,
with the recursion itself in the pure-Python `random_trees_partition`.

The reference's default Leiden route, leiden_method = "PCA" (.leiden_seurat_preprocess_routine, :699-723, DESIGN K18), runs
its variable-feature statistic, scaling, Gram matrix, projection, SNN graph and weighted Leiden on the GPU (`pca_stages`,
`leiden_seurat_preprocess_routine`); the trend fit (loess_fit.py) and the eigenpairs of the at most 2000 x 2000 Gram matrix
(numpy.linalg.eigh) are host work."""
from __future__ import annotations

import logging
from dataclasses import dataclass

import numpy as np

from . import _lib, device
from .infercnv_object import DeviceMatrix, InfercnvObject
from .loess_fit import loess_fit, window_points

log = logging.getLogger("infercnv_amd")


def parallelDist(infercnv_obj: InfercnvObject, cells, as_dist: bool = True):
    """parallelDist(t(expr.data[, cells]), method="euclidean").

    as_dist=True returns the R `dist` object's vector (lower triangle in column order == SciPy's condensed
    form); False the full symmetric (n, n) matrix."""
    import torch
    cells = np.asarray(cells, dtype=np.int32)
    if cells.ndim != 1 or cells.size < 1:
        raise ValueError("cells must be a non-empty index vector")
    d = device.cell_distances(_to_device(infercnv_obj), cells).cpu().numpy()
    if not as_dist:
        return d
    iu = np.triu_indices(cells.size, k=1)
    return d[iu]


# ------------------------------------------------------------------ Leiden subclustering: the kNN (DESIGN K8)
def _r_mean(v):
    """R's mean() of a double vector (summary.c): a long-double sum divided by n, then the mean of the residuals added."""
    v = np.asarray(v, dtype=np.float64).ravel()
    n = v.size
    s = np.sum(v, dtype=np.longdouble) / n
    t = np.sum(v.astype(np.longdouble) - s, dtype=np.longdouble)
    return float(s + t / n)


def _r_sd(v):
    """R's sd(): sqrt of the two-pass variance around R's mean, long-double accumulation, n - 1 denominator."""
    v = np.asarray(v, dtype=np.float64).ravel()
    m = _r_mean(v)
    d = v.astype(np.longdouble) - m
    return float(np.sqrt(float(np.sum(d * d, dtype=np.longdouble) / (v.size - 1))))


def zscore_outlier_genes(infercnv_obj: InfercnvObject, z_score_filter: float = 0.8):
    """The reference-based gene filter of define_signif_tumor_subclusters (R/inferCNV_tumor_subclusters.R:45-71): with
    z_score_filter > 0 and reference cells, z = (ref - mean(ref)) / sd(ref) over the whole reference matrix and the genes
    whose mean |z| is >= 0.8 (the literal; z_score_filter only switches the filter on).  Returns the outliers' 0-based
    row numbers (ascending), or None when the filter does not apply.
    A device-resident object (DeviceMatrix) takes the statistics from the device (device.zscore_gene_filter, DESIGN K32:
    double-double sums rounded once, where this host code follows R's long-double sums -- a row mean may differ by an ulp);
    only the G-byte decision crosses."""
    if not (z_score_filter > 0 and infercnv_obj.has_reference_cells()):
        return None
    if isinstance(infercnv_obj.expr_data, DeviceMatrix):
        import torch
        _, _, row_mean = device.zscore_gene_filter(infercnv_obj.expr_data.tensor, infercnv_obj.get_reference_grouped_cell_indices())
        return torch.nonzero(row_mean >= 0.8).flatten().cpu().numpy().astype(np.int64)
    x = np.asarray(infercnv_obj.expr_data, dtype=np.float64)
    ref = x[:, infercnv_obj.get_reference_grouped_cell_indices()]
    m, s = _r_mean(ref), _r_sd(ref)
    z = np.abs((ref - m) / s)
    row_mean = np.array([_r_mean(z[g]) for g in range(z.shape[0])])
    return np.flatnonzero(row_mean >= 0.8).astype(np.int64)


def zscore_kept_genes(infercnv_obj: InfercnvObject, z_score_filter: float = 0.8):
    """The rows of expr.data the subclustering goes on with (R/inferCNV_tumor_subclusters.R:45-71).  When the filter applies
    and finds no outlier, R's `expr.data[-outliers, ]` with `outliers = integer(0)` keeps NO row: mirrored as such."""
    G = infercnv_obj.expr_data.shape[0]
    out = zscore_outlier_genes(infercnv_obj, z_score_filter)
    if out is None:
        return np.arange(G, dtype=np.int64)
    if out.size == 0:
        return np.zeros(0, dtype=np.int64)
    return np.setdiff1d(np.arange(G, dtype=np.int64), out)


def _to_device(infercnv_obj):
    import torch
    if isinstance(infercnv_obj.expr_data, DeviceMatrix):       # resident: the tensor itself, nothing crosses (states: as float64)
        return infercnv_obj.expr_data.float_tensor()
    x = np.asarray(infercnv_obj.expr_data, dtype=np.float64)
    return torch.from_numpy(np.ascontiguousarray(x.T)).cuda()


def nn2(infercnv_obj: InfercnvObject, cells, k: int, genes=None):
    """RANN::nn2(t(expr.data[genes, cells]), k = k) with query = data (R/inferCNV_tumor_subclusters.R:726), exact on the GPU.
    Returns (nn_idx, nn_dists) as numpy arrays of shape (len(cells), k); nn_idx holds 0-based positions in `cells`
    (R's nn.idx is 1-based).  Exactly equal distances are ordered by position (RANN's order among them is its tree walk)."""
    cells = np.asarray(cells, dtype=np.int32)
    G = infercnv_obj.expr_data.shape[0]
    genes = np.arange(G, dtype=np.int32) if genes is None else np.asarray(genes, dtype=np.int32)
    if cells.ndim != 1 or genes.ndim != 1:
        raise ValueError("cells and genes must be index vectors")
    idx, dist = device.knn(_to_device(infercnv_obj), [(genes, cells)], k)
    return idx.cpu().numpy(), dist.cpu().numpy()


def snn_adjacency(nn_idx):
    """sparseMatrix(i = rep(1:n, each = k), j = t(snn), x = 1, dims = c(n, n)) of .leiden_simple_snn
    (R/inferCNV_tumor_subclusters.R:728-734) as a SciPy CSR matrix (0-based, not symmetrised: igraph's mode = "undirected"
    does that in R)."""
    from scipy.sparse import csr_matrix
    nn_idx = np.asarray(nn_idx)
    n, k = nn_idx.shape
    rows = np.repeat(np.arange(n), k)
    return csr_matrix((np.ones(n * k), (rows, nn_idx.ravel())), shape=(n, n))


def knn_per_chr(infercnv_obj: InfercnvObject, tumor_groups, k_nn: int, z_score_filter: float = 0.8, chr_levels=None):
    """The kNN of .whole_dataset_leiden_subclustering_per_chr (R/inferCNV_tumor_subclusters.R:646-697) with
    leiden_method_per_chr = "simple": for every chromosome level x tumor group, nn2 over the z-score-filtered genes of the
    chromosome (:45-71), all of them in ONE batched device call.

    tumor_groups: {name: 0-based cell indices}.  chr_levels: levels(chrs) (default: the chromosomes of the unfiltered
    gene order, in order of appearance).  Returns (results, skipped): results[(chr, group)] = (nn_idx, nn_dists) as nn2
    returns them; skipped[(chr, group)] = the reason R keeps the group as it is:
      "absent"     no filtered gene on the chromosome (R: the whole column range, :654-656)
      "too_few"    ncol < 3 (:661-664)
      "k_nn"       k_nn >= ncol (:665-668)"""
    chr_all = np.asarray(infercnv_obj.gene_order.chr).astype(str)
    kept = zscore_kept_genes(infercnv_obj, z_score_filter)
    chrs = chr_all[kept]
    if chr_levels is None:
        _, first = np.unique(chr_all, return_index=True)
        chr_levels = chr_all[np.sort(first)]
    present = set(chrs.tolist())
    problems, keys, skipped = [], [], {}
    for c in chr_levels:
        genes_c = kept[chrs == c].astype(np.int32)
        for name, cells in tumor_groups.items():
            cells = np.asarray(cells, dtype=np.int32)
            if c not in present:
                skipped[(c, name)] = "absent"
            elif cells.size < 3:
                skipped[(c, name)] = "too_few"
            elif k_nn >= cells.size:
                skipped[(c, name)] = "k_nn"
            else:
                problems.append((genes_c, cells))
                keys.append((c, name))
    results = {}
    if problems:
        idx, dist = device.knn(_to_device(infercnv_obj), problems, k_nn)
        idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
        r0 = 0
        for key, (_, cells) in zip(keys, problems):
            results[key] = (idx[r0:r0 + cells.size], dist[r0:r0 + cells.size])
            r0 += cells.size
    return results, skipped


# ------------------------------------------------------------------ hierarchical clustering (DESIGN K9)
@dataclass
class HClust:
    """The fields of R's hclust object (stats::hclust, as fastcluster::hclust returns it): merge (n-1, 2) int32 with
    singletons -(i+1) and clusters by step, height (n-1,), order (n,) 1-based, labels (the cells), method, dist_method."""
    merge: np.ndarray
    height: np.ndarray
    order: np.ndarray
    labels: np.ndarray
    method: str
    dist_method: str = "euclidean"


def hclust(infercnv_obj: InfercnvObject, cells, method: str = "ward.D2", genes=None):
    """hclust(parallelDist(t(expr.data[genes, cells])), method = method) as the subclustering calls it
    (R/inferCNV_tumor_subclusters.R:191, 582, 609; R/inferCNV_ops.R:1930, 3242), on the GPU (icnv_hclust_cells_dev).
    genes: 0-based rows (default all; the z-score-filtered genes of :45-71 come from `zscore_kept_genes`).  labels are the
    cells' column names (InfercnvObject.cells())."""
    cells = np.asarray(cells, dtype=np.int32)
    G = infercnv_obj.expr_data.shape[0]
    genes = np.arange(G, dtype=np.int32) if genes is None else np.asarray(genes, dtype=np.int32)
    if cells.ndim != 1 or genes.ndim != 1:
        raise ValueError("cells and genes must be index vectors")
    (merge, height, order), = device.hclust_cells(_to_device(infercnv_obj), [(genes, cells)], method)
    labels = np.asarray(infercnv_obj.cells())[cells]
    return HClust(merge.cpu().numpy(), height.cpu().numpy(), order.cpu().numpy(), labels, method)


def redo_hierarchical_clustering(infercnv_obj: InfercnvObject, hclust_method) -> InfercnvObject:
    """.redo_hierarchical_clustering (R/inferCNV_ops.R:3231-3249; step 17 of run() after a random_trees partition): every
    group's `hc` replaced by hclust(parallelDist(t(expr.data[, cells]))) of all its subclusters' cells sorted by index -- one
    K9 batch over the groups."""
    ts = infercnv_obj.tumor_subclusters
    groups = {g: np.sort(np.concatenate([np.asarray(v, dtype=np.int64).ravel() for v in subs.values()]))
              for g, subs in ts["subclusters"].items()}
    for g, c in groups.items():
        if c.size < 2:   # R's hclust stops: "must have n >= 2 objects to cluster"
            raise ValueError(f"group {g!r} has {c.size} cell(s): must have n >= 2 objects to cluster")
    genes = np.arange(infercnv_obj.expr_data.shape[0], dtype=np.int32)
    res = device.hclust_cells(_to_device(infercnv_obj), [(genes, c.astype(np.int32)) for c in groups.values()], hclust_method)
    cell_names = np.asarray(infercnv_obj.cells())
    out = infercnv_obj.copy()
    hc = dict(ts.get("hc") or {})
    for (g, c), (merge, height, order) in zip(groups.items(), res):
        hc[g] = HClust(merge.cpu().numpy(), height.cpu().numpy(), order.cpu().numpy(), cell_names[c], hclust_method)
    out.tumor_subclusters = dict(ts, hc=hc)
    return out


# ------------------------------------------------------------------ random-trees subclustering (DESIGN K10)
RANDOM_TREES_ITERATIONS = 100   # num_rand_iters (R/inferCNV_tumor_subclusters.random_smoothed_trees.R:254)


def fnv1a64(name: str) -> int:
    """FNV-1a-64 of the UTF-8 bytes of a clade name: the clade's token, the second key word of its permutation stream."""
    h = 0xCBF29CE484222325
    for b in str(name).encode("utf-8"):
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def cutree_h(merge, height, h):
    """cutree(tree, h = h) (stats::cutree / R_cutree): k = n + 1 - which.max(c(height, Inf) > h) groups, numbered 1.. in order
    of first appearance among the cells."""
    merge = np.asarray(merge)
    height = np.asarray(height, dtype=np.float64)
    n = merge.shape[0] + 1
    k = n - int(np.flatnonzero(np.append(height, np.inf) > h)[0])
    parent = np.arange(2 * n - 1)

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for step in range(n - k):   # the first n - k merges
        for v in merge[step]:
            node = -int(v) - 1 if v < 0 else n + int(v) - 1
            parent[find(node)] = n + step
    labels = np.zeros(n, dtype=np.int64)
    seen = {}
    for c in range(n):
        labels[c] = seen.setdefault(find(c), len(seen) + 1)
    return labels


def random_trees_pvalue(max_height: float, rand_max_heights) -> float:
    """1 - ecdf(rand)(max_height) as R evaluates it (:148-156, 291): 1 - (#{rand <= max_height} / n) in doubles; 1 when the
    observed tree is flat (max_height == 0)."""
    rand = np.asarray(rand_max_heights, dtype=np.float64)
    if not max_height > 0:
        return 1.0
    return 1.0 - int(np.count_nonzero(rand <= max_height)) / rand.size


def random_trees_partition(groups, clade_fn, p_val, max_recursion_depth=3, min_cluster_size_recurse=10):
    """The recursion of the random-trees subclustering (R/inferCNV_tumor_subclusters.random_smoothed_trees.R:3-67, 118-213)
    for every tumor group at once, one `clade_fn` call per recursion level.

    groups: {group: 0-based cell indices} in R's order.  clade_fn(list of (clade name, cell indices)) -> one
    ((merge, height, order), rand_max_heights) per clade: the clade's observed tree in R's format and the maximum heights of
    its permuted trees.  Returns (hc, subclusters): hc[group] = the level-1 observed tree, subclusters[group][name] = the
    group's cells of the final clade `name` in their original order, names sorted (split(grps, grps), C-locale order)."""
    groups = {g: np.asarray(c, dtype=np.int64) for g, c in groups.items()}
    for g, c in groups.items():
        if c.size < 2:   # R stops in apply() / hclust
            raise ValueError(f"tumor group {g!r} has {c.size} cell(s): at least two are needed to cluster")
    names = {g: np.array([f"{g}.1"] * c.size, dtype=object) for g, c in groups.items()}
    pending = [(g, np.arange(c.size), f"{g}.1") for g, c in groups.items()]
    hc = {}
    depth = 1
    while pending and depth <= max_recursion_depth:
        results = clade_fn([(name, groups[g][pos]) for g, pos, name in pending])
        nxt = []
        for (g, pos, name), ((merge, height, order), rand) in zip(pending, results):
            height = np.asarray(height, dtype=np.float64)
            if depth == 1:
                hc[g] = (merge, height, order)
            max_height = float(np.max(height))
            if random_trees_pvalue(max_height, rand) > p_val:
                continue                                      # "No cluster pruning"
            cut = _r_mean(height[-2:])                        # mean(c(h[n-1], h[n-2])); one value when n == 2
            labels = cutree_h(merge, height, cut)
            sizes = np.bincount(labels)[1:]
            if np.all(sizes < min_cluster_size_recurse):    # none big enough: the clade keeps its name
                continue
            for grp in range(1, sizes.size + 1):
                sub = pos[labels == grp]
                sub_name = f"{name}.{grp}"
                names[g][sub] = sub_name
                if sub.size >= min_cluster_size_recurse:
                    nxt.append((g, sub, sub_name))
        pending = nxt
        depth += 1
    subclusters = {}
    for g, c in groups.items():
        subclusters[g] = {nm: c[names[g] == nm] for nm in sorted(set(names[g].tolist()))}
    return hc, subclusters


def random_trees_groups(infercnv_obj: InfercnvObject, cluster_by_groups):
    """The tumor groups of the random-trees subclustering (:15-26): every observation and reference group, or
    all_observations (the observation groups' cells concatenated) and the reference groups."""
    obs = {k: np.asarray(v, dtype=np.int64) for k, v in infercnv_obj.observation_grouped_cell_indices.items()}
    ref = {k: np.asarray(v, dtype=np.int64) for k, v in infercnv_obj.reference_grouped_cell_indices.items()}
    if cluster_by_groups:
        return {**obs, **ref}
    allobs = np.concatenate(list(obs.values())) if obs else np.zeros(0, dtype=np.int64)
    return {"all_observations": allobs, **ref}


def define_signif_tumor_subclusters_via_random_smooothed_trees(infercnv_obj: InfercnvObject, p_val, hclust_method,
                                                               cluster_by_groups, window_size=101, max_recursion_depth=3,
                                                               min_cluster_size_recurse=10, seed=0):
    """tumor_subcluster_partition_method = "random_trees" (R/inferCNV_tumor_subclusters.random_smoothed_trees.R:3-67; run()
    step 7, R/inferCNV_ops.R:716-730) on the GPU: every recursion level of every group in one icnv_random_trees_dev call.

    The statistic works on subtract_ref_expr_from_obs(infercnv_obj, inv_log=TRUE); the returned copy keeps the input's
    expr_data and gets tumor_subclusters = {"hc": {group: HClust}, "subclusters": {group: {name: cell indices}}}.
    The null trees come from the library's own stream (icnv.h, K10): NumPy's Philox keyed by (seed, FNV-1a-64 of the clade
    name); R's is unseeded and thread-dependent.  The hspike mirror uses seed + 1."""
    import torch
    from . import ops
    work = infercnv_obj.copy()
    work.hspike = None
    sub = ops.subtract_ref_expr_from_obs(work, inv_log=True)
    groups = random_trees_groups(infercnv_obj, cluster_by_groups)
    x = []   # the subtracted matrix on the device, uploaded by the first level

    def clade_fn(clades):
        if not x:
            x.append(_to_device(sub))
        trees, rand = device.random_trees(x[0], [c for _, c in clades], [fnv1a64(n) for n, _ in clades], window_size,
                                          RANDOM_TREES_ITERATIONS, seed, hclust_method)
        rand = rand.cpu().numpy()
        return [((m.cpu().numpy(), h.cpu().numpy(), o.cpu().numpy()), rand[i]) for i, (m, h, o) in enumerate(trees)]

    hc, subclusters = random_trees_partition(groups, clade_fn, p_val, max_recursion_depth, min_cluster_size_recurse)
    cell_names = np.asarray(infercnv_obj.cells())
    out = infercnv_obj.copy()
    out.tumor_subclusters = {
        "hc": {g: HClust(m, h, o, cell_names[groups[g]], hclust_method) for g, (m, h, o) in hc.items()},
        "subclusters": subclusters,
    }
    if infercnv_obj.hspike is not None:
        # "-mirroring for hspike" (:49-54), with the reference's positional slip: its call binds cluster_by_groups =
        # window_size, window_size = max_recursion_depth and max_recursion_depth = min_cluster_size_recurse
        out.hspike = define_signif_tumor_subclusters_via_random_smooothed_trees(
            infercnv_obj.hspike, p_val, hclust_method, window_size, max_recursion_depth, min_cluster_size_recurse,
            seed=seed + 1)
    return out


# ------------------------------------------------------------------ Leiden subclustering (DESIGN K11)
LEIDEN_BETA = 0.01          # cluster_leiden's beta (R igraph default)
LEIDEN_ITERATIONS = 2       # cluster_leiden's n_iterations (R igraph default)


def auto_leiden_resolution(n: int) -> float:
    """leiden_resolution = "auto": (11.98 / ncol)^(1 / 1.165) (R/inferCNV_tumor_subclusters.R:583-586, 673-676)."""
    return (11.98 / n) ** (1 / 1.165)


def _device_leiden(seed):
    def fn(nn_idx, sizes, objective, gammas, tokens):
        memb, _ = device.leiden(nn_idx, sizes, objective, gammas, LEIDEN_BETA, LEIDEN_ITERATIONS, seed, tokens)
        return memb.cpu().numpy()
    return fn


def cluster_leiden(nn_idx, resolution_parameter, objective_function="CPM", beta=LEIDEN_BETA, n_iterations=LEIDEN_ITERATIONS,
                   seed=0, token=0):
    """cluster_leiden(graph, resolution_parameter, objective_function)$membership on the graph of one (n, k) nn_idx block
    (.leiden_simple_snn, R/inferCNV_tumor_subclusters.R:733-739) by icnv_leiden_dev: a 1-based numpy int32 vector.  The
    partition follows the library's contract (include/icnv.h, K11), not igraph's RNG."""
    import torch
    nn = nn_idx if isinstance(nn_idx, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(nn_idx, dtype=np.int32))
    nn = nn.to(device="cuda", dtype=torch.int32).contiguous()
    memb, _ = device.leiden(nn, [nn.shape[0]], objective_function, resolution_parameter, beta, n_iterations, seed, [token])
    return memb.cpu().numpy()


def leiden_simple_snn(infercnv_obj: InfercnvObject, cells, k_nn, resolution_parameter, objective_function="CPM", genes=None,
                      seed=0, token=0):
    """.leiden_simple_snn(expr.data[genes, cells], k_nn, resolution_parameter, objective_function)
    (R/inferCNV_tumor_subclusters.R:725-741): the exact kNN (K8) and the Leiden partition (K11), both on the GPU."""
    cells = np.asarray(cells, dtype=np.int32)
    G = infercnv_obj.expr_data.shape[0]
    genes = np.arange(G, dtype=np.int32) if genes is None else np.asarray(genes, dtype=np.int32)
    idx, _ = device.knn(_to_device(infercnv_obj), [(genes, cells)], k_nn)
    return cluster_leiden(idx, resolution_parameter, objective_function, seed=seed, token=token)


def _check_leiden_args(leiden_method, leiden_function, partition_method, restrict_to_DE_genes):
    if restrict_to_DE_genes:
        raise NotImplementedError("restrict_to_DE_genes = TRUE (.find_DE_stat_significance) is not implemented")
    if partition_method in ("qnorm", "pheight", "qgamma"):
        raise NotImplementedError(f'partition_method = "{partition_method}" is not implemented')
    if partition_method not in ("leiden", "none"):
        raise ValueError(f"unknown partition_method {partition_method!r}")
    if leiden_method not in ("PCA", "simple"):
        raise ValueError(f"unknown leiden_method {leiden_method!r}")
    if leiden_function not in ("CPM", "modularity"):
        raise ValueError(f"unknown leiden_function {leiden_function!r}")


def _resolution(leiden_resolution, n):
    return auto_leiden_resolution(n) if isinstance(leiden_resolution, str) and leiden_resolution == "auto" else float(leiden_resolution)


# ------------------------------------------------------------------ the PCA route of the Leiden subclustering (DESIGN K18)
PCA_NFEATURES = 2000        # FindVariableFeatures' nfeatures
PCA_NPCS = 10               # RunPCA(npcs = 10) (:711)
FALLBACK_MESSAGE = "Got a warning:\n\t%s\n\nFalling back to simple Leiden clustering for this chromosome.\n"   # :704


def vst_trend_sd(mean, var):
    """The expected standard deviation of FindVariableFeatures' "vst" for one problem's genes: sqrt(10^fit) of the local
    quadratic trend of log10(var) on log10(mean) (loess_fit.py) over the genes with var > 0, 0 elsewhere.  Returns (sd_e, None),
    or (None, reason) when the reference's FindVariableFeatures would warn and the route falls back.  A mean <= 0 among the
    fitted genes is a ValueError (R's loess stops on the NaN)."""
    mean = np.asarray(mean, dtype=np.float64)
    var = np.asarray(var, dtype=np.float64)
    pos = var > 0
    if np.any(mean[pos] <= 0):
        raise ValueError("a gene with positive variance has a mean <= 0: log10(mean) is not defined (R's loess stops)")
    m = int(np.count_nonzero(pos))
    q = window_points(m)
    if q < 4:
        return None, f"span is too small: {q} of {m} genes in a window"
    fit, ok = loess_fit(np.log10(mean[pos]), np.log10(var[pos]))
    if not ok:
        return None, "a window of the trend has fewer than 3 distinct means of positive weight"
    sd_e = np.zeros(mean.size, dtype=np.float64)
    sd_e[pos] = np.sqrt(np.power(10.0, fit))
    return sd_e, None


def select_features(v_std, nfeatures=PCA_NFEATURES):
    """head(order(-v_std), nfeatures): positions by decreasing v_std, ties by position."""
    v_std = np.asarray(v_std, dtype=np.float64)
    return np.argsort(-v_std, kind="stable")[:min(int(nfeatures), v_std.size)]


def top_eigenvectors(M, npcs):
    """The top `npcs` eigenvectors of the symmetric M (numpy.linalg.eigh on the host), by decreasing eigenvalue, each with its
    largest-magnitude entry positive (the first on ties): (values (npcs,), V (F, npcs))."""
    lam, vec = np.linalg.eigh(np.asarray(M, dtype=np.float64))
    lam, vec = lam[::-1][:npcs], vec[:, ::-1][:, :npcs]
    V = np.ascontiguousarray(vec)
    for j in range(V.shape[1]):
        if V[int(np.argmax(np.abs(V[:, j]))), j] < 0:
            V[:, j] = -V[:, j]
    return lam.copy(), V


def pca_stages(x, genes, cells, k_nn, timings=None):
    """Stages 1-4 of the PCA route (include/icnv.h, K18) for a batch of problems on the (C, G) device matrix x: problem p has
    the genes genes[p] (list order) and the cells cells[p]; x must be a CUDA tensor (there is no host route:
    NotImplementedError).  Returns a dict:
      active / fallback   the problems that went through / the (problem, reason) pairs that fall back to the simple route
    and, for the active problems in order (device tensors unless noted): mean, var (host, per problem over its genes), sd_e
    (host), v_std (host), features (host positions within genes[p]), Z, n_feat, n_cells, npcs, M, eigenvalues (host), V (host
    blocks), E, nn_idx, and the SNN graph row_off, col, shared, weight, loop.  timings: a dict that receives the wall
    milliseconds of every stage (each stage synchronises the device)."""
    import time
    import torch
    if not (isinstance(x, torch.Tensor) and x.is_cuda):
        # no quiet host route: every stage but the trend fit and the eigenpairs is a device kernel on the resident matrix
        raise NotImplementedError('leiden_method = "PCA" is implemented on the device-resident (cells, genes) matrix only; '
                                  'there is no host route (use "simple" likewise on the device, or partition_method = "none")')
    t_last = [time.perf_counter()]

    def lap(name):
        if timings is not None:
            torch.cuda.synchronize()
            now = time.perf_counter()
            timings[name] = timings.get(name, 0.0) + (now - t_last[0]) * 1e3
            t_last[0] = now

    P = len(cells)
    cells = [np.asarray(c, dtype=np.int32) for c in cells]
    genes = [np.asarray(g, dtype=np.int32) for g in genes]
    m_all, v_all, _ = device.group_gene_tables(x, cells)
    lap("moments")
    out = {"fallback": []}
    mean, var, sd_e = {}, {}, {}
    for p in range(P):
        gi = torch.from_numpy(genes[p].astype(np.int64)).to(x.device)
        mean[p] = m_all[p, gi].cpu().numpy()
        var[p] = v_all[p, gi].cpu().numpy()
        sd_e[p], why = vst_trend_sd(mean[p], var[p])
        if sd_e[p] is None:
            out["fallback"].append((p, why))
    failed = {p for p, _ in out["fallback"]}
    act = [p for p in range(P) if p not in failed]
    lap("trend_host")

    def dev(parts):
        return torch.from_numpy(np.ascontiguousarray(np.concatenate(parts), dtype=np.float64)).to(x.device)

    v_std, feats = {}, {}
    if act:
        packed = device.lpca_vstd(x, [(genes[p], cells[p]) for p in act], dev([mean[p] for p in act]),
                                  dev([sd_e[p] for p in act])).cpu().numpy()
        g0 = 0
        for p in act:
            v_std[p] = packed[g0:g0 + genes[p].size]
            g0 += genes[p].size
            feats[p] = select_features(v_std[p])
            if min(PCA_NPCS, feats[p].size - 1, cells[p].size - 1) < 1:
                out["fallback"].append((p, "fewer than 2 features or cells: no principal component"))
        failed = {p for p, _ in out["fallback"]}
        act = [p for p in act if p not in failed]
    lap("v_std_and_features")
    out["fallback"].sort()
    out["active"] = act
    out.update(mean=[mean[p] for p in act], var=[var[p] for p in act], sd_e=[sd_e[p] for p in act], v_std=[v_std[p] for p in act],
               features=[feats[p] for p in act])
    if not act:
        return out
    n_feat = [int(feats[p].size) for p in act]
    n_cells = [int(cells[p].size) for p in act]
    npcs = [min(PCA_NPCS, f - 1, n - 1) for f, n in zip(n_feat, n_cells)]
    Z = device.lpca_scale(x, [(genes[p][feats[p]], cells[p]) for p in act], dev([mean[p][feats[p]] for p in act]),
                          dev([np.sqrt(var[p][feats[p]]) for p in act]))
    lap("scale")
    M = device.lpca_gram(Z, n_feat, n_cells)
    lap("gram")
    lam, V, m0 = [], [], 0
    for f, c in zip(n_feat, npcs):
        l, v = top_eigenvectors(M[m0:m0 + f * f].reshape(f, f).cpu().numpy(), c)
        lam.append(l)
        V.append(v)
        m0 += f * f
    lap("eigh_host")
    E = device.lpca_project(Z, dev([v.ravel() for v in V]), n_feat, n_cells, npcs, PCA_NPCS)
    lap("project")
    rows = np.concatenate([[0], np.cumsum(n_cells)])
    nn_idx, _ = device.knn(E, [(np.arange(c, dtype=np.int32), np.arange(rows[i], rows[i + 1], dtype=np.int32))
                               for i, c in enumerate(npcs)], k_nn)
    lap("knn")
    row_off, col, shared, weight, loop = device.snn_jaccard(nn_idx, n_cells)
    lap("snn")
    out.update(Z=Z, n_feat=n_feat, n_cells=n_cells, npcs=npcs, M=M, eigenvalues=lam, V=V, E=E, nn_idx=nn_idx, row_off=row_off, col=col,
               shared=shared, weight=weight, loop=loop)
    return out


def _device_leiden_graph(seed):
    def fn(row_off, col, weight, loop, sizes, objective, gammas, tokens):
        memb, _ = device.leiden_graph(row_off, col, weight, loop, sizes, objective, gammas, LEIDEN_BETA, LEIDEN_ITERATIONS, seed, tokens)
        return memb.cpu().numpy()
    return fn


def _graph_resolution(objective, gamma):
    """CPM's resolution in units of the 24-bit fixed-point weights (an exact scaling); modularity's is homogeneous."""
    return gamma * _lib.SNN_WEIGHT_ONE if objective == "CPM" else gamma


def leiden_seurat_preprocess_routine(infercnv_obj: InfercnvObject, cells, k_nn, resolution_parameter, objective_function="CPM",
                                     genes=None, seed=0, token=0):
    """.leiden_seurat_preprocess_routine(expr.data[genes, cells], k_nn, resolution_parameter, objective_function)
    (R/inferCNV_tumor_subclusters.R:699-723) for one problem, by the library's contract (include/icnv.h, K18): a 1-based numpy
    int32 membership.  Falls back to `leiden_simple_snn` where the reference's FindVariableFeatures would warn."""
    cells = np.asarray(cells, dtype=np.int32)
    G = infercnv_obj.expr_data.shape[0]
    genes = np.arange(G, dtype=np.int32) if genes is None else np.asarray(genes, dtype=np.int32)
    return _leiden_problems(_to_device(infercnv_obj), [genes], [(cells, token)], k_nn, "PCA", objective_function, resolution_parameter,
                            _device_leiden(seed), _device_leiden_graph(seed))[0]


def _leiden_problems(x, genes, problems, k_nn, leiden_method, objective, leiden_resolution, leiden_fn, leiden_graph_fn=None):
    """One K8 call and one Leiden call for every (cells, token) problem: a list of 1-based partitions.  leiden_method "PCA":
    the batch goes through `pca_stages` and the weighted Leiden; the problems that fall back form a batch of the simple route."""
    if not problems:
        return []
    out = [None] * len(problems)
    simple = list(range(len(problems)))
    if leiden_method == "PCA":
        st = pca_stages(x, genes, [c for c, _ in problems], k_nn)
        for p, why in st["fallback"]:
            log.info(FALLBACK_MESSAGE, why)
        simple = [p for p, _ in st["fallback"]]
        act = st["active"]
        if act:
            sizes = st["n_cells"]
            gammas = [_graph_resolution(objective, _resolution(leiden_resolution, n)) for n in sizes]
            memb = leiden_graph_fn(st["row_off"], st["col"], st["weight"], st["loop"], sizes, objective, gammas,
                                   [problems[p][1] for p in act])
            r0 = 0
            for p, n in zip(act, sizes):
                out[p] = np.asarray(memb[r0:r0 + n])
                r0 += n
    if simple:
        idx, _ = device.knn(x, [(genes[p], problems[p][0]) for p in simple], k_nn)
        sizes = [problems[p][0].size for p in simple]
        memb = leiden_fn(idx, sizes, objective, [_resolution(leiden_resolution, n) for n in sizes], [problems[p][1] for p in simple])
        r0 = 0
        for p, n in zip(simple, sizes):
            out[p] = np.asarray(memb[r0:r0 + n])
            r0 += n
    return out


def define_signif_tumor_subclusters(infercnv_obj: InfercnvObject, p_val=0.1, k_nn=20, leiden_method="PCA", leiden_function="CPM",
                                    leiden_resolution="auto", leiden_method_per_chr="simple",
                                    leiden_function_per_chr="modularity", leiden_resolution_per_chr=1, hclust_method="ward.D2",
                                    cluster_by_groups=True, partition_method="leiden", per_chr_hmm_subclusters=False,
                                    per_chr_hmm_subclusters_references=False, z_score_filter=0.8, restrict_to_DE_genes=False,
                                    seed=0, leiden_fn=None, leiden_graph_fn=None):
    """define_signif_tumor_subclusters (R/inferCNV_tumor_subclusters.R:2-177) with leiden_method(_per_chr) = "PCA" (the
    reference's default, K18) or "simple", or partition_method = "none", on the GPU: per route one K8 call, one Leiden call
    (K11) and one K9 call over every group and partition; the PCA route's stages run as batches before them (`pca_stages`).  Returns (copy of the object with tumor_subclusters = {"hc": {group: ...}, "subclusters": {group: {name:
    0-based cells}}}, subclusters_per_chr or None).

    hc[group]: None (< 3 cells), one HClust (k_nn >= n, or "none"), or the list of the partitions' HClust of >= 2 cells in
    subcluster order (the Leiden branch; ape's binding of them into one tree, :602-640, is not mirrored).  Partitions are
    named "<group>_s<label>", by decreasing size then label (:604) -- ascending label on the per-chromosome route (:687).
    The streams are keyed by seed and FNV-1a-64 of the group name (of chr + "\\0" + group per chromosome); R's are
    igraph's.  leiden_fn(nn_idx, sizes, objective, gammas, tokens) -> 1-based memberships replaces the device Leiden
    (tests hold the driver to the restatement with it); leiden_graph_fn(row_off, col, weight, loop, sizes, objective, gammas,
    tokens) is its sibling for the weighted graphs of the PCA route (CUDA tensors of `device.snn_jaccard`; CPM's gammas
    already in units of the weights)."""
    leiden_method_per_chr = leiden_method_per_chr if per_chr_hmm_subclusters else "simple"
    _check_leiden_args(leiden_method, leiden_function, partition_method, restrict_to_DE_genes)
    _check_leiden_args(leiden_method_per_chr, leiden_function_per_chr, partition_method, False)
    leiden_fn = _device_leiden(seed) if leiden_fn is None else leiden_fn
    leiden_graph_fn = _device_leiden_graph(seed) if leiden_graph_fn is None else leiden_graph_fn
    kept = zscore_kept_genes(infercnv_obj, z_score_filter)
    if kept.size == 0:
        raise ValueError("the z-score filter keeps no gene (R: expr.data[-integer(0), ] has no row)")
    kept32 = kept.astype(np.int32)
    groups = random_trees_groups(infercnv_obj, cluster_by_groups)
    cell_names = np.asarray(infercnv_obj.cells())
    x = _to_device(infercnv_obj)

    hc, subclusters, trees = {}, {}, []          # trees: (group, cells) of the K9 batch, in order
    if partition_method == "none":               # .single_tumor_subclustering (:181-268): one tree, one subcluster
        for g, c in groups.items():
            if c.size > 2:
                trees.append((g, c))
            else:
                hc[g], subclusters[g] = None, {f"{g}_s1": c}
    else:                                        # .single_tumor_leiden_subclustering (:569-642)
        problems, keys = [], []
        for g, c in groups.items():
            if c.size < 3:
                hc[g], subclusters[g] = None, {f"{g}_s1": c}
            elif k_nn >= c.size:
                subclusters[g] = {g: c}
                trees.append((g, c))
            else:
                problems.append((c.astype(np.int32), fnv1a64(g)))
                keys.append(g)
        parts = _leiden_problems(x, [kept32] * len(problems), problems, k_nn, leiden_method, leiden_function,
                                 leiden_resolution, leiden_fn, leiden_graph_fn)
        for g, (c, _), part in zip(keys, problems, parts):
            labels, sizes = np.unique(part, return_counts=True)
            subclusters[g] = {}
            hc[g] = []
            for i in labels[np.lexsort((labels, -sizes))]:   # sort(table(partition), decreasing = TRUE): ties by label
                sub = c[part == i].astype(np.int64)
                subclusters[g][f"{g}_s{i}"] = sub
                if sub.size >= 2:
                    trees.append((g, sub))
    if trees:
        res = device.hclust_cells(x, [(kept32, c.astype(np.int32)) for _, c in trees], hclust_method)
        for (g, c), (merge, height, order) in zip(trees, res):
            tree = HClust(merge.cpu().numpy(), height.cpu().numpy(), order.cpu().numpy(), cell_names[c], hclust_method)
            if partition_method == "none":
                hc[g] = tree
                subclusters[g] = {f"{g}_s1": c[tree.order - 1]}    # cutree(hc, k = 1), cells in hc$order
            elif isinstance(hc.get(g), list):
                hc[g].append(tree)
            else:
                hc[g] = tree
    out = infercnv_obj.copy()
    out.tumor_subclusters = {"hc": {g: hc[g] for g in groups}, "subclusters": {g: subclusters[g] for g in groups}}

    per_chr = None
    if per_chr_hmm_subclusters and partition_method == "leiden":
        if per_chr_hmm_subclusters_references:
            chr_groups = groups
        else:
            obs = {k: np.asarray(v, dtype=np.int64) for k, v in infercnv_obj.observation_grouped_cell_indices.items()}
            chr_groups = obs if cluster_by_groups else {
                "all_observations": np.concatenate(list(obs.values())) if obs else np.zeros(0, dtype=np.int64)}
        per_chr = _leiden_per_chr(infercnv_obj, x, kept, chr_groups, k_nn, leiden_method_per_chr, leiden_function_per_chr,
                                  leiden_resolution_per_chr, leiden_fn, leiden_graph_fn)
        if not per_chr_hmm_subclusters_references:
            refs = {k: np.asarray(v, dtype=np.int64) for k, v in infercnv_obj.reference_grouped_cell_indices.items()}
            for c in per_chr:
                per_chr[c].update(refs)
    if infercnv_obj.hspike is not None:
        # "-mirroring for hspike" (:151-160): cluster_by_groups = TRUE, partition_method = "none", the rest at R's defaults
        out.hspike = define_signif_tumor_subclusters(infercnv_obj.hspike, cluster_by_groups=True, partition_method="none")[0]
    return out, per_chr


def _leiden_per_chr(infercnv_obj, x, kept, groups, k_nn, leiden_method, objective, leiden_resolution, leiden_fn, leiden_graph_fn=None):
    """.whole_dataset_leiden_subclustering_per_chr (R/inferCNV_tumor_subclusters.R:646-697) on the filtered genes."""
    chr_all = np.asarray(infercnv_obj.gene_order.chr).astype(str)
    chrs = chr_all[kept]
    _, first = np.unique(chr_all, return_index=True)
    levels = chr_all[np.sort(first)]
    present = set(chrs.tolist())
    C = infercnv_obj.expr_data.shape[1]
    out = {c: {} for c in levels}
    problems, genes, keys = [], [], []
    for c in levels:
        genes_c = kept[chrs == c].astype(np.int32)
        for g, cells in groups.items():
            if c not in present:
                out[c][g] = np.arange(C, dtype=np.int64)                     # every cell (:654-656)
            elif cells.size < 3 or k_nn >= cells.size:
                out[c][g] = cells                                            # kept as is (:661-668)
            else:
                out[c][g] = None                                             # placeholder: keeps R's order of the names
                problems.append((cells.astype(np.int32), fnv1a64(f"{c}\0{g}")))
                genes.append(genes_c)
                keys.append((c, g))
    parts = _leiden_problems(x, genes, problems, k_nn, leiden_method, objective, leiden_resolution, leiden_fn, leiden_graph_fn)
    for (c, g), (cells, _), part in zip(keys, problems, parts):
        entries = {}
        for i in np.unique(part):                                            # unique(partition[grouping(partition)])
            entries[f"{g}_s{i}"] = cells[part == i].astype(np.int64)
        d = out[c]
        out[c] = {}
        for name, v in d.items():
            if name == g and v is None:
                out[c].update(entries)
            else:
                out[c][name] = v
    return out


# ------------------------------------------------------------------ trees of sampled groups (sample_object)
def _merge_pair(a, b):
    """One row of R's merge matrix from two node references: a singleton (negative) before a cluster (positive); two
    singletons by leaf number, two clusters by row number."""
    return sorted((int(a), int(b)), key=lambda v: (v > 0, abs(v)))


def prune_hclust(tree: HClust, keep):
    """The induced subtree of `tree` on the kept leaves: what sample_object needs from
    as.hclust(drop.tip(as.phylo(hc), to_prune)) (R/infercnv_sampling.R:294).  There is no ape here: the result follows the
    contract below, which is believed, not verified, to be what ape's round trip returns.

    keep: a boolean mask over the leaves in label order, or the 0-based positions of the kept leaves (any order, no repeats).
    A merge of the result exists where both sides of an original merge hold kept leaves, at that merge's height; the new rows
    keep the original row order (heights stay non-decreasing) and R's conventions (singletons negative and before clusters,
    two of a kind ascending).  labels: the kept labels in original label order; order: the original order filtered and
    renumbered.  Fewer than two kept leaves: None (R's condition at :292).  Every leaf kept: an equal tree."""
    merge = np.asarray(tree.merge)
    n = merge.shape[0] + 1
    keep = np.asarray(keep)
    if keep.dtype == bool:
        if keep.shape != (n,):
            raise ValueError("a mask has one entry per leaf")
        mask = keep
    else:
        idx = keep.astype(np.int64).ravel()
        if idx.size and (idx.min() < 0 or idx.max() >= n or np.unique(idx).size != idx.size):
            raise ValueError("keep: distinct 0-based leaf positions")
        mask = np.zeros(n, dtype=bool)
        mask[idx] = True
    m = int(mask.sum())
    if m < 2:
        return None
    new_leaf = np.cumsum(mask)                       # 1-based number of a kept leaf among the kept
    rep = [None] * (n - 1)                           # per original row: the reference of its kept part in the new tree
    ref = lambda v: (-int(new_leaf[-v - 1]) if mask[-v - 1] else None) if v < 0 else rep[v - 1]
    rows, heights = [], []
    for r in range(n - 1):
        a, b = ref(int(merge[r, 0])), ref(int(merge[r, 1]))
        if a is not None and b is not None:
            rows.append(_merge_pair(a, b))
            heights.append(tree.height[r])
            rep[r] = len(rows)
        else:
            rep[r] = a if a is not None else b
    order = np.asarray(tree.order, dtype=np.int64)
    order = new_leaf[order - 1][mask[order - 1]]
    return HClust(np.asarray(rows, dtype=np.int32).reshape(m - 1, 2), np.asarray(heights, dtype=np.float64),
                  order.astype(np.asarray(tree.order).dtype), np.asarray(tree.labels)[mask], tree.method, tree.dist_method)


def expand_hclust(tree: HClust, copies, labels=None) -> HClust:
    """`tree` with leaf k replaced by copies[k] >= 1 leaves at distance 0 from each other: what sample_object needs from the
    Newick gsub of R/infercnv_sampling.R:334-369 and as.hclust(read.tree(...)).  There is no ape here: the result follows the
    contract below, which is believed, not verified, to be what ape's round trip returns.

    A leaf with m >= 2 copies becomes a caterpillar of m - 1 merges at height 0.  All of those rows come first, leaf by leaf
    in label order, then copy by copy; the original merges follow with their references remapped.  order: the original order
    with each leaf expanded in place.  labels: `<label>_<j>`, j = 1 .. m, also `_1` for a single copy (:362-367), built from
    `labels` (default: the tree's)."""
    merge = np.asarray(tree.merge)
    n = merge.shape[0] + 1
    copies = np.asarray(copies, dtype=np.int64).ravel()
    if copies.shape != (n,) or (copies < 1).any():
        raise ValueError("copies: one count >= 1 per leaf")
    base = np.asarray(tree.labels if labels is None else labels)
    if base.shape[0] != n:
        raise ValueError("labels: one per leaf")
    first = np.concatenate([[0], np.cumsum(copies)[:-1]]) + 1     # 1-based number of a leaf's first copy
    rows, leaf_ref = [], []
    for k in range(n):
        f, m = int(first[k]), int(copies[k])
        if m == 1:
            leaf_ref.append(-f)
            continue
        rows.append([-f, -(f + 1)])
        for j in range(2, m):
            rows.append([-(f + j), len(rows)])
        leaf_ref.append(len(rows))
    zero = len(rows)
    for r in range(n - 1):
        a, b = (leaf_ref[-int(v) - 1] if v < 0 else int(v) + zero for v in merge[r])
        rows.append(_merge_pair(a, b))
    height = np.concatenate([np.zeros(zero), np.asarray(tree.height, dtype=np.float64)])
    order = np.concatenate([np.arange(first[k - 1], first[k - 1] + copies[k - 1]) for k in np.asarray(tree.order, dtype=np.int64)])
    new_labels = np.array([f"{base[k]}_{j}" for k in range(n) for j in range(1, int(copies[k]) + 1)])
    return HClust(np.asarray(rows, dtype=np.int32).reshape(-1, 2), height, order.astype(np.asarray(tree.order).dtype), new_labels,
                  tree.method, tree.dist_method)


def plot_subclusters(infercnv_obj: InfercnvObject, out_dir, output_filename="subcluster_as_annotations"):
    """plot_subclusters (R/inferCNV_tumor_subclusters.R:336-361): the subclustering shown as annotation groups.  The
    subclusters of every reference group become the reference groups; those of every observation group, then of
    "all_observations", the observation groups (a repeated name replaces the earlier entry in place, as R's `[[<-` does);
    tumor_subclusters is dropped; the object is drawn by plot_cnv(cluster_by_groups = TRUE, write_expr_matrix = FALSE) into
    out_dir and returned.  An object without subclusters raises ValueError (R would draw a page without cells)."""
    from .heatmap import plot_cnv
    ts = infercnv_obj.tumor_subclusters
    if not ts or not ts.get("subclusters"):
        raise ValueError("plot_subclusters: the object has no tumor_subclusters$subclusters")
    subs = ts["subclusters"]
    out = infercnv_obj.copy()
    out.reference_grouped_cell_indices = {}
    for grp in infercnv_obj.reference_grouped_cell_indices:
        for grp2, cells in (subs.get(grp) or {}).items():
            out.reference_grouped_cell_indices[grp2] = np.asarray(cells)
    out.observation_grouped_cell_indices = {}
    for grp in list(infercnv_obj.observation_grouped_cell_indices) + ["all_observations"]:
        for grp2, cells in (subs.get(grp) or {}).items():
            out.observation_grouped_cell_indices[grp2] = np.asarray(cells)
    out.tumor_subclusters = None
    plot_cnv(out, cluster_by_groups=True, output_filename=output_filename, out_dir=out_dir, write_expr_matrix=False)
    return out
