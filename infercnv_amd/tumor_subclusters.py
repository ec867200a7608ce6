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
with the recursion itself in the pure-Python `random_trees_partition`."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import device
from .infercnv_object import InfercnvObject


def parallelDist(infercnv_obj: InfercnvObject, cells, as_dist: bool = True):
    """parallelDist(t(expr.data[, cells]), method="euclidean").

    as_dist=True returns the R `dist` object's vector (lower triangle in column order == SciPy's condensed
    form); False the full symmetric (n, n) matrix."""
    import torch
    cells = np.asarray(cells, dtype=np.int32)
    if cells.ndim != 1 or cells.size < 1:
        raise ValueError("cells must be a non-empty index vector")
    x = infercnv_obj.expr_data
    xd = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64).T)).cuda()
    d = device.cell_distances(xd, cells).cpu().numpy()
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
    row numbers (ascending), or None when the filter does not apply."""
    if not (z_score_filter > 0 and infercnv_obj.has_reference_cells()):
        return None
    x = np.asarray(infercnv_obj.expr_data, dtype=np.float64)
    ref = x[:, infercnv_obj.get_reference_grouped_cell_indices()]
    m, s = _r_mean(ref), _r_sd(ref)
    z = np.abs((ref - m) / s)
    row_mean = np.array([_r_mean(z[g]) for g in range(z.shape[0])])
    return np.flatnonzero(row_mean >= 0.8).astype(np.int64)


def zscore_kept_genes(infercnv_obj: InfercnvObject, z_score_filter: float = 0.8):
    """The rows of expr.data the subclustering goes on with (R/inferCNV_tumor_subclusters.R:45-71).  When the filter applies
    and finds no outlier, R's `expr.data[-outliers, ]` with `outliers = integer(0)` keeps NO row: mirrored as such."""
    G = np.asarray(infercnv_obj.expr_data).shape[0]
    out = zscore_outlier_genes(infercnv_obj, z_score_filter)
    if out is None:
        return np.arange(G, dtype=np.int64)
    if out.size == 0:
        return np.zeros(0, dtype=np.int64)
    return np.setdiff1d(np.arange(G, dtype=np.int64), out)


def _to_device(infercnv_obj):
    import torch
    x = np.asarray(infercnv_obj.expr_data, dtype=np.float64)
    return torch.from_numpy(np.ascontiguousarray(x.T)).cuda()


def nn2(infercnv_obj: InfercnvObject, cells, k: int, genes=None):
    """RANN::nn2(t(expr.data[genes, cells]), k = k) with query = data (R/inferCNV_tumor_subclusters.R:726), exact on the GPU.
    Returns (nn_idx, nn_dists) as numpy arrays of shape (len(cells), k); nn_idx holds 0-based positions in `cells`
    (R's nn.idx is 1-based).  Exactly equal distances are ordered by position (RANN's order among them is its tree walk)."""
    cells = np.asarray(cells, dtype=np.int32)
    G = np.asarray(infercnv_obj.expr_data).shape[0]
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
    G = np.asarray(infercnv_obj.expr_data).shape[0]
    genes = np.arange(G, dtype=np.int32) if genes is None else np.asarray(genes, dtype=np.int32)
    if cells.ndim != 1 or genes.ndim != 1:
        raise ValueError("cells and genes must be index vectors")
    (merge, height, order), = device.hclust_cells(_to_device(infercnv_obj), [(genes, cells)], method)
    labels = np.asarray(infercnv_obj.cells())[cells]
    return HClust(merge.cpu().numpy(), height.cpu().numpy(), order.cpu().numpy(), labels, method)


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
            x.append(torch.from_numpy(np.ascontiguousarray(np.asarray(sub.expr_data, dtype=np.float64).T)).cuda())
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
