"""Host-side mirror of the distance step of the reference's subclustering
(R/inferCNV_tumor_subclusters.R:180-194: `hclust(parallelDist(t(tumor_expr_data)))`): the Euclidean distances
between the cells of one tumor group, computed on the GPU (icnv_cell_distances_dev, fp64 matrix cores).  The
clustering itself (hclust / Leiden) stays in R -- SURVEY.md 8f #4 scopes only the dense contraction.

The Leiden route's neighbour search (R/inferCNV_tumor_subclusters.R:646-741, RANN::nn2) is the exact kNN of
icnv_knn_dev (DESIGN K8): `nn2`, `snn_adjacency`, `knn_per_chr`, with the reference-based gene filter of :45-71.

The hierarchical clustering itself, `hclust(parallelDist(t(x)), method = hclust_method)` (:191, 582, 609 and the other
call sites of DESIGN K9), runs on the GPU too: `hclust` returns R's hclust object without the distance matrix ever leaving
the device."""
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
