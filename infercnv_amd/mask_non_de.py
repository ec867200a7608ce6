"""Step 21 of run(), mask_nonDE_genes (R/inferCNV_ops.R:1509-1557): mask_non_DE_genes_basic and get_DE_genes_basic
(R/inferCNV_mask_non_DE.R:28-258) with every per-gene test of every (subcluster, normal type) comparison on the GPU
(icnv_de_tests_dev, DESIGN K12) and the mask in one device pass (icnv_mask_non_de_dev).

R draws the rank-sum jitter unseeded; the library draws it from a documented stream keyed by `seed` (include/icnv.h), one
draw per (gene, cell) shared by every comparison of the call.  Indices are 0-based."""
from __future__ import annotations

import numpy as np

from . import device
from .infercnv_object import DeviceMatrix, InfercnvObject

MIN_CLUSTER_SIZE_MASK = 5   # .mask_DE_genes(min_cluster_size_mask = 5)


def _check_test(test_use):
    if test_use == "perm":
        raise NotImplementedError("test_use='perm' (coin::oneway_test) is not implemented on the GPU")
    if test_use not in device.DE_TESTS:
        raise ValueError(f"unknown test_use {test_use!r}: 'wilcoxon' or 't'")


def _comparisons(obj: InfercnvObject):
    """R's loop order: observation group, its subclusters in order, normal type.  Returns (groups, pairs, entries) with
    groups = normal types then subclusters (0-based cell vectors), pairs = (normal group, subcluster group) per comparison and
    entries = (key, subcluster cells, normal name) per comparison."""
    normals = [(name, np.asarray(v, dtype=np.int64)) for name, v in obj.reference_grouped_cell_indices.items()]
    groups = [v for _, v in normals]
    pairs, entries = [], []
    subs = (obj.tumor_subclusters or {}).get("subclusters", {}) if obj.tumor_subclusters is not None else {}
    for group in obj.observation_grouped_cell_indices:
        ind = subs.get(group)
        if not isinstance(ind, dict):   # R: an unnamed vector gives a list without names, which the loop skips
            continue
        for name, cells in ind.items():
            cells = np.asarray(cells, dtype=np.int64)
            q = len(groups)
            groups.append(cells)
            for k, (nname, _) in enumerate(normals):
                pairs.append((k, q))
                entries.append((f"{name},{nname}", cells, nname))
    return groups, pairs, entries


def _tests(x, obj, test_use, seed, jitter):
    groups, pairs, entries = _comparisons(obj)
    if not pairs:
        return None, None, None, entries
    stat, p, padj = device.de_tests(x, groups, pairs, test=test_use, jitter=jitter, seed=seed)
    return stat, p, padj, entries


def _final(entries):
    """all_DE_results keeps one entry per key (a repeated key replaces the value in place, as R's list assignment does):
    key -> comparison row."""
    rows = {}
    for i, (key, _, _) in enumerate(entries):
        rows[key] = i
    return rows


def get_DE_genes_basic(obj: InfercnvObject, p_val_thresh=0.05, test_use="wilcoxon", seed=0, jitter=True):
    """R's all_DE_results: {"subcluster,normal": {"tumor_indices", "normal", "pvals" (BH-adjusted, by gene name),
    "de_genes"}}.  de_genes: the genes with padj < p_val_thresh (R's names(pvals)[pvals < thresh] adds NA entries for NA
    p-values; they match no gene and are left out)."""
    import torch
    _check_test(test_use)
    if isinstance(obj.expr_data, DeviceMatrix):
        x = obj.expr_data.tensor
    else:
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(obj.expr_data, dtype=np.float64).T)).cuda()
    _, _, padj, entries = _tests(x, obj, test_use, seed, jitter)
    genes = np.asarray(obj.genes())
    out = {}
    if padj is None:
        return out
    pa = padj.cpu().numpy()
    for key, row in _final(entries).items():
        _, cells, nname = entries[row]
        v = pa[row]
        out[key] = {"tumor_indices": cells, "normal": nname, "pvals": dict(zip(genes.tolist(), v.tolist())),
                    "de_genes": genes[v < p_val_thresh].tolist()}
    return out


def mask_plan(C, obj: InfercnvObject, entries, rows):
    """(base, cell_cmps) of .mask_DE_genes: base N for reference cells and the cells of subclusters under 5 cells, and per
    cell the comparison rows of the larger subclusters that contain it."""
    N = len(obj.reference_grouped_cell_indices)
    base = np.zeros(C, dtype=np.int32)
    ref = obj.get_reference_grouped_cell_indices()
    base[ref] = N
    cell_cmps = [[] for _ in range(C)]
    for row in rows.values():
        cells = entries[row][1]
        if cells.size < MIN_CLUSTER_SIZE_MASK:
            base[cells] = N
    for row in rows.values():
        cells = entries[row][1]
        if cells.size >= MIN_CLUSTER_SIZE_MASK:
            for c in cells.tolist():
                cell_cmps[c].append(row)
    return base, cell_cmps


def mask_non_de_device(x, obj: InfercnvObject, p_val_thresh=0.05, test_use="wilcoxon", center_val=None,
                       require_DE_all_normals="any", seed=0, jitter=True, out=None):
    """mask_non_DE_genes_basic on a (C, G) CUDA matrix x (obj supplies the groups and subclusters): returns (masked CUDA
    matrix, mask value used)."""
    _check_test(test_use)
    if require_DE_all_normals not in device.DE_RULES:
        raise ValueError(f"Error, not recognizing require_DE_all_normals={require_DE_all_normals}")
    if not obj.has_reference_cells():
        raise ValueError("Error, cannot mask non-DE genes when there are no normal references set")
    _, _, padj, entries = _tests(x, obj, test_use, seed, jitter)
    rows = _final(entries)
    base, cell_cmps = mask_plan(x.shape[0], obj, entries, rows)
    return device.mask_non_de(x, padj, p_val_thresh, base, cell_cmps, len(obj.reference_grouped_cell_indices),
                              rule=require_DE_all_normals, mask_val=center_val, out=out)


def mask_non_DE_genes_basic(obj: InfercnvObject, p_val_thresh=0.05, test_use="wilcoxon", center_val=None,
                            require_DE_all_normals="any", seed=0, jitter=True) -> InfercnvObject:
    """mask_non_DE_genes_basic (R/inferCNV_mask_non_DE.R:28-50) -> a new object.  center_val None: mean(expr.data),
    correctly rounded."""
    import torch
    from .ops import _with_expr
    _check_test(test_use)
    if require_DE_all_normals not in device.DE_RULES:
        raise ValueError(f"Error, not recognizing require_DE_all_normals={require_DE_all_normals}")
    if isinstance(obj.expr_data, DeviceMatrix):              # resident (DESIGN K32): a new tensor, the input object keeps its own
        out, _ = mask_non_de_device(obj.expr_data.tensor, obj, p_val_thresh, test_use, center_val, require_DE_all_normals, seed, jitter)
        return _with_expr(obj, DeviceMatrix(out))
    x = torch.from_numpy(np.ascontiguousarray(np.asarray(obj.expr_data, dtype=np.float64).T)).cuda()
    out, _ = mask_non_de_device(x, obj, p_val_thresh, test_use, center_val, require_DE_all_normals, seed, jitter, out=x)
    return _with_expr(obj, out.cpu().numpy().T.copy())
