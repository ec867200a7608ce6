"""Python mirror of add_to_seurat / .get_features / .get_top_n_regions (R/seurat_interaction.R:23-214, 244-445, 463-553): the
per-cell CNV feature table map_metadata_from_infercnv.txt with top_losses.txt and top_duplis.txt.

The reference filters the two report tables of step 17 / 19 once per subcluster, or once per cell with HMM_report_by =
"cell".  Here everything follows from the state matrix on the device: four integers per (column,
chromosome) from icnv_cnv_features, the non-neutral runs from icnv_cnv_runs, and in group mode the groups' consensus columns
from icnv_state_consensus first, because the reports hold a group's consensus state and not the cells' own states.

Chromosome columns follow InfercnvObject.chr_layout(), the order of first appearance: GeneOrder carries no factor levels, and
after .order_reduce the two orders coincide.  A level that has lost all its genes cannot be represented (R prints all-zero
columns for it).  When chr_layout() returns a permutation the genes are gathered first: the kernels see contiguous
chromosomes only.  There is no Seurat object here: add_to_seurat returns the table it writes.  Ties between regions of equal
gene count are taken in byte order of the region name (include/icnv.h), where R's table() order depends on the locale.
"""
from __future__ import annotations

import os
from decimal import Decimal

import numpy as np

from .cnv_regions import _cell_groups, _fmt, _range_reduce
from .infercnv_object import DeviceMatrix, InfercnvObject

CENTER_STATE = {"i6": 3, "i3": 2}
N_STATES = {"i6": 6, "i3": 3}
SCALING_FACTOR = 2
FEATURES_I3 = ("has_cnv", "has_loss", "has_dupli", "proportion_cnv", "proportion_loss", "proportion_dupli")
FEATURES_I6 = FEATURES_I3 + ("proportion_scaled_cnv", "proportion_scaled_loss", "proportion_scaled_dupli")


def _fmt_r(v):
    """as.character of a double, which is what cbind with the subcluster names makes of the feature matrix: 15 significant
    digits, fixed notation unless the scientific one is shorter ("2e-04", but "0.001").  The width rule is R's as read from
    its documentation (print.default / format: fixed unless wider than scientific); R is not available here to pin it."""
    v = float(v)
    if v.is_integer():
        return str(int(v))
    sign, digits, exp = Decimal(repr(float(f"{abs(v):.15g}"))).normalize().as_tuple()
    nsig, e10 = len(digits), len(digits) + exp - 1
    fixed = (e10 + 1 + (nsig - e10 if nsig > e10 + 1 else 0)) if e10 >= 0 else nsig - e10 + 1
    sci = nsig + (1 if nsig > 1 else 0) + (4 if abs(e10) < 100 else 5)
    if fixed <= sci:
        return _fmt(v)
    d = "".join(map(str, digits))
    return ("-" if v < 0 else "") + d[0] + ("." + d[1:] if nsig > 1 else "") + f"e{'-' if e10 < 0 else '+'}{abs(e10):02d}"


def features_from_counts(counts, chr_sizes, HMM_type="i6"):
    """counts: int (n_chr, n_cols, 4) of n_loss, n_gain, d_loss, d_gain; chr_sizes: genes per chromosome -> {feature name:
    (n_chr, n_cols) array}, bool for has_*, float64 for the proportions: one division each (.get_features, :284-353)."""
    c = np.asarray(counts).astype(np.int64)
    n = np.asarray(chr_sizes, dtype=np.float64)[:, None]
    n_loss, n_gain, d_loss, d_gain = (c[:, :, k] for k in range(4))
    out = {"has_cnv": (n_loss + n_gain) > 0, "has_loss": n_loss > 0, "has_dupli": n_gain > 0,
           "proportion_cnv": (n_loss + n_gain) / n, "proportion_loss": n_loss / n, "proportion_dupli": n_gain / n}
    if HMM_type == "i6":
        out["proportion_scaled_cnv"] = (d_loss + d_gain) / (n * SCALING_FACTOR)
        out["proportion_scaled_loss"] = d_loss / (n * SCALING_FACTOR)
        out["proportion_scaled_dupli"] = d_gain / (n * SCALING_FACTOR)
    return out


def get_top_n_regions(runs, gene_start, gene_end, center_state, loss, top_n=10, bp_tolerance=2000000):
    """.get_top_n_regions (:463-553) on run records.  runs: dict of arrays over the non-neutral runs in report order -- col
    (cell group), chr, gene_first, gene_last (positions in gene_start / gene_end, inclusive), state -- and the list `name`.
    Seeds are the runs of one sign (loss: state < center_state), largest gene count first, ties in byte order of the name.
    Each unused seed grows by the fixed point of :500-523 over the unused runs of EITHER sign on its chromosome: a run joins
    when one of its genes starts within bp_tolerance of the joined runs' starts and one of its genes ends within
    bp_tolerance of their ends.  Returns [(record indices of the merged runs in report order, cell groups in report order)]."""
    col, chr_i, first, last, state = (np.asarray(runs[k], dtype=np.int64) for k in ("col", "chr", "gene_first", "gene_last", "state"))
    names = list(runs["name"])
    gene_start, gene_end = np.asarray(gene_start), np.asarray(gene_end)
    r_start, r_end = _range_reduce(np.minimum, gene_start, first, last), _range_reduce(np.maximum, gene_end, first, last)
    sign = np.nonzero(state < center_state if loss else state > center_state)[0]
    size = last - first + 1
    seeds = sorted(sign.tolist(), key=lambda r: (-int(size[r]), names[r].encode()))
    used = np.zeros(col.size, dtype=bool)
    out = []
    for seed in seeds:
        if used[seed]:
            continue
        cand = np.nonzero((chr_i == chr_i[seed]) & ~used)[0]
        s_lo = s_hi = r_start[seed]
        e_lo = e_hi = r_end[seed]
        joined = None
        for _ in range(4 * col.size + 8):
            ps = np.concatenate([[0], np.cumsum((gene_start >= s_lo - bp_tolerance) & (gene_start <= s_hi + bp_tolerance))])
            pe = np.concatenate([[0], np.cumsum((gene_end >= e_lo - bp_tolerance) & (gene_end <= e_hi + bp_tolerance))])
            close = cand[(ps[last[cand] + 1] > ps[first[cand]]) & (pe[last[cand] + 1] > pe[first[cand]])]
            if joined is not None and np.array_equal(close, joined):
                break
            joined = close
            s_lo, s_hi, e_lo, e_hi = r_start[close].min(), r_start[close].max(), r_end[close].min(), r_end[close].max()
        else:
            raise RuntimeError("the merge of the top CNV regions did not reach a fixed point")
        used[joined] = True
        out.append((joined, np.array(list(dict.fromkeys(col[joined].tolist())), dtype=np.int64)))
        if len(out) == top_n:
            break
    return out


def _groups_and_map(infercnv_obj, by_cells):
    """Report-order cell groups and, in group mode, the cell -> group map (-1: in no group); overlapping groups are refused."""
    C = infercnv_obj.expr_data.shape[1]
    if by_cells:
        groups = _cell_groups(infercnv_obj, "cell")
        return groups, None
    if infercnv_obj.tumor_subclusters is None:
        raise ValueError("add_to_seurat works on tumor subclusters (or per cell): the object has none")
    groups = _cell_groups(infercnv_obj, "subcluster")
    cell_to_group = np.full(C, -1, dtype=np.int64)
    for q, (name, idx) in enumerate(groups):
        if (cell_to_group[idx] >= 0).any() or np.unique(idx).size != idx.size:
            raise ValueError(f"subcluster {name!r} shares a cell with another subcluster")
        cell_to_group[idx] = q
    return groups, cell_to_group


def device_pass(infercnv_obj: InfercnvObject, hmm_obj, HMM_type="i6", by_cells=False):
    """The device part of get_features: the consensus columns in group mode, the four integers per (cell, chromosome) and the
    non-neutral run records in report order.  Returns (groups, chr_names, chr_start, gene starts, gene stops in the gathered
    gene order, (n_chr, C, 4) counts per CELL, (6, n) run records)."""
    import torch
    from . import device
    if HMM_type not in CENTER_STATE:
        raise ValueError("HMM_type must be i6 or i3")
    s0, K = CENTER_STATE[HMM_type], N_STATES[HMM_type]
    groups, cell_to_group = _groups_and_map(infercnv_obj, by_cells)
    perm, chr_start = infercnv_obj.chr_layout()
    go = infercnv_obj.gene_order
    chrs = np.asarray(go.chr)
    G = chrs.size
    start = np.asarray(go.start) if go.start is not None else np.arange(G)
    stop = np.asarray(go.stop) if go.stop is not None else np.arange(G)
    if isinstance(hmm_obj, torch.Tensor):
        states = hmm_obj
        if tuple(states.shape) != infercnv_obj.expr_data.shape[::-1]:
            raise ValueError("the state matrix and the final object differ in shape")
        if perm is not None:
            states = states[:, torch.as_tensor(perm, device=states.device)].contiguous()
    elif isinstance(hmm_obj.expr_data, DeviceMatrix):       # a resident state object (DESIGN K32): its bytes as they lie
        from .cnv_regions import _states_dev
        if hmm_obj.expr_data.shape != infercnv_obj.expr_data.shape:
            raise ValueError("the state object and the final object differ in shape")
        states = _states_dev(hmm_obj.expr_data, perm)
    else:
        st = np.asarray(hmm_obj.expr_data)
        if st.shape != infercnv_obj.expr_data.shape:
            raise ValueError("the state object and the final object differ in shape")
        if st.dtype != np.uint8:
            st = np.where((st >= 0) & (st <= 255) & (st == np.floor(st)), st, 255).astype(np.uint8)
        if perm is not None:
            st = st[perm]
        states = torch.from_numpy(np.ascontiguousarray(st.T)).cuda()
    if perm is not None:
        chrs, start, stop = chrs[perm], start[perm], stop[perm]
    chr_names = chrs[chr_start[:-1]]
    if by_cells:
        counts, run_counts = device.cnv_features(states, chr_start, K, s0, want_run_counts=True)
        rec, _ = device.cnv_runs(states, chr_start, neutral=s0, K=K, col_idx=np.concatenate([g for _, g in groups]),
                                 run_counts=run_counts)
        cell_counts = counts.cpu().numpy()
    else:
        cons = device.state_consensus(states, [g for _, g in groups])
        counts, run_counts = device.cnv_features(cons, chr_start, K, s0, want_run_counts=True)
        rec, _ = device.cnv_runs(cons, chr_start, neutral=s0, K=K, run_counts=run_counts)
        ext = torch.cat([counts, torch.zeros_like(counts[:, :1])], dim=1)          # the last column serves the cells in no group
        gather = torch.as_tensor(np.where(cell_to_group < 0, len(groups), cell_to_group), device=ext.device)
        cell_counts = ext[:, gather].cpu().numpy()
    return groups, chr_names, chr_start, start, stop, cell_counts, rec.cpu().numpy().astype(np.int64)


def get_features(infercnv_obj: InfercnvObject, hmm_obj, HMM_type="i6", by_cells=False, top_n=10, bp_tolerance=2000000):
    """.get_features (:244-445) from the state matrix.  infercnv_obj: the final object (gene order, cell names,
    tumor_subclusters); hmm_obj: the final state object (expr_data = the genes x cells states 1 .. K of step 17, or of step
    19 after filterHighPNormals), or those states as a (cells, genes) uint8 CUDA tensor in the object's gene order.  Returns
    a dict: chr_names, the (n_chr, C) arrays of FEATURES_I6 / FEATURES_I3, top_loss / top_dupli (lists of (C,) bool vectors),
    top_loss_groups / top_dupli_groups (per top region the owning cell groups, as (name, cell indices)), and
    top_loss_region_names / top_dupli_region_names (per top region the merged regions' names).  Cells in no subcluster keep
    0 / False; subclusters that share a cell are refused with ValueError, as are states outside 1 .. K."""
    groups, chr_names, chr_start, start, stop, cell_counts, rec = device_pass(infercnv_obj, hmm_obj, HMM_type, by_cells)
    s0 = CENTER_STATE[HMM_type]
    C = cell_counts.shape[1]
    out = {"chr_names": chr_names}
    out.update(features_from_counts(cell_counts, np.diff(chr_start), HMM_type))
    runs = {"col": rec[0], "chr": rec[1], "gene_first": rec[2], "gene_last": rec[3], "state": rec[4],
            "name": [f"{chr_names[c]}-region_{o}" for c, o in zip(rec[1], rec[5])]}
    for sign, loss in (("loss", True), ("dupli", False)):
        tops = get_top_n_regions(runs, start, stop, s0, loss, top_n, bp_tolerance)
        vecs = []
        for _, owners in tops:
            v = np.zeros(C, dtype=bool)
            for q in owners:
                v[groups[q][1]] = True
            vecs.append(v)
        out["top_" + sign] = vecs
        out["top_" + sign + "_groups"] = [[groups[q] for q in owners] for _, owners in tops]
        out["top_" + sign + "_region_names"] = [[runs["name"][r] for r in joined] for joined, _ in tops]
    return out


def subcluster_of_cells(infercnv_obj: InfercnvObject):
    """The `subcluster` column (:111-123): per cell the name of its subcluster, None where it has none.  Annotations are
    visited in the order reference groups, observation groups, "all_observations"; a later assignment wins."""
    cells = infercnv_obj.cells()
    out = np.full(cells.size, None, dtype=object)
    subs = (infercnv_obj.tumor_subclusters or {}).get("subclusters", {})
    for annot in list(infercnv_obj.reference_grouped_cell_indices) + list(infercnv_obj.observation_grouped_cell_indices) + ["all_observations"]:
        for name, idx in subs.get(annot, {}).items():
            out[np.asarray(idx, dtype=np.int64)] = name
    return out


def format_table(cells, subcluster, features, HMM_type):
    """The lines of map_metadata_from_infercnv.txt (:167-211, write.table(quote = FALSE, sep = "\\t")): the header has one
    field fewer than the rows; logicals print as 1 / 0, doubles with 15 significant digits, a missing subcluster as NA."""
    names = FEATURES_I6 if HMM_type == "i6" else FEATURES_I3
    columns, cols = ["subcluster"], []
    for k, lv in enumerate(features["chr_names"]):
        for f in names:
            columns.append(f"{f}_{lv}")
            cols.append(features[f][k])
    for sign in ("loss", "dupli"):
        for i, v in enumerate(features["top_" + sign]):
            columns.append(f"top_{sign}_{i + 1}")
            cols.append(v)
    text = []
    for col in cols:                                       # few distinct values per column: each is formatted once
        vals, inv = np.unique(np.asarray(col, dtype=np.float64), return_inverse=True)
        text.append(np.array([_fmt_r(v) for v in vals], dtype=object)[inv])
    lines = ["\t".join(columns)]
    for c, cell in enumerate(cells):
        row = [str(cell), "NA" if subcluster[c] is None else str(subcluster[c])]
        row += [t[c] for t in text]
        lines.append("\t".join(row))
    return columns, lines


def top_lines(features, sign, by_cells):
    """The lines of top_losses.txt / top_duplis.txt (:374-442): "<feature>;<cell group>;<cell>" per member cell."""
    lines = []
    for i, owners in enumerate(features["top_" + sign + "_groups"]):
        for name, members in owners:
            if by_cells:
                lines.append(f"top_{sign}_{i + 1};{name};{name}")
            else:
                lines += [f"top_{sign}_{i + 1};{name};{c}" for c in members] if len(members) else [f"top_{sign}_{i + 1};{name};"]
    return lines if lines else [""]


def add_to_seurat(infercnv_obj: InfercnvObject, hmm_obj: InfercnvObject, infercnv_output_path, top_n=10, bp_tolerance=2000000,
                  HMM_type=None, by_cells=None):
    """add_to_seurat (:23-214) without a Seurat object: writes map_metadata_from_infercnv.txt, top_losses.txt and
    top_duplis.txt under infercnv_output_path and returns {"columns", "lines", "features"}.  hmm_obj: as in
    get_features.  HMM_type / by_cells default to
    the object's options (HMM_type, HMM_report_by == "cell").  Raises if there is no HMM result (the reference warns, then
    fails on the missing tables)."""
    if hmm_obj is None:
        raise ValueError("add_to_seurat transcribes the HMM results: it cannot be used without having run the HMM")
    if HMM_type is None:
        HMM_type = infercnv_obj.options.get("HMM_type", "i6")
    if by_cells is None:
        by_cells = infercnv_obj.options.get("HMM_report_by") == "cell"
    feats = get_features(infercnv_obj, hmm_obj, HMM_type, by_cells, top_n, bp_tolerance)
    cells = infercnv_obj.cells()
    for sign in ("loss", "dupli"):                         # owners carry cell names in the files
        feats["top_" + sign + "_groups"] = [[(name, cells[np.asarray(idx, dtype=np.int64)]) for name, idx in owners]
                                            for owners in feats["top_" + sign + "_groups"]]
    columns, lines = format_table(cells, subcluster_of_cells(infercnv_obj), feats, HMM_type)
    os.makedirs(infercnv_output_path, exist_ok=True)
    for fname, body in (("map_metadata_from_infercnv.txt", lines), ("top_losses.txt", top_lines(feats, "loss", by_cells)),
                        ("top_duplis.txt", top_lines(feats, "dupli", by_cells))):
        with open(os.path.join(infercnv_output_path, fname), "w") as fh:
            fh.write("\n".join(body) + "\n")
    return {"columns": columns, "lines": lines, "features": feats}
