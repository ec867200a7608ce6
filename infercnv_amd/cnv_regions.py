"""CNV region / consensus reporting (second "next" row): host-side mirror of
get_predicted_CNV_regions, .define_cnv_gene_regions, .get_cnv_gene_region_bounds and
generate_cnv_region_reports (R/inferCNV_HMM.R:706-869, 1005-1087).  The per-gene consensus over a
group's cells (.get_state_consensus, :977-987) and the run-length segmentation run on the GPU (icnv_state_consensus,
icnv_cnv_runs); the four report files are written on the host, in the reference's formats.
"""
from __future__ import annotations

import ctypes as ct
import os

import numpy as np

from . import _lib
from ._lib import check, i32, pack_groups
from .infercnv_object import InfercnvObject


def _states_u8(obj):
    st = np.asarray(obj.expr_data)
    return np.asfortranarray(np.where(st < 0, 255, st).astype(np.uint8))


def _consensus_u8(st, groups):
    """(G, n_groups) uint8 consensus of the (G, C) uint8 state matrix (icnv_state_consensus)."""
    L = _lib.load()
    G, C = st.shape
    idx, off = pack_groups(groups)
    idx, ip = i32(idx)
    off, op = i32(off)
    cons = np.empty((G, len(groups)), dtype=np.uint8, order="F")
    check(L.icnv_state_consensus(st.ctypes.data_as(ct.c_void_p), G, C, ip, op, len(groups), cons.ctypes.data_as(ct.c_void_p), None))
    return cons


def state_consensus(infercnv_obj: InfercnvObject, groups):
    """(G, n_groups) consensus states (float, -1 where the consensus is the invalid state)."""
    cons = _consensus_u8(_states_u8(infercnv_obj), groups)
    out = cons.astype(np.float64)
    out[cons == 255] = -1.0
    return out


def overwrite_with_consensus(infercnv_obj: InfercnvObject, groups) -> InfercnvObject:
    """expr.data[genes, group_cells] <- consensus state, the effect of R/inferCNV_HMM.R:473-483."""
    L = _lib.load()
    st = _states_u8(infercnv_obj)
    G, C = st.shape
    idx, off = pack_groups(groups)
    idx, ip = i32(idx)
    off, op = i32(off)
    out = np.empty((G, C), dtype=np.uint8, order="F")
    check(L.icnv_state_consensus(st.ctypes.data_as(ct.c_void_p), G, C, ip, op, len(groups), None,
                                 out.ctypes.data_as(ct.c_void_p)))
    res = out.astype(np.float64)
    res[out == 255] = -1.0
    # chromosomes with fewer than two genes are skipped by .define_cnv_gene_regions (:1013): untouched
    chrs = np.asarray(infercnv_obj.gene_order.chr)
    for c in np.unique(chrs):
        rows = np.nonzero(chrs == c)[0]
        if rows.size < 2:
            res[rows] = np.asarray(infercnv_obj.expr_data)[rows]
    new = infercnv_obj.copy()
    new.expr_data = res
    return new


def _cell_groups(obj, by):
    """R/inferCNV_HMM.R:713-733 -> list of (name, 0-based index vector)."""
    if obj.tumor_subclusters is None:
        by = "consensus"
    if by == "consensus":
        d = dict(obj.reference_grouped_cell_indices)
        d.update(obj.observation_grouped_cell_indices)
        return [(k, np.asarray(v, dtype=np.int32)) for k, v in d.items()]
    if by == "subcluster":
        out = []
        for grp, subs in obj.tumor_subclusters["subclusters"].items():
            for name, v in subs.items():
                out.append((f"{grp}.{name}", np.asarray(v, dtype=np.int32)))   # unlist(recursive=FALSE) names
        return out
    if by == "cell":
        cells = obj.cells()
        order = np.concatenate([np.asarray(v, dtype=np.int32) for v in obj.reference_grouped_cell_indices.values()] +
                               [np.asarray(v, dtype=np.int32) for v in obj.observation_grouped_cell_indices.values()])
        return [(str(cells[i]), np.array([i], dtype=np.int32)) for i in order]
    raise ValueError("by must be one of consensus, subcluster, cell")


def _range_reduce(ufunc, a, first, last):
    """ufunc.reduce(a[first[i] : last[i] + 1]) for every i, without a loop."""
    if first.size == 0:
        return a[:0]
    idx = np.empty(2 * first.size, dtype=np.int64)
    idx[0::2], idx[1::2] = first, last + 1
    return ufunc.reduceat(np.concatenate([a, a[-1:]]), idx)[0::2]


def predicted_cnv_runs(infercnv_obj: InfercnvObject, by="consensus", neutral=0, K=0):
    """The run-length segmentation of get_predicted_CNV_regions (R/inferCNV_HMM.R:706-764 with .define_cnv_gene_regions,
    :1005-1057) as arrays, from the device (icnv_cnv_runs): one record per run of equal states within a chromosome whose state
    is not `neutral` (0: every run), ordered by (cell group in report order, gene).  Group modes segment the groups' consensus
    states (icnv_state_consensus); by = "cell" segments the cells' own columns in report order -- reference groups, then
    observation groups -- without a consensus.  Returns a dict: groups [(name, 0-based cell indices)], chr_names (order of
    first appearance), chr_start, perm (the gene gather of chr_layout(), or None), n_runs (runs of every state: the last
    region counter), and per record the arrays col (index into groups), chr (index into chr_names), gene_first / gene_last
    (positions in the gathered gene order, inclusive), state (-1: the invalid state), ordinal, name ("<chr>-region_<ordinal>"),
    start / end (min start / max stop over the run's genes).  K > 0 refuses states outside 1 .. K with ValueError."""
    L = _lib.load()
    groups = _cell_groups(infercnv_obj, by)
    by_cell = by == "cell" and infercnv_obj.tumor_subclusters is not None
    perm, chr_start = infercnv_obj.chr_layout()
    chrs = np.asarray(infercnv_obj.gene_order.chr)
    n = chrs.size
    start = np.asarray(infercnv_obj.gene_order.start) if infercnv_obj.gene_order.start is not None else np.arange(n)
    stop = np.asarray(infercnv_obj.gene_order.stop) if infercnv_obj.gene_order.stop is not None else np.arange(n)
    st = _states_u8(infercnv_obj)
    if perm is not None:                                   # the kernels see contiguous chromosomes only
        st, chrs, start, stop = np.asfortranarray(st[perm]), chrs[perm], start[perm], stop[perm]
    chr_names = chrs[chr_start[:-1]]                       # chr_layout() yields no empty chromosome
    if by_cell:
        # what the consensus over one cell gave before: a byte outside 1 .. 6 is the invalid state (reported as -1)
        mat = np.asfortranarray(np.where((st >= 1) & (st <= 6), st, 255).astype(np.uint8))
        col_idx, cp = i32(np.concatenate([g for _, g in groups]) if groups else np.zeros(0, dtype=np.int32))
        n_cols = col_idx.size
    else:
        mat = _consensus_u8(st, [g for _, g in groups])
        col_idx, cp, n_cols = None, None, len(groups)
    G, C = mat.shape
    cs, csp = i32(chr_start)
    n_rec, n_runs = ct.c_int64(), ct.c_int64()

    def call(cap, rec):
        rc = L.icnv_cnv_runs(mat.ctypes.data_as(ct.c_void_p), G, C, csp, cs.size - 1, cp, n_cols, int(K), int(neutral), cap,
                             rec.ctypes.data_as(ct.c_void_p) if rec is not None else None, ct.byref(n_rec), ct.byref(n_runs))
        if rc == _lib.ERR_ARG:
            raise ValueError(L.icnv_last_error().decode("utf-8", "replace"))
        check(rc)

    rec = np.zeros((6, 0), dtype=np.int32)
    if C and n_cols:
        call(0, None)
        rec = np.empty((6, max(n_rec.value, 1)), dtype=np.int32)
        call(rec.shape[1], rec)
        rec = rec[:, :n_rec.value]
    col, chr_i, first, last, state, ordinal = (rec[k].astype(np.int64) for k in range(6))
    state = np.where(state == 255, -1, state)
    names = [f"{chr_names[c]}-region_{o}" for c, o in zip(chr_i, ordinal)]
    return {"groups": groups, "chr_names": chr_names, "chr_start": chr_start, "perm": perm, "n_runs": n_runs.value,
            "col": col, "chr": chr_i, "gene_first": first, "gene_last": last, "state": state, "ordinal": ordinal, "name": names,
            "start": _range_reduce(np.minimum, start, first, last), "end": _range_reduce(np.maximum, stop, first, last)}


def get_predicted_CNV_regions(infercnv_obj: InfercnvObject, by="consensus"):
    """R/inferCNV_HMM.R:706-764.  Returns a list of dicts {cell_group_name, cells, gene_regions, cnv_ranges};
    gene_regions = ordered list of (region name, dict(state, gene idx array, chr, start, end arrays)).  Built from the run
    records of predicted_cnv_runs (every run, the neutral ones included)."""
    runs = predicted_cnv_runs(infercnv_obj, by)
    perm = runs["perm"]
    n = np.asarray(infercnv_obj.gene_order.chr).size
    start = np.asarray(infercnv_obj.gene_order.start) if infercnv_obj.gene_order.start is not None else np.arange(n)
    stop = np.asarray(infercnv_obj.gene_order.stop) if infercnv_obj.gene_order.stop is not None else np.arange(n)
    cells = infercnv_obj.cells()
    bounds = np.searchsorted(runs["col"], np.arange(len(runs["groups"]) + 1))
    out = []
    for gi, (name, idx) in enumerate(runs["groups"]):
        regions = []
        for r in range(bounds[gi], bounds[gi + 1]):
            rows = np.arange(runs["gene_first"][r], runs["gene_last"][r] + 1)
            if perm is not None:
                rows = perm[rows]
            regions.append((runs["name"][r], {"state": float(runs["state"][r]), "gene": rows, "chr": runs["chr_names"][runs["chr"][r]],
                                              "start": start[rows], "end": stop[rows]}))
        ranges = [(rn, r["state"], r["chr"], r["start"].min(), r["end"].max()) for rn, r in regions]   # :1071-1087
        out.append({"cell_group_name": name, "cells": cells[idx], "gene_regions": regions, "cnv_ranges": ranges})
    return out


def _fmt(v):
    """write.table(quote=FALSE) formatting of numbers: integers without a decimal point, up to 15 significant digits."""
    if isinstance(v, (float, np.floating)):
        return str(int(v)) if float(v).is_integer() else repr(float(np.float64(f"{v:.15g}")))
    return str(v)


def generate_cnv_region_reports(infercnv_obj: InfercnvObject, output_filename_prefix, out_dir, ignore_neutral_state=None,
                                by="consensus"):
    """R/inferCNV_HMM.R:790-869: writes <prefix>.cell_groupings, .pred_cnv_regions.dat, .pred_cnv_genes.dat and
    .genes_used.dat (tab separated, header row, no quotes, no row names except for genes_used)."""
    cnv_regions = get_predicted_CNV_regions(infercnv_obj, by)
    os.makedirs(out_dir, exist_ok=True)
    genes = infercnv_obj.genes()
    path = lambda suffix: os.path.join(out_dir, output_filename_prefix + suffix)
    with open(path(".cell_groupings"), "w") as fh:
        fh.write("cell_group_name\tcell\n")
        for x in cnv_regions:
            for c in x["cells"]:
                fh.write(f"{x['cell_group_name']}\t{c}\n")
    keep = (lambda s: True) if ignore_neutral_state is None else (lambda s: s != ignore_neutral_state)
    with open(path(".pred_cnv_regions.dat"), "w") as fh:
        fh.write("cell_group_name\tcnv_name\tstate\tchr\tstart\tend\n")
        for x in cnv_regions:
            for rn, state, c, s, e in x["cnv_ranges"]:
                if keep(state):
                    fh.write("\t".join([x["cell_group_name"], rn, _fmt(state), str(c), _fmt(s), _fmt(e)]) + "\n")
    with open(path(".pred_cnv_genes.dat"), "w") as fh:
        fh.write("cell_group_name\tgene_region_name\tstate\tgene\tchr\tstart\tend\n")
        for x in cnv_regions:
            for rn, r in x["gene_regions"]:
                if keep(r["state"]):
                    for g, s, e in zip(r["gene"], r["start"], r["end"]):
                        fh.write("\t".join([x["cell_group_name"], rn, _fmt(r["state"]), str(genes[g]), str(r["chr"]),
                                            _fmt(s), _fmt(e)]) + "\n")
    go = infercnv_obj.gene_order
    with open(path(".genes_used.dat"), "w") as fh:        # write.table(gene_order, quote=FALSE, sep="\t"): row names kept
        fh.write("chr\tstart\tstop\n")
        n = np.asarray(go.chr).size
        st = go.start if go.start is not None else np.arange(n)
        sp = go.stop if go.stop is not None else np.arange(n)
        for i in range(n):
            fh.write(f"{genes[i]}\t{np.asarray(go.chr)[i]}\t{_fmt(st[i])}\t{_fmt(sp[i])}\n")
    return cnv_regions


def adjust_genes_regions_report(mcmc_obj, input_filename_prefix, output_filename_prefix, out_dir):
    """adjust_genes_regions_report (R/inferCNV_HMM.R:891-963): the step-17 reports <input prefix>.pred_cnv_genes.dat and
    .pred_cnv_regions.dat restricted to the regions the Bayesian filter kept (mcmc_obj.cell_gene), their state column
    replaced by the region's state after the filter, written under the output prefix.  Every other field passes through
    as text."""
    new_state = {str(cg["cnv_regions"]): cg["State"] for cg in mcmc_obj.cell_gene}
    for suffix, name_col in ((".pred_cnv_genes.dat", "gene_region_name"), (".pred_cnv_regions.dat", "cnv_name")):
        src = os.path.join(out_dir, input_filename_prefix + suffix)
        if not os.path.exists(src):
            raise FileNotFoundError(f"Cannot find and adjust the following file. {src}")
        with open(src) as fh:
            lines = fh.read().splitlines()
        header = lines[0].split("\t")
        i_name, i_state = header.index(name_col), header.index("state")
        with open(os.path.join(out_dir, output_filename_prefix + suffix), "w") as fh:
            fh.write(lines[0] + "\n")
            for ln in lines[1:]:
                f = ln.split("\t")
                if f[i_name] in new_state:
                    f[i_state] = _fmt(new_state[f[i_name]])
                    fh.write("\t".join(f) + "\n")
