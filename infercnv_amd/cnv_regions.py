"""CNV region / consensus reporting (second "next" row): mirror of get_predicted_CNV_regions,
.define_cnv_gene_regions, .get_cnv_gene_region_bounds and generate_cnv_region_reports (R/inferCNV_HMM.R:706-869, 1005-1087).
The per-gene consensus over a group's cells (.get_state_consensus, :977-987) and the run-length segmentation run on the GPU
(icnv_state_consensus, icnv_cnv_runs).

generate_cnv_region_reports writes its two large files, <prefix>.pred_cnv_regions.dat and .pred_cnv_genes.dat, on the GPU
(DESIGN K24): the state matrix goes to the device once, the run records stay there, and the text of the files is formatted
from them by icnv_cnv_report_format_dev and streamed to disk in chunks of whole records (text_stream.stream_chunks).  The
two small files, .cell_groupings and .genes_used.dat, are joined on the host and written at once.  The function returns a
lazy sequence: a cell group's dict is built from the run records when somebody asks for it.  The earlier host writer is kept
as _generate_cnv_region_reports_host: it is the byte-level yardstick of the device writer, and it still runs when the gene
positions are not integers that int64 holds (the device prints integers only).
"""
from __future__ import annotations

import ctypes as ct
import locale
import logging
import operator
import os
import time
from collections.abc import Sequence

import numpy as np

from . import _lib
from ._lib import check, i32, pack_groups
from .infercnv_object import DeviceMatrix, InfercnvObject

log = logging.getLogger("infercnv_amd")
REPORT_CHUNK = 256 << 20           # bytes of one chunk of the report bodies; ICNV_CNV_REPORT_CHUNK (developer switch) overrides it
LAST_REPORT_STATS = {}             # seconds and counts of the last generate_cnv_region_reports (scripts/bench_cnv_reports.py)


def _states_u8(obj):
    st = np.asarray(obj.expr_data)
    return np.asfortranarray(np.where(st < 0, 255, st).astype(np.uint8))


def _states_dev(states, perm=None, by_cell=False):
    """The (C, G) uint8 CUDA tensor of a resident state matrix (DESIGN K32) as the kernels want it: 255 for what is no state,
    the genes gathered by `perm` into per-chromosome blocks, and for by = "cell" every byte outside 1 .. 6 as the invalid
    state.  Nothing crosses; the permutation and the masks are element-wise device operations on bytes."""
    import torch
    t = states.tensor
    if states.kind != "states":
        t = torch.where(t < 0, 255.0, t).to(torch.uint8)
    if perm is not None:
        t = t.index_select(1, torch.from_numpy(np.asarray(perm, dtype=np.int64)).to(t.device))
    if by_cell:
        t = torch.where((t >= 1) & (t <= 6), t, torch.full_like(t, 255))
    return t.contiguous()


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
    if isinstance(infercnv_obj.expr_data, DeviceMatrix):
        from . import device
        cons = device.state_consensus(_states_dev(infercnv_obj.expr_data), groups).cpu().numpy().T    # G x n_groups bytes
        out = cons.astype(np.float64)
        out[cons == 255] = -1.0
        return out
    cons = _consensus_u8(_states_u8(infercnv_obj), groups)
    out = cons.astype(np.float64)
    out[cons == 255] = -1.0
    return out


def overwrite_with_consensus(infercnv_obj: InfercnvObject, groups) -> InfercnvObject:
    """expr.data[genes, group_cells] <- consensus state, the effect of R/inferCNV_HMM.R:473-483."""
    L = _lib.load()
    if isinstance(infercnv_obj.expr_data, DeviceMatrix):
        import torch
        from . import device
        t = _states_dev(infercnv_obj.expr_data)
        _, out = device.state_consensus(t, groups, overwrite=True)
        chrs = np.asarray(infercnv_obj.gene_order.chr)
        for c in np.unique(chrs):                            # (see below: a chromosome of one gene keeps its states)
            rows = np.nonzero(chrs == c)[0]
            if rows.size < 2:
                rt = torch.from_numpy(rows.astype(np.int64)).to(t.device)
                out[:, rt] = t[:, rt]
        new = infercnv_obj.copy()
        new.expr_data = DeviceMatrix(out, "states")
        return new
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
    if isinstance(infercnv_obj.expr_data, DeviceMatrix):   # resident states: the same two kernels through their _dev entries
        from . import device
        t = _states_dev(infercnv_obj.expr_data, perm, by_cell)
        if perm is not None:
            chrs, start, stop = chrs[perm], start[perm], stop[perm]
        chr_names = chrs[chr_start[:-1]]
        rec, n_runs_dev = np.zeros((6, 0), dtype=np.int32), 0
        if t.shape[0] and groups:
            if by_cell:
                r, n_runs_dev = device.cnv_runs(t, chr_start, neutral=neutral, K=K, col_idx=np.concatenate([g for _, g in groups]))
            else:
                r, n_runs_dev = device.cnv_runs(device.state_consensus(t, [g for _, g in groups]), chr_start, neutral=neutral, K=K)
            rec = r.cpu().numpy()
        col, chr_i, first, last, state, ordinal = (rec[k].astype(np.int64) for k in range(6))
        state = np.where(state == 255, -1, state)
        names = [f"{chr_names[c]}-region_{o}" for c, o in zip(chr_i, ordinal)]
        return {"groups": groups, "chr_names": chr_names, "chr_start": chr_start, "perm": perm, "n_runs": n_runs_dev,
                "col": col, "chr": chr_i, "gene_first": first, "gene_last": last, "state": state, "ordinal": ordinal, "name": names,
                "start": _range_reduce(np.minimum, start, first, last), "end": _range_reduce(np.maximum, stop, first, last)}
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


def _generate_cnv_region_reports_host(infercnv_obj: InfercnvObject, output_filename_prefix, out_dir, ignore_neutral_state=None,
                                      by="consensus"):
    """R/inferCNV_HMM.R:790-869 line by line on the host: writes <prefix>.cell_groupings, .pred_cnv_regions.dat,
    .pred_cnv_genes.dat and .genes_used.dat (tab separated, header row, no quotes, no row names except for genes_used).
    The yardstick of generate_cnv_region_reports, and its writer for gene positions that are not int64 integers."""
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


# ------------------------------------------------------------------ the reports on the device (DESIGN K24)
REGIONS_HEADER = "cell_group_name\tcnv_name\tstate\tchr\tstart\tend\n"
GENES_HEADER = "cell_group_name\tgene_region_name\tstate\tgene\tchr\tstart\tend\n"


def _int64_positions(a):
    """`a` as an int64 array when every element is an integer that int64 holds -- the numbers the device writer prints exactly
    as _fmt does -- else None (the host writer runs)."""
    a = np.asarray(a)
    if a.dtype.kind == "i" or (a.dtype.kind == "u" and (a.size == 0 or int(a.max()) <= np.iinfo(np.int64).max)):
        return a.astype(np.int64)
    if a.dtype.kind == "f" and bool(np.all(np.isfinite(a))) and bool(np.all(a == np.floor(a))) and bool(np.all(np.abs(a) < 2.0 ** 63)):
        return a.astype(np.int64)
    return None


def _neutral_byte(ignore_neutral_state):
    """The `neutral` byte of icnv_cnv_runs that leaves out what `state != ignore_neutral_state` leaves out of the host writer's
    files: 0 keeps every run, 255 is the invalid state (reported as -1).  None: a value the byte cannot express (0)."""
    if ignore_neutral_state is None:
        return 0
    v = float(ignore_neutral_state)
    if v == -1.0:
        return 255
    if v == 0.0:
        return None
    return int(v) if v.is_integer() and 1.0 <= v <= 254.0 else 0      # no state equals any other value: nothing is left out


def _report_tables(group_names, chr_names, gene_names, enc):
    """The three string tables of icnv_cnv_report_begin_dev as (uint8 bytes, int64 offsets) pairs."""
    from .device import pack_labels
    return tuple(pack_labels([str(n).encode(enc) for n in names]) for names in (group_names, chr_names, gene_names))


def _int_len(v):
    """Bytes of the decimal text of every element of an int64 array (`-` included)."""
    v = np.asarray(v, dtype=np.int64)
    mag = np.where(v < 0, -(v + 1), v).astype(np.uint64) + (v < 0).astype(np.uint64)
    return np.searchsorted(10 ** np.arange(1, 19, dtype=np.uint64), mag, side="right") + 1 + (v < 0)


def report_lengths(kind, rec, tables, start, end):
    """The closed form of DESIGN K24 in NumPy, as the kernels compute it: (bytes of every record, F of every record, P).
    rec: the six record arrays (col, chr, gene_first, gene_last, state with 255 for the invalid state, ordinal); tables:
    _report_tables(); start, end: int64 in the records' gene order.  kind "genes": a record of n genes takes
    n F + P[last + 1] - P[first] bytes, its line i starts at i F + P[first + i] - P[first]; "regions": F - 1 + digits(min
    start) + digits(max end)."""
    col, chr_i, first, last, state, ordinal = (np.asarray(r, dtype=np.int64) for r in rec)
    (_, g_off), (_, c_off), (_, n_off) = tables
    start, end = np.asarray(start, dtype=np.int64), np.asarray(end, dtype=np.int64)
    P = np.concatenate([[0], np.cumsum(np.diff(n_off) + _int_len(start) + _int_len(end))]).astype(np.int64)
    F = np.diff(g_off)[col] + 2 * np.diff(c_off)[chr_i] + 8 + _int_len(ordinal) + _int_len(np.where(state == 255, -1, state)) + 7
    if kind == "genes":
        return (last - first + 1) * F + P[last + 1] - P[first], F, P
    lo, hi = _range_reduce(np.minimum, start, first, last), _range_reduce(np.maximum, end, first, last)
    return F - 1 + _int_len(lo) + _int_len(hi), F, P


class _RegionList(Sequence):
    """What generate_cnv_region_reports returns: element i equals get_predicted_CNV_regions(...)[i] and is built from the run
    records (every run, the neutral ones included) when it is asked for."""

    def __init__(self, groups, cells, rec, chr_names, perm, start, stop):
        self._groups, self._cells, self._chr_names, self._perm, self._start, self._stop = groups, cells, chr_names, perm, start, stop
        self._col, self._chr, self._first, self._last, state, self._ordinal = (np.asarray(r).astype(np.int64) for r in rec)
        self._state = np.where(state == 255, -1, state)
        self._bounds = np.searchsorted(self._col, np.arange(len(groups) + 1))

    def __len__(self):
        return len(self._groups)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(len(self)))]
        i = operator.index(i)
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError("cell group index out of range")
        name, idx = self._groups[i]
        regions = []
        for r in range(self._bounds[i], self._bounds[i + 1]):
            rows = np.arange(self._first[r], self._last[r] + 1)
            if self._perm is not None:
                rows = self._perm[rows]
            chr_name = self._chr_names[self._chr[r]]
            regions.append((f"{chr_name}-region_{self._ordinal[r]}", {"state": float(self._state[r]), "gene": rows, "chr": chr_name,
                                                                     "start": self._start[rows], "end": self._stop[rows]}))
        ranges = [(rn, r["state"], r["chr"], r["start"].min(), r["end"].max()) for rn, r in regions]   # :1071-1087
        return {"cell_group_name": name, "cells": self._cells[idx], "gene_regions": regions, "cnv_ranges": ranges}


def _stream_report(path, kind, header, rec, tables, g_start, g_stop, chunk):
    """One report file: `header` (bytes), then the text of the records `rec` (int32 (6, n) CUDA tensor) from
    device.CnvReportPlan, streamed in chunks of whole records.  Returns (stream_chunks' statistics or None, lines)."""
    from . import device
    from .text_stream import stream_chunks
    with open(path, "wb") as fh, device.CnvReportPlan(kind, rec, *tables, g_start, g_stop) as plan:
        fh.write(header)
        state = {"next": 0}

        def fill(buf):
            if state["next"] >= plan.n_records:
                return None
            done, nbytes, _ = plan.format_into(buf, state["next"])
            state["next"] += done
            return nbytes

        streamed = None
        if plan.n_records:
            streamed = stream_chunks(fh, max(plan.max_record_bytes, min(chunk, plan.total_bytes)), rec.device, fill)
        return streamed, plan.total_lines


def generate_cnv_region_reports(infercnv_obj: InfercnvObject, output_filename_prefix, out_dir, ignore_neutral_state=None,
                                by="consensus"):
    """R/inferCNV_HMM.R:790-869: writes <prefix>.cell_groupings, .pred_cnv_regions.dat, .pred_cnv_genes.dat and
    .genes_used.dat (tab separated, header row, no quotes, no row names except for genes_used), byte for byte the files of
    _generate_cnv_region_reports_host.  The states go to the device once; group modes take the groups' consensus columns
    (device.state_consensus), by = "cell" the cells' own columns in report order with every byte outside 1 .. 6 as the invalid
    state; device.cnv_runs gives the run records and device.CnvReportPlan the text of the two .dat bodies, streamed in chunks
    of whole records (DESIGN K24).  Returns a read-only sequence with one entry per cell group, equal to
    get_predicted_CNV_regions(infercnv_obj, by) element by element; an entry is built when it is indexed."""
    go = infercnv_obj.gene_order
    n = np.asarray(go.chr).size
    start = np.asarray(go.start) if go.start is not None else np.arange(n)
    stop = np.asarray(go.stop) if go.stop is not None else np.arange(n)
    start64, stop64, neutral = _int64_positions(start), _int64_positions(stop), _neutral_byte(ignore_neutral_state)
    if start64 is None or stop64 is None or neutral is None:
        log.info("generate_cnv_region_reports: gene positions that are not int64 integers, or ignore_neutral_state = 0: "
                 "the host writer runs")
        return _generate_cnv_region_reports_host(infercnv_obj, output_filename_prefix, out_dir, ignore_neutral_state, by)
    import torch
    from . import device
    t0 = time.perf_counter()
    enc = locale.getpreferredencoding(False)
    groups = _cell_groups(infercnv_obj, by)
    by_cell = by == "cell" and infercnv_obj.tumor_subclusters is not None
    perm, chr_start = infercnv_obj.chr_layout()
    chrs, genes, cells = np.asarray(go.chr), infercnv_obj.genes(), infercnv_obj.cells()
    resident = isinstance(infercnv_obj.expr_data, DeviceMatrix)
    st = None if resident else _states_u8(infercnv_obj)
    g_chrs, g_genes, g_start, g_stop = chrs, genes, start64, stop64
    if perm is not None:                                   # the kernels see contiguous chromosomes only
        g_chrs, g_genes, g_start, g_stop = chrs[perm], np.asarray(genes)[perm], start64[perm], stop64[perm]
        if not resident:
            st = np.asfortranarray(st[perm])
    chr_names = g_chrs[chr_start[:-1]]
    if by_cell and not resident:
        # what the consensus over one cell gave before: a byte outside 1 .. 6 is the invalid state (reported as -1)
        st = np.asfortranarray(np.where((st >= 1) & (st <= 6), st, 255).astype(np.uint8))
    stats = {"device_writer": True, "by": by}
    G, C = infercnv_obj.expr_data.shape if resident else st.shape
    rec = rec_all = torch.zeros((6, 0), dtype=torch.int32, device="cuda")
    if C and groups:
        # (C, G) rows = the columns of the (G, C) column-major matrix; a resident state matrix (DESIGN K32) is there already
        dev_states = _states_dev(infercnv_obj.expr_data, perm, by_cell) if resident else torch.from_numpy(st.T).cuda()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if by_cell:
            mat, col_idx = dev_states, np.concatenate([g for _, g in groups]).astype(np.int32)
        else:
            mat, col_idx = device.state_consensus(dev_states, [g for _, g in groups]), None
        rec, _ = device.cnv_runs(mat, chr_start, neutral=neutral, K=0, col_idx=col_idx)
        rec_all = rec if neutral == 0 else device.cnv_runs(mat, chr_start, neutral=0, K=0, col_idx=col_idx)[0]
        del dev_states, mat
    else:
        t1 = time.perf_counter()
    rec_host = rec_all.cpu().numpy()
    stats["convert_upload_s"], stats["runs_s"] = t1 - t0, time.perf_counter() - t1

    os.makedirs(out_dir, exist_ok=True)
    path = lambda suffix: os.path.join(out_dir, output_filename_prefix + suffix)
    with open(path(".cell_groupings"), "w") as fh:
        fh.write("cell_group_name\tcell\n" + "".join(f"{name}\t{c}\n" for name, idx in groups for c in cells[idx]))
    tables = _report_tables([name for name, _ in groups] or [""], chr_names, g_genes, enc)
    chunk = int(os.environ.get("ICNV_CNV_REPORT_CHUNK", REPORT_CHUNK))
    for kind, suffix, header in (("regions", ".pred_cnv_regions.dat", REGIONS_HEADER), ("genes", ".pred_cnv_genes.dat", GENES_HEADER)):
        t2 = time.perf_counter()
        streamed, stats[kind + "_lines"] = _stream_report(path(suffix), kind, header.encode(enc), rec, tables, g_start, g_stop, chunk)
        if streamed is not None:
            stats[kind] = streamed
        stats[kind + "_s"] = time.perf_counter() - t2
    t3 = time.perf_counter()
    with open(path(".genes_used.dat"), "w") as fh:        # write.table(gene_order, quote=FALSE, sep="\t"): row names kept
        fh.write("chr\tstart\tstop\n" + "".join(f"{g}\t{c}\t{a}\t{b}\n" for g, c, a, b in zip(genes, chrs, start64.tolist(), stop64.tolist())))
    stats["genes_used_s"], stats["total_s"] = time.perf_counter() - t3, time.perf_counter() - t0
    LAST_REPORT_STATS.clear()
    LAST_REPORT_STATS.update(stats)
    return _RegionList(groups, cells, rec_host, chr_names, perm, start, stop)


def _adjust_from_records(mcmc_obj, output_filename_prefix, out_dir):
    """adjust_genes_regions_report from the run records of mcmc_obj.table (DESIGN K25).  The parser keeps a line of the
    step-17 files when its region NAME is one the filter kept and gives it the state of the last kept region of that name:
    this is the same rule on (chromosome, ordinal) keys over the table the filter started from, whether or not a name is
    unique.  False -- nothing written -- when the gene positions are not int64 integers (the device prints integers only)."""
    import torch
    kept = mcmc_obj.table
    full = kept.source if kept.source is not None else kept
    obj = mcmc_obj.infercnv_obj
    go = obj.gene_order
    n = np.asarray(go.chr).size
    start64 = _int64_positions(np.asarray(go.start) if go.start is not None else np.arange(n))
    stop64 = _int64_positions(np.asarray(go.stop) if go.stop is not None else np.arange(n))
    if start64 is None or stop64 is None:
        log.info("adjust_genes_regions_report: gene positions that are not int64 integers: the step-17 files are parsed")
        return False
    enc = locale.getpreferredencoding(False)
    genes = np.asarray(obj.genes())
    if full.perm is not None:
        genes, start64, stop64 = genes[full.perm], start64[full.perm], stop64[full.perm]
    span = int(max(full.ordinal.max(initial=0), kept.ordinal.max(initial=0))) + 1
    key_kept, key_full = kept.chr * span + kept.ordinal, full.chr * span + full.ordinal
    names, last = np.unique(key_kept[::-1], return_index=True)          # the last kept region of every name
    state_of = kept.state[::-1][last]
    pos = np.minimum(np.searchsorted(names, key_full), max(names.size - 1, 0))
    hit = (names[pos] == key_full) if names.size else np.zeros(key_full.size, dtype=bool)
    state = state_of[pos[hit]]
    rec = np.stack([full.col[hit], full.chr[hit], full.gene_first[hit], full.gene_first[hit] + full.gene_count[hit] - 1,
                    np.where(state < 0, 255, state), full.ordinal[hit]]).astype(np.int32)
    rec = torch.from_numpy(np.ascontiguousarray(rec)).cuda()
    tables = _report_tables([name for name, _ in full.groups] or [""], full.chr_names, genes, enc)
    chunk = int(os.environ.get("ICNV_CNV_REPORT_CHUNK", REPORT_CHUNK))
    os.makedirs(out_dir, exist_ok=True)
    for kind, suffix, header in (("genes", ".pred_cnv_genes.dat", GENES_HEADER), ("regions", ".pred_cnv_regions.dat", REGIONS_HEADER)):
        _stream_report(os.path.join(out_dir, output_filename_prefix + suffix), kind, header.encode(enc), rec, tables, start64, stop64, chunk)
    return True


def adjust_genes_regions_report(mcmc_obj, input_filename_prefix, output_filename_prefix, out_dir):
    """adjust_genes_regions_report (R/inferCNV_HMM.R:891-963): the step-17 reports <input prefix>.pred_cnv_genes.dat and
    .pred_cnv_regions.dat restricted to the regions the Bayesian filter kept (mcmc_obj.cell_gene), their state column
    replaced by the region's state after the filter, written under the output prefix.  Every other field passes through
    as text.  When the object carries a RegionTable (bayes_net route="table", DESIGN K25) the two files are written from its
    records instead of being parsed back from text -- the same bytes, provided the step-17 reports were written without the
    normal state's regions (ignore_neutral_state = the normal state, as run() writes them); gene positions that are not
    int64 integers take the parser."""
    if getattr(mcmc_obj, "table", None) is not None:
        for suffix in (".pred_cnv_genes.dat", ".pred_cnv_regions.dat"):      # R stops where an input file is missing
            src = os.path.join(out_dir, input_filename_prefix + suffix)
            if not os.path.exists(src):
                raise FileNotFoundError(f"Cannot find and adjust the following file. {src}")
        if _adjust_from_records(mcmc_obj, output_filename_prefix, out_dir):
            return
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
