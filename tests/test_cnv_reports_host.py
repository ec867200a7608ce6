"""Host side of the CNV region reports (DESIGN K24), no GPU: the closed-form record and line lengths against the restatement's
lines, the packing of the string tables, the decision for the host writer, and the prototypes."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

import cnv_reports_restate as rr

from infercnv_amd import _lib, cnv_regions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def records_of(obj, by, ignore):
    """The six record arrays and the tables, from the restatement's regions (state 255 for the invalid state)."""
    groups = rr.cell_groups(obj, by)
    chrs = [str(c) for c in obj.gene_order.chr]
    chr_names = list(dict.fromkeys(chrs))
    perm = [i for c in chr_names for i, cc in enumerate(chrs) if cc == c]               # the gathered gene order
    where = {g: k for k, g in enumerate(perm)}
    by_cell = by == "cell" and obj.tumor_subclusters is not None
    rec, counter = [], 0
    for pos, (_, idx) in enumerate(groups):
        regs, counter = rr.regions_of(rr.group_states(np.asarray(obj.expr_data), idx, by_cell), chrs, counter)
        rec += [(pos, chr_names.index(c), where[rows[0]], where[rows[-1]], 255 if state == -1 else state, ordinal)
                for c, ordinal, state, rows in regs if state != ignore]
    tables = cnv_regions._report_tables([n for n, _ in groups], chr_names, np.asarray(obj.genes())[perm], "utf-8")
    start, stop = np.asarray(obj.gene_order.start, dtype=np.int64)[perm], np.asarray(obj.gene_order.stop, dtype=np.int64)[perm]
    return np.array(rec, dtype=np.int64).reshape(-1, 6).T, tables, start, stop


@pytest.mark.parametrize("make,by,ignore", [(lambda: rr.edge_object(odd_bytes=True), "cell", None), (rr.edge_object, "subcluster", 3),
                                            (rr.edge_object, "consensus", 2), (lambda: rr.width_object(C=16, G=700, seed=2), "cell", 3),
                                            (lambda: rr.width_object(C=16, G=600, seed=5, scramble=True), "cell", None)])
def test_closed_form_lengths(make, by, ignore):
    obj = make()
    rec, tables, start, stop = records_of(obj, by, ignore)
    region_lines, gene_lines = rr.report_lines(obj, by, ignore)
    assert rec.shape[1] == len(region_lines) > 0
    got, F, P = cnv_regions.report_lengths("genes", rec, tables, start, stop)
    assert got.tolist() == [sum(len(l.encode()) for l in ls) for ls in gene_lines]
    for r, ls in enumerate(gene_lines):                                                  # where every line of a record starts
        first = rec[2, r]
        at = [i * F[r] + P[first + i] - P[first] for i in range(len(ls))]
        assert at == np.concatenate([[0], np.cumsum([len(l.encode()) for l in ls])])[:-1].tolist()
    got, _, _ = cnv_regions.report_lengths("regions", rec, tables, start, stop)
    assert got.tolist() == [len(l.encode()) for l in region_lines]


def test_int_len():
    vals = [0, 9, 10, 99, 100, 99999999, 2 ** 31, 10 ** 15, 10 ** 18 - 1, 10 ** 18, 2 ** 63 - 1, -1, -5, -10, -(2 ** 63)]
    assert cnv_regions._int_len(np.array(vals, dtype=np.int64)).tolist() == [len(str(v)) for v in vals]


def test_string_tables():
    names = ["a", "", "bcd", "zelle_äö€", "x" * 300]
    (b, off), (cb, coff), (gb, goff) = cnv_regions._report_tables(names, ["chr1"], np.array(["g1", "g22"], dtype=object), "utf-8")
    enc = [n.encode("utf-8") for n in names]
    assert b.dtype == np.uint8 and off.dtype == np.int64 and off.tolist() == np.concatenate([[0], np.cumsum([len(e) for e in enc])]).tolist()
    assert [b[off[i]:off[i + 1]].tobytes() for i in range(len(names))] == enc
    assert coff.tolist() == [0, 4] and goff.tolist() == [0, 2, 5] and gb[:5].tobytes() == b"g1g22"
    assert len(enc[3]) == 13                                                             # multi-byte UTF-8 counts in bytes


def test_host_writer_decision():
    ok = cnv_regions._int64_positions
    assert ok(np.array([0, 5, -5])).dtype == np.int64
    assert ok(np.array([0.0, 1e15, -5.0])).tolist() == [0, 10 ** 15, -5]
    assert ok(np.array([1, 2], dtype=np.uint64)).tolist() == [1, 2]
    assert ok(np.array([1.5, 2.0])) is None and ok(np.array([1.0, np.nan])) is None and ok(np.array([np.inf])) is None
    assert ok(np.array([2.0 ** 63])) is None and ok(np.array([2 ** 63], dtype=np.uint64)) is None
    assert ok(np.array(["1", "2"])) is None and ok(np.array([True])) is None
    nb = cnv_regions._neutral_byte
    assert (nb(None), nb(3), nb(2.0), nb(np.int64(1)), nb(-1), nb(254)) == (0, 3, 2, 1, 255, 254)
    assert nb(0) is None                                                                 # a byte cannot say "leave out state 0"
    assert (nb(2.5), nb(255), nb(300), nb(-3)) == (0, 0, 0, 0)                           # no state equals these: nothing is left out


def test_fallback_runs_the_host_writer(monkeypatch, tmp_path, caplog):
    """Non-integral positions: one log line and the host writer, with the caller's arguments."""
    obj = rr.edge_object()
    obj.gene_order.start = np.asarray(obj.gene_order.start, dtype=np.float64) + 0.5
    calls = []
    monkeypatch.setattr(cnv_regions, "_generate_cnv_region_reports_host", lambda *a: calls.append(a) or ["host"])
    with caplog.at_level("INFO", logger="infercnv_amd"):
        assert cnv_regions.generate_cnv_region_reports(obj, "p", str(tmp_path), ignore_neutral_state=3, by="cell") == ["host"]
    assert len(calls) == 1 and calls[0][0] is obj and calls[0][1:] == ("p", str(tmp_path), 3, "cell")
    assert sum("host writer" in r.getMessage() for r in caplog.records) == 1


def test_prototypes():
    header = open(os.path.join(ROOT, "include", "icnv.h")).read()
    assert "ICNV_REPORT_GENES 0" in header and "ICNV_REPORT_REGIONS 1" in header
    assert (_lib.REPORT_GENES, _lib.REPORT_REGIONS) == (0, 1)
    ctype = {"int64_t": ct.c_int64, "int32_t": ct.c_int32}
    for name in ("icnv_cnv_report_begin_dev", "icnv_cnv_report_begin", "icnv_cnv_report_format_dev", "icnv_cnv_report_format",
                 "icnv_cnv_report_end", "icnv_cnv_report_stats", "icnv_cnv_report_stats_reset"):
        m = re.search(r"\n(int|void) " + name + r"\(([^;]*)\);", header)
        assert m, name
        res, args = _lib.PROTOTYPES[name]
        assert (res is None) == (m.group(1) == "void")
        params = [] if m.group(2).strip() == "void" else [" ".join(p.split()) for p in m.group(2).split(",")]
        assert len(params) == len(args), name
        for p, a in zip(params, args):
            if "*" in p:                                                                 # a pointer of some kind
                assert a is ct.c_void_p or issubclass(a, ct._Pointer), (name, p)
                if p.startswith("int64_t *") or p.startswith("const int64_t *"):
                    assert a is ct.POINTER(ct.c_int64), (name, p)
            else:
                assert a is ctype[p.split()[0]], (name, p)
