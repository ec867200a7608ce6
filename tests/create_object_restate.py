"""Restatement of CreateInfercnvObject and .order_reduce, written from R/inferCNV.R:133-428 alone, in plain Python: str.split,
float() per field, lists and dicts.  It shares no code with infercnv_amd; the tests compare the library with it slot by slot.

read.table's part: the first line is the header, every other non-blank line a row whose first field is the row name; a field
is float(text), with R's NA (the double with bits 0x7FF00000000007A2) for `NA` and the empty field.  Values travel as int64 bit
patterns so that NA and NaN compare.

Where the reference leaves a choice to the machine it runs on, the library's documented choice is restated: names sort by
their UTF-8 bytes; a reference group without cells is an error; max_cells_per_group keeps the first entries of
numpy.random.Generator(Philox(key = [seed, FNV-1a-64(group)])).permutation(n); column sums are exact (math.fsum).
"""
import gzip
import math
import struct

import numpy as np

NA_BITS = 0x7FF00000000007A2


def bits(text):
    if text in ("NA", ""):
        return NA_BITS
    return struct.unpack("<q", struct.pack("<d", float(text)))[0] & 0xFFFFFFFFFFFFFFFF


def signed(b):
    return b - (1 << 64) if b >= 1 << 63 else b


def strip_quotes(s):
    return s[1:-1] if len(s) >= 2 and s[0] == '"' and s[-1] == '"' else s


def read_table(path, sep="\t"):
    """(row names, column names, int64 bits [rows][cols]) of a file read as read.table(header = TRUE, row.names = 1) reads it."""
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rb") as fh:
        text = fh.read().decode("utf-8")
    lines = [ln[:-1] if ln.endswith("\r") else ln for ln in text.split("\n")]
    header = [strip_quotes(t) for t in lines[0].split(sep)]
    rows = [ln.split(sep) for ln in lines[1:] if ln != ""]
    width = len(rows[0])
    assert all(len(r) == width for r in rows)
    cols = header if len(header) == width - 1 else header[1:]
    assert len(cols) == width - 1
    names = [strip_quotes(r[0]) for r in rows]
    vals = np.array([[signed(bits(t)) for t in r[1:]] for r in rows], dtype=np.int64).reshape(len(rows), width - 1)
    return names, cols, vals


def as_double(vals):
    return np.asarray(vals, dtype=np.int64).view(np.float64)


def fnv(name):
    h = 0xCBF29CE484222325
    for b in name.encode("utf-8"):
        h = ((h ^ b) * 0x100000001B3) % (1 << 64)
    return h


def small_table(src, sep):
    if isinstance(src, str):
        with (gzip.open(src, "rt") if src.endswith(".gz") else open(src)) as fh:
            return [ln.rstrip("\n").rstrip("\r").split(sep) for ln in fh if ln.strip("\r\n") != ""]
    return [list(r) for r in src]


def create_object(genes, cells, x_bits, gene_order, annotations, ref_group_names, delim="\t", max_cells_per_group=None,
                  min_max_counts_per_cell=(100, float("inf")), chr_exclude=("chrX", "chrY", "chrM"), seed=0):
    """genes, cells, x_bits: what read_table returned (or names and the bits of a genes x cells array).  Returns a dict of the
    object's slots; raises ValueError with the reference's text where the reference stops."""
    x = as_double(x_bits)
    if len(set(genes)) != len(genes):
        raise ValueError("duplicate 'row.names' are not allowed")
    if len(set(cells)) != len(cells):
        raise ValueError("duplicate cell name")
    # :168-181
    pos = []
    for name, chrom, start, stop in small_table(gene_order, "\t"):
        if chr_exclude is None or chrom not in chr_exclude:
            pos.append((name, chrom, int(start), int(stop)))
    if len({p[0] for p in pos}) != len(pos):
        raise ValueError("duplicate 'row.names' are not allowed")
    # :183-198
    ann = [(c, k) for c, k in small_table(annotations, delim)]
    if len({a[0] for a in ann}) != len(ann):
        raise ValueError("duplicate 'row.names' are not allowed")
    if ann and ann[0][0] == "V1":
        ann = ann[1:]
    # :200-210
    missing = [c for c, _ in ann if c not in cells]
    if missing:
        raise ValueError(" ".join(["Please make sure that all the annotated cell ", "names match a sample in your data matrix. ",
                                   "Attention to: ", ",".join(missing)]))
    # .order_reduce :352-428
    pos = [p for p in pos if p[2] + p[3] != 0]
    chr_levels = []
    for p in pos:
        if p[1] not in chr_levels:
            chr_levels.append(p[1])
    pos_names = [p[0] for p in pos]
    keep_genes = [g for g in genes if g in pos_names]
    if not keep_genes:
        raise ValueError(" ".join(["None of the genes in the expression data", "matched the genes in the reference genomic",
                                   "position file. Analysis Stopped."]))
    order = [pos[pos_names.index(g)] for g in keep_genes]
    rank = sorted(range(len(order)), key=lambda i: (chr_levels.index(order[i][1]), order[i][2], order[i][3]))
    order = [order[i] for i in rank]
    x = x[[genes.index(p[0]) for p in order], :]
    # :236-258
    if min_max_counts_per_cell is None:
        min_max_counts_per_cell = (1, float("inf"))
    lo, hi = max(1, min_max_counts_per_cell[0]), min_max_counts_per_cell[1]
    cs = [math.fsum(x[:, j].tolist()) for j in range(x.shape[1])]
    keep = [j for j in range(x.shape[1]) if lo <= cs[j] <= hi]
    cols = [cells[j] for j in keep]
    x = x[:, keep]
    ann = [a for a in ann if a[0] in cols]
    # :260-265 (the reference fails here when a group is gone)
    ref_group_names = list(ref_group_names or [])
    if any(r not in {k for _, k in ann} for r in ref_group_names):
        raise ValueError("reference group without cells")
    # :269-282
    if max_cells_per_group is not None:
        out = []
        for grp in sorted({k for _, k in ann}, key=lambda s: s.encode("utf-8")):
            members = [a for a in ann if a[1] == grp]
            if len(members) > max_cells_per_group:
                perm = np.random.Generator(np.random.Philox(key=[seed, fnv(grp)])).permutation(len(members))
                members = [members[i] for i in perm[:max_cells_per_group]]
            out += members
        ann = out
    # :284-288
    annotated = {a[0]: a[1] for a in ann}
    keep = [j for j, c in enumerate(cols) if c in annotated]
    x = x[:, keep]
    cols = [cols[j] for j in keep]
    classes = [annotated[c] for c in cols]
    # :291-312
    ref = {r: [i for i, k in enumerate(classes) if k == r] for r in ref_group_names}
    others = sorted({k for k in classes if k not in ref_group_names}, key=lambda s: s.encode("utf-8"))
    obs = {o: [i for i, k in enumerate(classes) if k == o] for o in others}
    return {"expr_bits": np.ascontiguousarray(x).view(np.int64), "gene_names": [p[0] for p in order], "cell_names": cols,
            "chr": [p[1] for p in order], "start": [p[2] for p in order], "stop": [p[3] for p in order],
            "ref": ref, "obs": obs, "ref_order": list(ref), "obs_order": list(obs)}


def compare(obj, want):
    """Assert that an InfercnvObject equals create_object's dict in every slot."""
    got = np.ascontiguousarray(np.asarray(obj.expr_data, dtype=np.float64)).view(np.int64)
    assert got.shape == want["expr_bits"].shape
    assert np.array_equal(got, want["expr_bits"])
    assert obj.count_data is obj.expr_data
    assert list(obj.gene_names) == want["gene_names"] and list(obj.cell_names) == want["cell_names"]
    assert list(obj.gene_order.chr) == want["chr"]
    assert list(obj.gene_order.start) == want["start"] and list(obj.gene_order.stop) == want["stop"]
    assert list(obj.reference_grouped_cell_indices) == want["ref_order"]
    assert list(obj.observation_grouped_cell_indices) == want["obs_order"]
    for name, idx in want["ref"].items():
        assert obj.reference_grouped_cell_indices[name].tolist() == idx
    for name, idx in want["obs"].items():
        assert obj.observation_grouped_cell_indices[name].tolist() == idx
