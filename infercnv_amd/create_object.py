"""CreateInfercnvObject (R/inferCNV.R:133-337) and .order_reduce (:352-428): from a counts matrix, a gene-position table and
a cell-annotation table to the InfercnvObject every step function takes (DESIGN K21).

The matrix is parsed and kept on the device (device.read_table, icnv_parse_table_dev); the two small tables are read here.
The host decisions -- which genes in which order, which cells, which groups -- are plain functions of names and column sums
(read_gene_order, read_annotations, order_reduce, select_cells), so they run and are tested without a GPU; the matrix work is
colSums over the kept genes (icnv_col_sums_dev) and two gathers (icnv_gather_matrix_dev).

Deviations from the reference, all of them where the reference cannot be followed:
  * R's sort() of the observation group names, and split()'s group order, collate by locale; the names are sorted by their
    UTF-8 bytes here (the choice K14 made for ties).
  * A reference group without cells is an error.  R's `if (!all.equal(...))` (:262) fails on the character result there, so
    the reference cannot continue either.
  * Duplicate cell names are refused: check.names = FALSE would let them through to an ambiguous %in%.
  * max_cells_per_group: R's sample() is unseeded.  The cells of a group with more than the limit are the first
    max_cells_per_group entries of numpy.random.Generator(Philox(key = [seed, FNV-1a-64 of the group name])).permutation(n)
    (tumor_subclusters.fnv1a64, as K10 keys its streams).
  * options["counts_md5"] is None: R's digest() of its own serialisation is not reproducible, and only run()'s resume reads it.
  * Numbers are C's strtod, bit for bit.  R's R_strtod works in long double and can differ in the last bit on rare fields;
    agreement with read.table's bits is believed for short decimals and not verified.
"""
from __future__ import annotations

import gzip
import os

import numpy as np

from .infercnv_object import GeneOrder, InfercnvObject

CHR_EXCLUDE = ("chrX", "chrY", "chrM")
ERR_MISSING_CELLS = "Please make sure that all the annotated cell  names match a sample in your data matrix.  Attention to:  "
ERR_NO_GENES = ("None of the genes in the expression data matched the genes in the reference genomic position file. "
                "Analysis Stopped.")
ERR_DUP_ROW_NAMES = "duplicate 'row.names' are not allowed"


def _open_text(path):
    path = os.fspath(path)
    return gzip.open(path, "rt", encoding="utf-8", errors="surrogateescape") if path.endswith(".gz") else \
        open(path, "rt", encoding="utf-8", errors="surrogateescape", newline=None)


def _unquote(tok):
    return tok[1:-1] if len(tok) >= 2 and tok[0] == tok[-1] and tok[0] in "\"'" else tok


def _table_rows(table, sep, n_fields, what):
    """The rows of a small table: a path (one line per row, `sep` between the fields, blank lines skipped, quotes around a
    field dropped) or a sequence of rows."""
    if isinstance(table, (str, os.PathLike)):
        rows = []
        with _open_text(table) as fh:
            for no, line in enumerate(fh, 1):
                line = line.rstrip("\n").rstrip("\r")
                if not line:
                    continue
                toks = [_unquote(t) for t in line.split(sep)]
                if len(toks) != n_fields:
                    raise ValueError(f"{what}: line {no} has {len(toks)} fields, {n_fields} are expected")
                rows.append(toks)
        return rows
    rows = [[str(v) if isinstance(v, (str, bytes, np.str_)) else v for v in row] for row in np.asarray(table, dtype=object).tolist()]
    for row in rows:
        if len(row) != n_fields:
            raise ValueError(f"{what}: a row has {len(row)} fields, {n_fields} are expected")
    return rows


def _number(v):
    if isinstance(v, str):
        try:
            return int(v)
        except ValueError:
            return float(v)
    return v


def _first_duplicate(names):
    seen = set()
    for n in names:
        if n in seen:
            return n
        seen.add(n)
    return None


def read_gene_order(gene_order_file, chr_exclude=CHR_EXCLUDE):
    """read.table(gene_order_file, header = FALSE, row.names = 1, sep = "\\t") with the chr_exclude rows removed (:168-181):
    (names, chr, start, stop) as lists in file order.  gene_order_file: a path, or rows of (name, chr, start, stop)."""
    rows = _table_rows(gene_order_file, "\t", 4, "gene_order_file")
    names = [str(r[0]) for r in rows]
    if _first_duplicate(names) is not None:
        raise ValueError(f"gene_order_file: {ERR_DUP_ROW_NAMES} ({_first_duplicate(names)!r})")
    excl = set(chr_exclude) if chr_exclude is not None else set()
    keep = [i for i, r in enumerate(rows) if str(r[1]) not in excl]
    return ([names[i] for i in keep], [str(rows[i][1]) for i in keep], [_number(rows[i][2]) for i in keep],
            [_number(rows[i][3]) for i in keep])


def read_annotations(annotations_file, delim="\t"):
    """read.table(annotations_file, header = FALSE, row.names = 1, sep = delim, colClasses = character) and the removal of a
    first row named "V1" (:183-198): (cell names, classifications) in file order."""
    rows = _table_rows(annotations_file, delim, 2, "annotations_file")
    cells, classes = [str(r[0]) for r in rows], [str(r[1]) for r in rows]
    if _first_duplicate(cells) is not None:
        raise ValueError(f"annotations_file: {ERR_DUP_ROW_NAMES} ({_first_duplicate(cells)!r})")
    if cells and cells[0] == "V1":
        cells, classes = cells[1:], classes[1:]
    return cells, classes


def order_reduce(gene_names, positions):
    """.order_reduce (:352-428).  gene_names: the matrix's row names; positions: read_gene_order's tuple.  Returns (rows, chr,
    start, stop): the matrix rows to keep, in genomic order, and their positions; chr holds the names, whose levels are in
    order of first appearance in the position table (after the drop of start + stop == 0).  rows is None when no gene matches."""
    names, chrs, start, stop = positions
    ok = [i for i in range(len(names)) if start[i] + stop[i] != 0]
    levels = {}
    for i in ok:
        levels.setdefault(chrs[i], len(levels))
    where = {names[i]: i for i in ok}
    keep = [gi for gi, g in enumerate(gene_names) if g in where]          # intersect(): matrix row order
    if not keep:
        return None, [], [], []
    order = sorted(range(len(keep)), key=lambda k: (levels[chrs[where[gene_names[keep[k]]]]], start[where[gene_names[keep[k]]]],
                                                    stop[where[gene_names[keep[k]]]]))                      # sorted() is stable
    rows = np.array([keep[k] for k in order], dtype=np.int64)
    at = [where[gene_names[r]] for r in rows]
    return rows, [chrs[i] for i in at], [start[i] for i in at], [stop[i] for i in at]


def check_annotated_cells(cell_names, annotations):
    """Every annotated cell must be a column of the matrix (:200-210); the reference's error text otherwise."""
    known = set(cell_names)
    missing = [c for c in annotations[0] if c not in known]
    if missing:
        raise ValueError(ERR_MISSING_CELLS + ",".join(missing))


def _byte_sorted(names):
    return sorted(names, key=lambda s: s.encode("utf-8", "surrogateescape"))


def select_cells(cell_names, col_sums, annotations, ref_group_names, min_max_counts_per_cell=(100, float("inf")),
                 max_cells_per_group=None, seed=0):
    """The cell side of CreateInfercnvObject (:200-210, :236-312).  cell_names: the matrix's column names; col_sums: colSums
    over the kept genes; annotations: read_annotations' pair.  Returns (columns, classes, ref, obs): the matrix columns that
    stay, in matrix order, their classifications, and the two dicts of 0-based indices into `columns` -- the reference groups
    in the caller's order, the observation groups sorted by bytes."""
    from .tumor_subclusters import fnv1a64
    cell_names = [str(c) for c in cell_names]
    if _first_duplicate(cell_names) is not None:
        raise ValueError(f"duplicate cell name in the matrix: {_first_duplicate(cell_names)!r}")
    a_cells, a_classes = annotations
    column = {c: j for j, c in enumerate(cell_names)}
    check_annotated_cells(column, annotations)
    if min_max_counts_per_cell is None:
        min_max_counts_per_cell = (1, float("inf"))
    lo, hi = max(1, min_max_counts_per_cell[0]), min_max_counts_per_cell[1]
    cs = np.asarray(col_sums, dtype=np.float64)
    kept = (cs >= lo) & (cs <= hi)
    annot = [(c, k) for c, k in zip(a_cells, a_classes) if kept[column[c]]]            # annotation order
    present = {k for _, k in annot}
    if isinstance(ref_group_names, str):
        ref_group_names = [ref_group_names]
    ref_group_names = [str(r) for r in (ref_group_names if ref_group_names is not None else [])]
    gone = [r for r in ref_group_names if r not in present]
    if gone:
        raise ValueError("reference group(s) without cells: " + ", ".join(gone))
    if max_cells_per_group is not None:
        trimmed = []
        for grp in _byte_sorted(present):
            members = [(c, k) for c, k in annot if k == grp]
            if len(members) > max_cells_per_group:
                rng = np.random.Generator(np.random.Philox(key=[int(seed), fnv1a64(grp)]))
                members = [members[i] for i in rng.permutation(len(members))[:int(max_cells_per_group)]]
            trimmed += members
        annot = trimmed
    klass = dict(annot)
    columns = np.array([j for j, c in enumerate(cell_names) if kept[j] and c in klass], dtype=np.int64)
    classes = [klass[cell_names[j]] for j in columns]
    ref = {r: np.array([i for i, k in enumerate(classes) if k == r], dtype=np.int32) for r in ref_group_names}
    seen = list(dict.fromkeys(classes))
    obs = {o: np.array([i for i, k in enumerate(classes) if k == o], dtype=np.int32)
           for o in _byte_sorted([k for k in seen if k not in ref])}
    return columns, classes, ref, obs


def _matrix_on_device(raw_counts_matrix, delim, gene_names, cell_names, chunk_bytes):
    """(gene names, cell names, (C, G) CUDA float64 tensor, reader stats or None)."""
    import torch
    from . import device
    if isinstance(raw_counts_matrix, (str, os.PathLike)):
        genes, cells, x, stats = device.read_table(raw_counts_matrix, sep=delim, chunk_bytes=chunk_bytes)
        return genes, cells, x, stats
    if gene_names is None or cell_names is None:
        raise ValueError("a matrix given as an array comes with gene_names and cell_names")
    if hasattr(raw_counts_matrix, "toarray") and not isinstance(raw_counts_matrix, np.ndarray):
        raw_counts_matrix = raw_counts_matrix.toarray()                  # scipy sparse: densified on the host, as as.matrix does
    m = np.asarray(raw_counts_matrix, dtype=np.float64)
    if m.ndim != 2 or m.shape != (len(gene_names), len(cell_names)):
        raise ValueError("the matrix must be genes x cells, with one name per row and per column")
    return [str(g) for g in gene_names], [str(c) for c in cell_names], torch.from_numpy(np.ascontiguousarray(m.T)).cuda(), None


def make_unique(names, sep="."):
    """R's make.unique: the first occurrence of a name stays, every later one gets `sep` and the smallest number, counted up
    from 1 per name, that gives a string neither among the input nor handed out before."""
    taken, used, nxt, out = set(names), set(), {}, []
    for n in names:
        if n not in used:
            used.add(n)
            out.append(n)
            continue
        k = nxt.get(n, 1)
        while f"{n}{sep}{k}" in taken:
            k += 1
        taken.add(f"{n}{sep}{k}")
        nxt[n] = k + 1
        out.append(f"{n}{sep}{k}")
    return out


def _name_list(src, column, what):
    """Names given as a list, or as the path of a .tsv[.gz] whose `column`-th tab-separated field (1-based) holds them."""
    if not isinstance(src, (str, os.PathLike)):
        return [str(v) for v in src]
    out = []
    with _open_text(src) as fh:
        for no, line in enumerate(fh, 1):
            line = line.rstrip("\n").rstrip("\r")
            if not line:
                continue
            toks = line.split("\t")
            if len(toks) < column:
                raise ValueError(f"{what}: line {no} has {len(toks)} fields, column {column} is asked for")
            out.append(toks[column - 1])
    return out


def _first_existing(directory, names):
    for n in names:
        if os.path.exists(os.path.join(directory, n)):
            return os.path.join(directory, n)
    raise ValueError(f"{directory}: none of {', '.join(names)} is there")


def _mtx_source(raw_counts_matrix, gene_names, cell_names, gene_column):
    """(matrix path, gene names, cell names) when the matrix is a MatrixMarket file or a directory in 10x layout, else None."""
    if not isinstance(raw_counts_matrix, (str, os.PathLike)):
        return None
    path = os.fspath(raw_counts_matrix)
    if os.path.isdir(path):                                              # what Seurat::Read10X reads
        mtx = _first_existing(path, ("matrix.mtx.gz", "matrix.mtx"))
        genes = _name_list(_first_existing(path, ("features.tsv.gz", "features.tsv", "genes.tsv")), gene_column, "features")
        cells = _name_list(_first_existing(path, ("barcodes.tsv.gz", "barcodes.tsv")), 1, "barcodes")
        return mtx, make_unique(genes), cells
    if not (path.endswith(".mtx") or path.endswith(".mtx.gz")):
        return None
    if gene_names is None or cell_names is None:
        raise ValueError("a .mtx matrix comes with gene_names and cell_names (lists, or paths of .tsv files)")
    return path, _name_list(gene_names, gene_column, "gene_names"), _name_list(cell_names, 1, "cell_names")


RDS_SUFFIXES = (".rds", ".rda", ".rdata")


def _rds_source(raw_counts_matrix):
    """The path when the matrix is an R file -- .rds, or an .rda / .RData container (the suffix in any case) --, else None."""
    if not isinstance(raw_counts_matrix, (str, os.PathLike)):
        return None
    path = os.fspath(raw_counts_matrix)
    return path if path.lower().endswith(RDS_SUFFIXES) and not os.path.isdir(path) else None


def _rds_names(gene_names, cell_names, gene_column):
    return {"gene_names": None if gene_names is None else _name_list(gene_names, gene_column, "gene_names"),
            "cell_names": None if cell_names is None else _name_list(cell_names, 1, "cell_names")}


def CreateInfercnvObject(raw_counts_matrix, gene_order_file, annotations_file, ref_group_names, delim="\t", max_cells_per_group=None,
                         min_max_counts_per_cell=(100, float("inf")), chr_exclude=CHR_EXCLUDE, seed=0, gene_names=None,
                         cell_names=None, return_device=False, chunk_bytes=None, sparse=None, gene_column=2):
    """CreateInfercnvObject (R/inferCNV.R:133-337) with the reference's formals, plus `seed` (the down-sampling of
    max_cells_per_group; see the module's notes on the deviations), `gene_names` / `cell_names` (for a matrix given as a NumPy
    array, a scipy sparse matrix or a .mtx file, genes x cells), `return_device`, `sparse` and `gene_column`.

    raw_counts_matrix: a path (text, or .gz; .rds / .rda / .RData: below), an array or a sparse matrix.  gene_order_file,
    annotations_file: paths, or small tables given as rows.  The matrix file is parsed on the device; a byte outside the
    grammar of include/icnv.h raises IcnvError with its line and field.

    R files (DESIGN K34; R/inferCNV.R:151-162 reads them with readRDS).  A path that ends in .rds -- or .rda / .RData, a
    container with exactly one variable -- is decoded on the device from the serialised stream (device.read_rds_counts): a
    numeric or integer matrix and a data.frame of numeric / integer columns take the dense route; a dgCMatrix takes the sparse
    route of K22 (sparse=None or True), or is expanded on the device and continues on the dense route (sparse=False); sparse=True
    with a dense kind is the ValueError below.  A dgCMatrix is validated on the device (ValueError with the rule, the column and
    the entry), and one that holds non-integers is refused with the sparse route's message.  gene_names / cell_names supply the
    names a file lacks (compact row.names, no dimnames).  What a file may hold and what each refusal names: rds.locate_counts.

    Sparse input (DESIGN K22).  raw_counts_matrix may also be a MatrixMarket coordinate file (.mtx, .mtx.gz; gene_names and
    cell_names are then lists, or paths of .tsv[.gz] files whose `gene_column`-th, for cells first, column holds the names), or a
    directory in 10x layout (matrix.mtx[.gz], features.tsv[.gz] or genes.tsv, barcodes.tsv[.gz]; the gene names are the
    `gene_column`-th column made unique as R's make.unique does, which is what Seurat::Read10X hands the reference).
      sparse = None   every input that worked before takes the route it took (a sparse object is densified by toarray());
                      .mtx and directory input take the sparse route
      sparse = True   a scipy sparse matrix (anything with tocsc) stays sparse too
      sparse = False  .mtx input is expanded on the device (DeviceCounts.to_dense) and continues on the dense route
    The sparse route: device.read_mtx or DeviceCounts.from_scipy, the name and annotation checks, .order_reduce, the column
    sums over the kept genes (device.ingest_col_sums: integer sums, equal to the dense route's bit for bit), the cell filter,
    device.csc_select.  expr_data and count_data are then the same scipy.sparse.csc_matrix (float64 data, as a dgCMatrix
    holds; the entries of a column in the file's order); every other slot is what the dense route gives.  The counts must be
    integers in 0 .. 2^31 - 1 (ValueError pointing to sparse=False otherwise).

    Returns the InfercnvObject: expr_data and count_data (the same genes x cells array, as in R), gene_order (chr, start, stop),
    gene_names, cell_names, the two 0-based index dicts, options (chr_exclude, max_cells_per_group, min_max_counts_per_cell,
    counts_md5 = None), validated.  return_device = True returns (object, x) with x the (cells, genes) CUDA float64 tensor of
    the same values -- on the sparse route the CSC DeviceCounts --, for a caller that goes on with device.*."""
    from . import device
    positions = read_gene_order(gene_order_file, chr_exclude)
    annotations = read_annotations(annotations_file, delim)
    counts = x = None
    rds_path = _rds_source(raw_counts_matrix)
    mtx = None if rds_path is not None else _mtx_source(raw_counts_matrix, gene_names, cell_names, gene_column)
    if rds_path is not None:
        genes, cells, got, _ = device.read_rds_counts(rds_path, chunk_bytes=chunk_bytes, **_rds_names(gene_names, cell_names, gene_column))
        if isinstance(got, device.DeviceCounts):
            counts, x = (None, got.to_dense()) if sparse is False else (got, None)
        elif sparse:
            raise ValueError("sparse=True wants a .mtx file, a 10x directory or a scipy sparse matrix")
        else:
            x = got
    elif mtx is not None:
        genes, cells = mtx[1], mtx[2]
        counts, _ = device.read_mtx(mtx[0], chunk_bytes=chunk_bytes)
        if (counts.G, counts.C) != (len(genes), len(cells)):
            raise ValueError(f"the matrix is {counts.G} x {counts.C}, but there are {len(genes)} gene names and {len(cells)} cell names")
        if sparse is False:
            counts, x = None, counts.to_dense()
    elif sparse and hasattr(raw_counts_matrix, "tocsc"):
        if gene_names is None or cell_names is None:
            raise ValueError("a matrix given as an array comes with gene_names and cell_names")
        genes, cells = [str(g) for g in gene_names], [str(c) for c in cell_names]
        if tuple(raw_counts_matrix.shape) != (len(genes), len(cells)):
            raise ValueError("the matrix must be genes x cells, with one name per row and per column")
        counts = device.DeviceCounts.from_scipy(raw_counts_matrix)
    elif sparse:
        raise ValueError("sparse=True wants a .mtx file, a 10x directory or a scipy sparse matrix")
    else:
        genes, cells, x, _ = _matrix_on_device(raw_counts_matrix, delim, gene_names, cell_names, chunk_bytes)
    if _first_duplicate(genes) is not None:
        raise ValueError(f"{ERR_DUP_ROW_NAMES} ({_first_duplicate(genes)!r})")
    check_annotated_cells(cells, annotations)                      # before .order_reduce, as in R; select_cells refuses duplicates
    rows, chrs, start, stop = order_reduce(genes, positions)
    if rows is None:
        raise ValueError(ERR_NO_GENES)
    if counts is not None:
        cs = device.ingest_col_sums(counts, rows).cpu().numpy()          # over the kept genes, every cell
    else:
        x = device.gather_matrix(x, genes=rows)                          # kept genes in genomic order, every cell
        cs = device.col_sums(x).cpu().numpy()
    columns, _, ref, obs = select_cells(cells, cs, annotations, ref_group_names, min_max_counts_per_cell, max_cells_per_group, seed)
    if columns.size == 0:
        raise ValueError("no cell is left after the counts-per-cell filter and the annotations")
    if counts is not None:
        x = device.csc_select(counts, rows, columns)
        expr = x.to_scipy()                                              # genes x cells, float64 data
    else:
        if columns.size != len(cells):
            x = device.gather_matrix(x, cells=columns)
        expr = x.cpu().numpy().T                                         # genes x cells, R's column-major storage
    obj = InfercnvObject(expr_data=expr, count_data=expr, gene_order=GeneOrder(chr=np.array(chrs), start=np.array(start), stop=np.array(stop)),
                         reference_grouped_cell_indices=ref, observation_grouped_cell_indices=obs,
                         options={"chr_exclude": list(chr_exclude) if chr_exclude is not None else None,
                                  "max_cells_per_group": max_cells_per_group,
                                  "min_max_counts_per_cell": list(min_max_counts_per_cell) if min_max_counts_per_cell is not None else None,
                                  "counts_md5": None},
                         gene_names=np.array([genes[r] for r in rows]), cell_names=np.array([cells[j] for j in columns]))
    obj.validate()
    return (obj, x) if return_device else obj
