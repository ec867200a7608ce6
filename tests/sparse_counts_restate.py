"""Restatement of the K22 contract (include/icnv.h "sparse count matrices", infercnv_amd.device.read_mtx, DESIGN K22) in plain
Python: bytes.split, int(), lists.  It shares no code with infercnv_amd; the tests compare the library with it array for array.

  reader        the banner, the % comments and the size line; the body's grammar line by line, with the refusal's line, field,
                reason and bytes.  The triplet grammar is the MatrixMarket specification's; scipy.io.mmread is the independent
                check of this reader (tests/test_sparse_counts_host.py).  A value field goes through the Python model of K21's
                field parser (csrc/gen_parse_pow10_table.py: model_field, itself held against float() by
                tests/test_table_parse_host.py) and counts when its double is an integer in 0 .. 2^31 - 1 (value_field).
  make_unique   R's make.unique, from its documentation: a repeated name gets ".1", ".2", ... -- per name the smallest numbers
                that give a string found neither in the input nor among the names already made; make.unique(c("a", "a", "a.2",
                "a")) is "a" "a.1" "a.2" "a.3".
  csc, select   the column pointers of triplets in (col, row) order; rows and columns selected with the entries of a column
                kept in source order.
  writer        a triplet file from a dense table, in a chosen entry order and number spelling.
"""
import gzip
import importlib.util
import os
import re
from fractions import Fraction

import numpy as np

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "infercnv_amd", "csrc")
_spec = importlib.util.spec_from_file_location("gen_parse_pow10_table", os.path.join(_CSRC, "gen_parse_pow10_table.py"))
k21 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(k21)

INT_MAX = 2147483647


class Refusal(Exception):
    """A refused byte of the body: str() is the text after "parse_triplets: "."""

    def __init__(self, line, field, what, shown):
        super().__init__(f"line {line}, field {field}: {what}: '{shown}'")
        self.line, self.field = line, field


def read_bytes(path):
    with (gzip.open(path, "rb") if str(path).endswith(".gz") else open(path, "rb")) as fh:
        return fh.read()


def header(data):
    """(field, G, C, nnz, number of header lines, bytes of the header) of the bytes of a file; ValueError as read_mtx words it."""
    lines = data.split(b"\n")
    toks = lines[0].decode("latin-1").split()
    if not toks or toks[0].lower() != "%%matrixmarket":
        raise ValueError("read_mtx: the banner line must start with %%MatrixMarket")
    if len(toks) != 5:
        raise ValueError(f"read_mtx: the banner has {len(toks)} fields, 5 are expected")
    low = [t.lower() for t in toks]
    if low[1] != "matrix":
        raise ValueError(f"read_mtx: banner object '{toks[1]}': only 'matrix' is read")
    if low[2] != "coordinate":
        raise ValueError(f"read_mtx: banner format '{toks[2]}': only 'coordinate' is read")
    if low[3] not in ("integer", "real", "pattern"):
        raise ValueError(f"read_mtx: banner field '{toks[3]}': only 'integer', 'real' and 'pattern' are read")
    if low[4] != "general":
        raise ValueError(f"read_mtx: banner symmetry '{toks[4]}': only 'general' is read")
    used = len(lines[0]) + 1
    for no in range(1, len(lines)):
        ln = lines[no]
        if no == len(lines) - 1 and ln == b"":
            break
        used += len(ln) + 1
        if ln.startswith(b"%") or ln.strip() == b"":
            continue
        size = ln.split()
        if len(size) != 3 or not all(t.isdigit() and len(t) <= 18 for t in size):
            raise ValueError(f"read_mtx: size line '{ln.decode('latin-1').strip()}': three integers G C nnz are expected")
        G, C, nnz = (int(t) for t in size)
        if not (1 <= G <= INT_MAX and 1 <= C <= INT_MAX):
            raise ValueError("read_mtx: size line: G and C must be 1 .. 2147483647")
        if nnz > G * C:
            raise ValueError(f"read_mtx: size line: {nnz} entries do not fit a {G} x {C} matrix")
        return low[3], G, C, nnz, no + 1, min(used, len(data))
    raise ValueError("read_mtx: the size line is missing")


def index_field(tok, limit):
    """0-based index of a plain unsigned decimal of at most 10 digits in 1 .. limit, or None."""
    if not 1 <= len(tok) <= 10 or any(not 48 <= b <= 57 for b in tok):
        return None
    v = int(tok)
    return v - 1 if 1 <= v <= limit else None


def value_field(tok):
    """The count a value field spells, or None.  The field must be in K21's number grammar with at most 40 bytes and 19
    significant digits, and the double nearest to it an integer in 0 .. 2^31 - 1 (not -0, not NA, NaN or Inf).  Where K21's field
    model certifies the double, that double decides; where it does not (a significand above 2^53 with an exact result, an
    underflow, ...), the field counts exactly when its exact value is such an integer -- the nearest double of any other
    field of at most 19 digits is not an integer."""
    if not 1 <= len(tok) <= 40:
        return None
    got = k21.model_field(bytes(tok))
    if got[0] == "host":
        scanned = k21.scan_field(bytes(tok))
        if scanned[0] != "decimal":                   # more than 19 significant digits
            return None
        _, w, q, neg = scanned
        exact = Fraction(w) * Fraction(10) ** q
        return int(exact) if not neg and exact.denominator == 1 and exact <= INT_MAX else None
    if got[0] != "value":
        return None
    bits = got[1]
    if bits >> 63:
        return None
    x = np.array([bits], dtype=np.uint64).view(np.float64)[0]
    if not np.isfinite(x) or x != np.floor(x) or x > INT_MAX:
        return None
    return int(x)


def parse_body(body, field, G, C, line0=1):
    """The entries [(row, col, val)] (0-based) of the bytes of a body in file order; Refusal at the first refused line."""
    want = 2 if field == "pattern" else 3
    out = []
    pieces = body.split(b"\n")
    for no, ln in enumerate(pieces):
        if ln.endswith(b"\r"):                       # "\r\n", or a "\r" that ends the text
            ln = ln[:-1]
        core = ln.strip(b" \t")
        if core == b"":
            continue
        line = line0 + no
        shown = ln[:60].decode("latin-1")
        if core.startswith(b"%"):
            raise Refusal(line, 1, "a comment line inside the body", shown)
        toks = re.split(rb"[ \t]+", core)
        if len(toks) != want:
            raise Refusal(line, len(toks), f"{len(toks)} fields where {want} are expected", shown)
        r, c = index_field(toks[0], G), index_field(toks[1], C)
        if r is None:
            raise Refusal(line, 1, f"not an index in 1 .. {G}", toks[0][:60].decode("latin-1"))
        if c is None:
            raise Refusal(line, 2, f"not an index in 1 .. {C}", toks[1][:60].decode("latin-1"))
        v = 1
        if want == 3:
            v = value_field(toks[2])
            if v is None:
                raise Refusal(line, 3, "not an integer count in 0 .. 2147483647", toks[2][:60].decode("latin-1"))
        out.append((r, c, v))
    return out


def csc_from_triplets(entries, G, C):
    """(colptr, rowidx, vals, sorted_already): the triplets ordered by (col, row); ValueError on a pair stored twice."""
    keys = [c * G + r for r, c, _ in entries]
    sorted_already = all(keys[k] > keys[k - 1] for k in range(1, len(keys)))
    if not sorted_already:
        order = sorted(range(len(entries)), key=lambda k: keys[k])
        entries = [entries[k] for k in order]
        keys = [keys[k] for k in order]
    for k in range(1, len(keys)):
        if keys[k] == keys[k - 1]:
            raise ValueError(f"duplicate entry for row {entries[k][0] + 1}, column {entries[k][1] + 1}")
    colptr = [0] * (C + 1)
    for _, c, _ in entries:
        colptr[c + 1] += 1
    for c in range(C):
        colptr[c + 1] += colptr[c]
    return (np.array(colptr, dtype=np.int64), np.array([e[0] for e in entries], dtype=np.int32),
            np.array([e[2] for e in entries], dtype=np.int32), sorted_already)


def read_mtx(path):
    """(G, C, colptr, rowidx, vals, sorted_already) of a file, as device.read_mtx must give them."""
    data = read_bytes(path)
    field, G, C, nnz, n_lines, n_bytes = header(data)
    entries = parse_body(data[n_bytes:], field, G, C, line0=n_lines + 1)
    if len(entries) != nnz:
        raise ValueError(f"read_mtx: the size line says {nnz} entries, the body has {len(entries)}")
    return (G, C) + csc_from_triplets(entries, G, C)


def select(colptr, rowidx, vals, G, genes, cells):
    """The CSC arrays of rows `genes` (in their new order) and columns `cells`; a column's entries stay in source order."""
    new_row = {int(g): i for i, g in enumerate(genes)}
    out_ptr, out_row, out_val = [0], [], []
    for c in cells:
        for k in range(int(colptr[c]), int(colptr[c + 1])):
            if int(rowidx[k]) in new_row:
                out_row.append(new_row[int(rowidx[k])])
                out_val.append(int(vals[k]))
        out_ptr.append(len(out_row))
    return np.array(out_ptr, dtype=np.int64), np.array(out_row, dtype=np.int32), np.array(out_val, dtype=np.int32)


def to_dense(colptr, rowidx, vals, G):
    """genes x cells int64 array of CSC arrays."""
    C = len(colptr) - 1
    m = np.zeros((G, C), dtype=np.int64)
    for c in range(C):
        for k in range(int(colptr[c]), int(colptr[c + 1])):
            m[int(rowidx[k]), c] = int(vals[k])
    return m


def make_unique(names, sep="."):
    taken = set(names)
    seen, counter, out = set(), {}, []
    for name in names:
        if name not in seen:
            seen.add(name)
            out.append(name)
            continue
        k = counter.get(name, 1)
        while name + sep + str(k) in taken:
            k += 1
        made = name + sep + str(k)
        taken.add(made)
        counter[name] = k + 1
        out.append(made)
    return out


def write_mtx(path, dense, field="integer", order="column", spell=None, eol=b"\n", final_newline=True, blank_every=0, keep_zero=(),
              comments=(b"% written by the test",), gaps=(b" ",), edge_blanks=False, seed=0):
    """Write the non-zero entries of a genes x cells integer table (and the explicit zeros at the (row, col) pairs of keep_zero)
    as a coordinate file.  order: "column" (column-major, sorted), "row" (row-major) or "shuffle" (seeded).  spell(k, v): the
    bytes of the value of the k-th entry written (default: the plain integer).  gaps: the runs of blanks between fields, used
    in turn; edge_blanks: every third line begins with a blank and every fourth ends with one.  eol: a line end, or a callable k -> line end.  blank_every: a blank line after every such number of entries.
    Returns the entries [(row, col, val)] in the order written."""
    dense = np.asarray(dense)
    G, C = dense.shape
    zero = set(keep_zero)
    entries = [(r, c, int(dense[r, c])) for c in range(C) for r in range(G) if dense[r, c] != 0 or (r, c) in zero]
    if order == "row":
        entries.sort(key=lambda e: (e[0], e[1]))
    elif order == "shuffle":
        perm = np.random.default_rng(seed).permutation(len(entries))
        entries = [entries[k] for k in perm]
    out = [b"%%MatrixMarket matrix coordinate " + field.encode() + b" general\n"]
    out += [c + b"\n" for c in comments]
    out.append(b"%d %d %d\n" % (G, C, len(entries)))
    for k, (r, c, v) in enumerate(entries):
        gap1, gap2 = gaps[k % len(gaps)], gaps[(k + 1) % len(gaps)]
        text = b"%d" % (r + 1) + gap1 + b"%d" % (c + 1)
        if field != "pattern":
            text += gap2 + (spell(k, v) if spell else b"%d" % v)
        if edge_blanks:
            text = (b" " if k % 3 == 0 else b"") + text + (b"\t" if k % 4 == 0 else b"")
        end = eol(k) if callable(eol) else eol
        if k == len(entries) - 1 and not final_newline:
            end = b""
        out.append(text + end)
        if blank_every and (k + 1) % blank_every == 0 and k != len(entries) - 1:
            out.append(b"\r\n" if k % 2 else b"\n")
    data = b"".join(out)
    with (gzip.open(path, "wb") if str(path).endswith(".gz") else open(path, "wb")) as fh:
        fh.write(data)
    return entries


def compare(cor, obj, want):
    """Assert that an InfercnvObject of the sparse route equals create_object's dict in every slot, the matrix after toarray()."""
    import copy
    assert obj.count_data is obj.expr_data and hasattr(obj.expr_data, "tocsc") and obj.expr_data.dtype == np.float64
    dense = copy.copy(obj)
    dense.expr_data = dense.count_data = np.ascontiguousarray(obj.expr_data.toarray())
    cor.compare(dense, want)


def sparse_create_object(cor, mtx_path, genes, cells, gene_order, annotations, ref_group_names, **kw):
    """The sparse route of CreateInfercnvObject restated on top of create_object_restate (`cor`): the file is read, expanded, and
    handed to the dense restatement, whose slots the sparse route must reproduce (the matrix after toarray())."""
    G, C, colptr, rowidx, vals, _ = read_mtx(mtx_path)
    if (G, C) != (len(genes), len(cells)):
        raise ValueError("the names do not fit the matrix")
    x = to_dense(colptr, rowidx, vals, G).astype(np.float64)
    return cor.create_object(list(genes), list(cells), x.view(np.int64), gene_order, annotations, ref_group_names, **kw)
