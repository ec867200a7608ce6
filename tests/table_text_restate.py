"""Restatement of the K20 contract (include/icnv.h "matrix files of plot_cnv", DESIGN K20): the text of one field from the exact
decimal value of the double, rounded with the decimal module -- no "%.14e" anywhere -- and the rows and files built from it."""
import math
from decimal import ROUND_HALF_EVEN, Context, Decimal
from fractions import Fraction

_CTX = Context(prec=15, rounding=ROUND_HALF_EVEN, Emin=-999999, Emax=999999)


def field(x):
    """The text of one number: 15 significant digits of the exact value, ties to even, trailing zeros dropped, fixed notation
    unless scientific is strictly narrower, a two-digit exponent (three from 100 on)."""
    x = float(x)
    if x != x:
        return "NaN"
    if math.isinf(x):
        return "Inf" if x > 0 else "-Inf"
    if x == 0.0:
        return "0"
    r = _CTX.create_decimal(Decimal(abs(x)))          # Decimal(float) is exact; the context rounds to 15 digits
    e = r.adjusted()
    digits = "".join(str(d) for d in r.as_tuple().digits).rstrip("0")
    nsig = len(digits)
    neg = "-" if x < 0 else ""
    w_sci = len(neg) + (nsig + 1 if nsig > 1 else 1) + (4 if abs(e) < 100 else 5)
    right = max(0, nsig - e - 1)
    w_fix = len(neg) + (e + 1 if e >= 0 else 1) + (right + 1 if right else 0)
    if w_fix <= w_sci:
        if e >= 0:
            whole = digits[:e + 1].ljust(e + 1, "0")
            frac = digits[e + 1:]
        else:
            whole, frac = "0", "0" * (-e - 1) + digits
        return neg + whole + ("." + frac if frac else "")
    return neg + digits[0] + ("." + digits[1:] if nsig > 1 else "") + ("e+" if e >= 0 else "e-") + "%02d" % abs(e)


def is_exact_tie(x):
    """Does the exact value of x lie half way between two 15-digit decimals?"""
    x = float(x)
    if x != x or math.isinf(x) or x == 0.0:
        return False
    v = Fraction(abs(x))
    e = 0
    while Fraction(10) ** (e + 1) <= v:
        e += 1
    while Fraction(10) ** e > v:
        e -= 1
    scaled = v * Fraction(10) ** (14 - e)
    return scaled - math.floor(scaled) == Fraction(1, 2)


def quote(s):
    return '"' + str(s).replace('"', '\\"') + '"'


def rows(x_gc, orientation, cells, row0, n_rows, labels=None, sep=" "):
    """The file rows row0 .. row0 + n_rows - 1 as a list of bytes.  x_gc[g, c]; labels: one bytes per row of the range, as
    written (the caller quotes), or None."""
    out = []
    for i in range(n_rows):
        r = row0 + i
        vals = [x_gc[r, c] for c in cells] if orientation == "gene_rows" else list(x_gc[:, cells[r]])
        line = sep.join(field(v) for v in vals).encode()
        if labels is not None:
            line = labels[i] + sep.encode() + line
        out.append(line + b"\n")
    return out


def file_bytes(x_gc, orientation, cells, row_names=None, col_names=None, quoted=True, sep=" "):
    """write.table's file: the header of column names, then one row per gene (gene_rows) or per listed cell (cell_rows)."""
    q = quote if quoted else str
    n = x_gc.shape[0] if orientation == "gene_rows" else len(cells)
    head = b"" if col_names is None else (sep.join(q(str(c)) for c in col_names) + "\n").encode()
    labels = None if row_names is None else [q(str(r)).encode() for r in row_names]
    return head + b"".join(rows(x_gc, orientation, cells, 0, n, labels, sep))
