"""A sequential restatement of K34 (include/icnv.h "K34"): payload bytes -> values with struct / NumPy on the host, and the CSC
rules as a plain loop that returns the same status record as icnv_rds_csc_check_dev.  Nothing here shares code with the
kernels: the byte order is NumPy's big-endian dtypes, the count test is floating-point comparison, the checks are loops."""
import math
import struct

import numpy as np

INT, REAL = 13, 14                                          # ICNV_RDS_INT, ICNV_RDS_REAL: the SEXP types
OK, P_FIRST, P_DESCENT, P_LAST, ROW_RANGE, ROW_ORDER, VALUE = range(7)      # ICNV_RDS_*
NA_REAL_BITS = 0x7FF00000000007A2
NA_INTEGER = -2 ** 31


def column_bits(stream, off, kind, rows):
    """The bits (uint64) of the `rows` doubles an output column holds: the elements of `kind` at byte `off` of `stream`."""
    if kind == REAL:
        return np.frombuffer(stream, dtype=">u8", count=rows, offset=off).astype(np.uint64)
    v = np.frombuffer(stream, dtype=">i4", count=rows, offset=off).astype(np.int64)
    bits = v.astype(np.float64).view(np.uint64).copy()
    bits[v == NA_INTEGER] = NA_REAL_BITS
    return bits


def columns(stream, col_off, col_kind, rows):
    """(n_out, rows) uint64: icnv_rds_columns_dev's output, as bits."""
    return np.stack([column_bits(stream, int(o), int(k), rows) for o, k in zip(col_off, col_kind)])


def count_of(bits):
    """The count a double's bits stand for, or -1: an integer value in 0 .. 2^31 - 1."""
    v = struct.unpack("<d", struct.pack("<Q", int(bits)))[0]
    if v != v or math.isinf(v) or v < 0 or v > 2 ** 31 - 1 or v != math.floor(v):
        return -1
    return int(v)


def csc_check(i, p, x_bits, G, C, nnz, cells=None):
    """(code, file column, index) as icnv_rds_csc_check_dev reports it.  i, p: Python ints; x_bits: the doubles' bits."""
    for j in range(C + 1):                                   # the whole of p, in index order; the smallest code at an index
        if j == 0 and p[0] != 0:
            return P_FIRST, 0, 0
        if j > 0 and p[j] < p[j - 1]:
            return P_DESCENT, min(j, C - 1), j
        if j == C and p[C] != nnz:
            return P_LAST, C - 1, C
    best = None
    for c in (range(C) if cells is None else cells):
        for e in range(p[c], p[c + 1]):
            code = OK
            if not 0 <= i[e] < G:
                code = ROW_RANGE
            elif e > p[c] and i[e - 1] >= i[e]:
                code = ROW_ORDER
            elif count_of(x_bits[e]) < 0:
                code = VALUE
            if code and (best is None or e < best[2]):
                best = (code, c, e)
    return best if best is not None else (OK, -1, -1)


def csc_fill(i, p, x_bits, C, cells=None):
    """(colptr, rowidx, vals) of the selected columns in the list's order, a column's entries in stream order."""
    sel = list(range(C)) if cells is None else list(cells)
    colptr, rowidx, vals = [0], [], []
    for c in sel:
        for e in range(p[c], p[c + 1]):
            rowidx.append(i[e])
            vals.append(count_of(x_bits[e]))
        colptr.append(len(rowidx))
    return np.array(colptr, dtype=np.int64), np.array(rowidx, dtype=np.int32), np.array(vals, dtype=np.int32)


# the special values of the tests and of the host check's corpus
REAL_SPECIALS = [NA_REAL_BITS, 0x7FF8000000000001, 0xFFF0000000ABCDEF, 0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000,
                 0xFFF0000000000000, 0x0000000000000001, 0x800FFFFFFFFFFFFF, 0x3FF0000000000000, 0x40C3880000000000]
INT_SPECIALS = [NA_INTEGER, NA_INTEGER + 1, 2 ** 31 - 1, 0, 1, -1, 6927]
COUNT_SPECIALS = [0x0000000000000000, 0x8000000000000000, 0x3FF0000000000000, 0x3FE0000000000000, 0xBFF0000000000000,
                  0x41DFFFFFFFC00000,     # 2^31 - 1
                  0x41E0000000000000,     # 2^31
                  0x41DFFFFFFFE00000,     # 2^31 - 0.5
                  0x7FF8000000000000, NA_REAL_BITS, 0x7FF0000000000000, 0xFFF0000000000000, 0x0000000000000001,
                  0x3FF0000000000001, 0x4008000000000000, 0x4330000000000000, 0x4035800000000000]


def real_payload(n, seed):
    """n doubles as bits: the specials first, then seeded random bit patterns."""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2 ** 64, size=n, dtype=np.uint64)
    k = min(n, len(REAL_SPECIALS))
    bits[:k] = np.array(REAL_SPECIALS[:k], dtype=np.uint64)
    return bits


def int_payload(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.integers(-2 ** 31, 2 ** 31, size=n, dtype=np.int64)
    k = min(n, len(INT_SPECIALS))
    v[:k] = INT_SPECIALS[:k]
    return v.astype(np.int32)
