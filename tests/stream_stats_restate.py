"""Restatement of the ingest and streaming-statistics steps, for tests/test_stream_stats_host.py and
tests/test_gpu_stream_stats.py.

Plain Python and NumPy, no import of the library or of the oracle.  Written from the arithmetic of the R sources
(R/inferCNV_ops.R:2128-2213 gene filters, :3064-3111 normalize_counts_by_seq_depth, :2756-2769 log2xplus1, :3174-3185
scale, :2723-2742 get_average_bounds, :1998-2054 remove_outliers_norm; R/inferCNV_HMM.R:84-99 and R/inferCNV_i3HMM.R:38-52
mean / sd of a block; :1191-1206 / i3 :405-417 proxy values) and from the contracts of include/icnv.h, not from the kernels:

  * integer sums are Python ints (exact at any size),
  * float sums are math.fsum (the correctly rounded sum),
  * a quotient that must be correctly rounded goes through fractions.Fraction,
  * the builders make the count matrices and CSC layouts the GPU tests run on,
  * sum_bound() / ulp_distance() turn "close" into a number that is derived and not measured.

A matrix is a NumPy array of shape (G genes, C cells) throughout, like R's expr.data.
"""
import math
import struct
from fractions import Fraction

import numpy as np

INT32_MAX = 2 ** 31 - 1
U = 2.0 ** -53                      # unit roundoff of a double
CSC_LENGTHS = (0, 1, 63, 64, 65, 130)
CSC_G = 131
# the columns of each CSC layout case: a number is that many stored entries, "dropped" a column whose stored entries all lie
# in genes that keep_mask() drops.  Every length of CSC_LENGTHS occurs; C % 4 is 1, 2, 3, 1, 3 and three cases have C < 4.
CSC_CASES = {1: (65,), 2: (130, 0), 3: (63, "dropped", 64), 5: (0, 1, 63, "dropped", 65), 7: (0, 1, 63, 64, 65, 130, "dropped")}


# ------------------------------------------------------------------ helpers: bounds and ulps
def sum_bound(n, abs_sum):
    """|computed - exact| of a sum of n doubles added in ANY order (trees, chains, lanes): every one of the n - 1 additions
    rounds a partial sum that is at most sum|x| (1 + small), so the error is below n * 2^-53 * sum|x|."""
    return n * U * abs_sum


def _ordered(x):
    i = struct.unpack("<q", struct.pack("<d", float(x)))[0]
    return i if i >= 0 else -(i & 0x7FFFFFFFFFFFFFFF)


def ulp_distance(a, b):
    """Number of doubles between a and b (0 = the same value; -0.0 and 0.0 count as the same)."""
    if math.isnan(a) or math.isnan(b):
        return 0 if (math.isnan(a) and math.isnan(b)) else 2 ** 63
    return abs(_ordered(a) - _ordered(b))


def ulp_distance_array(a, b):
    """ulp_distance elementwise on finite float64 arrays, as int64."""
    def ordered(v):
        i = np.ascontiguousarray(v, dtype=np.float64).view(np.int64)
        return np.where(i >= 0, i, -(i & np.int64(0x7FFFFFFFFFFFFFFF)))
    return np.abs(ordered(a) - ordered(b))


def bits(x):
    """The 64-bit patterns of a float64 array: equality of these sees NaN payloads and the sign of zero."""
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------ exact statistics of integer counts
def keep_mask(G):
    """The keep mask of the column-sum and apply tests: the first gene, the last gene and a run in the middle dropped
    (as far as G allows: G = 1 keeps its gene, G = 2 drops the first)."""
    keep = np.ones(G, dtype=bool)
    if G >= 2:
        keep[0] = False
    if G >= 3:
        keep[G - 1] = False
    if G >= 8:
        keep[G // 2: G // 2 + max(1, G // 16)] = False
    return keep


def gene_stats_int(x):
    """Per gene (sum of the counts, number of cells with count > 0) as Python ints."""
    rows = np.asarray(x).tolist()
    return [sum(r) for r in rows], [sum(1 for v in r if v > 0) for r in rows]


def col_sums_int(x, keep=None):
    """colSums over the kept genes as Python ints."""
    x = np.asarray(x)
    if keep is not None:
        x = x[np.asarray(keep, dtype=bool)]
    return [sum(col) for col in x.T.tolist()]


def partial_sums_below_2_53(x):
    """Every partial sum of any subset of a row or a column stays below 2^53 in magnitude, so a double accumulator is as
    exact as an integer one and "equal" is a fair demand."""
    a = np.abs(np.asarray(x).astype(object))
    big = max([0] + [int(v) for v in a.sum(axis=0).ravel()] + [int(v) for v in a.sum(axis=1).ravel()])
    return big < 2 ** 53


def select_genes(sums, pos, C_total, min_mean_expr_cutoff=None, min_cells_per_gene=0):
    """Step 2: a gene with rowMeans(counts) < cutoff is removed (:2157), then one with fewer than min_cells_per_gene cells
    above zero (:2184).  The mean is compared as an exact rational; mean_gap() says how far the data keep from a tie."""
    keep = []
    for g, (s, n) in enumerate(zip(sums, pos)):
        ok = True
        if min_mean_expr_cutoff is not None:
            ok = not (Fraction(s, C_total) < Fraction(min_mean_expr_cutoff))
        if ok and min_cells_per_gene > 0:
            ok = n >= min_cells_per_gene
        if ok:
            keep.append(g)
    return np.array(keep, dtype=np.int32)


def mean_gap(sums, C_total, cutoff):
    """Smallest |rowMean - cutoff| as a float: above 0 no rounding of the mean can change the decision that matters."""
    return float(min(abs(Fraction(s, C_total) - Fraction(cutoff)) for s in sums))


def r_median(values):
    """stats::median of finite doubles: the middle one, or (a + b) / 2 of the two middle ones."""
    v = sorted(float(t) for t in values)
    n = len(v)
    if n == 0:
        return math.nan
    return v[n // 2] if n % 2 else (v[n // 2 - 1] + v[n // 2]) / 2.0


def apply_counts(x_kept, col_sums, factor, do_normalize=True, do_log2=True):
    """.normalize_data_matrix_by_seq_depth and log2xplus1 on the kept rows: divide, multiply, add, log2 -- each an IEEE
    operation on doubles in R's order.  The first three are correctly rounded everywhere, so NumPy gives R's bits; log2 is
    the platform's."""
    y = np.asarray(x_kept, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        if do_normalize:
            y = y / np.asarray(col_sums, dtype=np.float64)[None, :] * float(factor)
        if do_log2:
            y = np.log2(y + 1.0)
    return y


# ------------------------------------------------------------------ builders: count matrices and CSC layouts
def count_matrix(G, C, seed=0):
    """int32 counts (G, C), about 90 % zeros, small counts otherwise, with the planted entries of the issue:

      * gene `g_big` (kept by keep_mask) holds INT32_MAX in min(5, C) cells: its sum passes 2^32 from three cells on;
      * cell `c_big` holds INT32_MAX in min(3, kept genes) kept genes: its column sum passes 2^32 likewise;
      * for C >= 4 cell `c_zero` is 0 in every kept gene and 7 in every dropped gene: its column sum over the kept genes is 0.

    Returns (x, info) with info = dict(keep, g_big, c_big, c_zero or None)."""
    rng = np.random.default_rng(1000 + seed)
    x = np.where(rng.random((G, C)) < 0.1, rng.integers(1, 60, size=(G, C)), 0).astype(np.int32)
    keep = keep_mask(G)
    kept = np.nonzero(keep)[0]
    c_zero = C // 2 if C >= 4 else None
    free = np.array([c for c in range(C) if c != c_zero])
    g_big = int(kept[len(kept) // 3])
    x[g_big, rng.permutation(free)[:5]] = INT32_MAX
    c_big = int(free[-1])
    x[rng.permutation(kept)[:3], c_big] = INT32_MAX
    if c_zero is not None:
        x[:, c_zero] = np.where(keep, 0, 7)
    return x, {"keep": keep, "g_big": g_big, "c_big": c_big, "c_zero": c_zero}


def dense_to_csc(x, seed=0, explicit_zeros=0.02):
    """CSC arrays (colptr int64, rowidx int32, vals int32) of a dense count matrix: every nonzero, plus a share of the zero
    entries stored explicitly, in a shuffled order inside each column."""
    rng = np.random.default_rng(2000 + seed)
    G, C = x.shape
    colptr, rows, vals = [0], [], []
    for c in range(C):
        col = x[:, c]
        stored = np.nonzero((col != 0) | (rng.random(G) < explicit_zeros))[0]
        stored = rng.permutation(stored)
        rows.append(stored)
        vals.append(col[stored])
        colptr.append(colptr[-1] + stored.size)
    return (np.array(colptr, dtype=np.int64), np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, np.int32),
            np.concatenate(vals).astype(np.int32) if vals else np.zeros(0, np.int32))


def csc_to_dense(colptr, rowidx, vals, G):
    C = len(colptr) - 1
    x = np.zeros((G, C), dtype=np.int32)
    for c in range(C):
        sl = slice(int(colptr[c]), int(colptr[c + 1]))
        x[rowidx[sl], c] = vals[sl]
    return x


def csc_layout(C):
    """The CSC layout case of C cells on CSC_G = 131 genes (CSC_CASES): per column the stated number of stored entries at
    distinct random genes, roughly one in six of them an explicitly stored zero (at least one from two entries on), the
    order shuffled until it is not ascending.  Returns (colptr, rowidx, vals, keep)."""
    rng = np.random.default_rng(3000 + C)
    keep = keep_mask(CSC_G)
    dropped = np.nonzero(~keep)[0]
    colptr, rows, vals = [0], [], []
    for kind in CSC_CASES[C]:
        if kind == "dropped":
            r = dropped.copy()
            v = rng.integers(1, 1000, size=r.size)
        else:
            r = rng.permutation(CSC_G)[:kind]
            v = rng.integers(1, 1000, size=kind)
            v[rng.random(kind) < 1 / 6] = 0
            if kind >= 2:
                v[int(rng.integers(kind))] = 0
            if kind >= 3:
                v[(np.nonzero(v == 0)[0][0] + 1) % kind] = 5      # ... and never only zeros
        order = rng.permutation(r.size)
        while r.size >= 2 and np.all(np.diff(r[order]) > 0):
            order = rng.permutation(r.size)
        rows.append(r[order])
        vals.append(v[order])
        colptr.append(colptr[-1] + r.size)
    return np.array(colptr, dtype=np.int64), np.concatenate(rows).astype(np.int32), np.concatenate(vals).astype(np.int32), keep


# ------------------------------------------------------------------ float statistics
def position_coded(G, C):
    """Integer-valued doubles that name their position: x[g, c] = 1 + g + G * c (all sums far below 2^53).  A dropped
    element changes a sum by its own code, a doubled one likewise."""
    return (1.0 + np.arange(G)[:, None] + G * np.arange(C)[None, :]).astype(np.float64)


def gene_sums_fsum(x):
    return np.array([math.fsum(r) for r in np.asarray(x, dtype=np.float64).tolist()])


def col_sums_fsum(x):
    return np.array([math.fsum(c) for c in np.asarray(x, dtype=np.float64).T.tolist()])


def positive_counts(x):
    """sum(x > 0 & !is.na(x)) per gene: NaN, -0.0 and negatives do not count, +Inf and denormals do."""
    return [sum(1 for v in r if v > 0.0) for r in np.asarray(x, dtype=np.float64).tolist()]


def scale_rows(x):
    """t(scale(t(x))): centre = the gene's mean, scale = sqrt(sum(centred^2) / max(1, C - 1)) (scale.default), the sums
    correctly rounded (fsum).  A constant gene and C = 1 give 0 / 0 = NaN."""
    x = np.asarray(x, dtype=np.float64)
    G, C = x.shape
    out = np.empty_like(x)
    for g in range(G):
        row = x[g].tolist()
        m = math.fsum(row) / C
        cen = [v - m for v in row]
        sc = math.sqrt(math.fsum(d * d for d in cen) / max(1, C - 1))
        out[g] = [d / sc if sc != 0.0 else (math.nan if d == 0.0 else math.copysign(math.inf, d)) for d in cen]
    return out


def scale_input(G, C, seed=0, constant=()):
    """Lognormal rows with a spread that keeps every gene's sd well away from 0, and the planted constant genes."""
    rng = np.random.default_rng(4000 + seed)
    x = rng.lognormal(0.5, 0.8, size=(G, C))
    for g in constant:
        x[g] = 2.5
    return x


def dyadic(G, C, seed=0):
    """Multiples of 2^-20 in (-2^10, 2^10): sums of up to 2^22 of them are exact in a double and in a long double."""
    rng = np.random.default_rng(5000 + seed)
    return rng.integers(-(2 ** 30) + 1, 2 ** 30, size=(G, C)).astype(np.float64) * 2.0 ** -20


def average_bounds(x):
    """get_average_bounds: per cell quantile(x, na.rm = TRUE)[c(1, 5)] = min and max of the values that are not NaN, then
    mean() over the cells.  A cell of nothing but NaN has the quantile NA, and mean() of a vector with an NA is NA: both
    bounds are then NaN.  The means are exact rationals rounded once."""
    x = np.asarray(x, dtype=np.float64)
    lo, hi = [], []
    for col in x.T.tolist():
        vals = [v for v in col if not math.isnan(v)]
        if not vals:
            return math.nan, math.nan
        lo.append(min(vals))
        hi.append(max(vals))
    C = x.shape[1]
    return float(sum(Fraction(v) for v in lo) / C), float(sum(Fraction(v) for v in hi) / C)


def remove_outliers(x, lower, upper):
    """data[data < lower] <- lower; data[data > upper] <- upper (:2049-2051): a NaN fails both tests, -0.0 is not < 0."""
    out = np.array(x, dtype=np.float64, copy=True)
    with np.errstate(invalid="ignore"):
        out[out < lower] = lower
        out[out > upper] = upper
    return out


PROXY = {6: {1: 0.0, 2: 0.5, 3: 1.0, 4: 1.5, 5: 2.0, 6: 3.0}, 3: {1: 0.5, 2: 1.0, 3: 1.5}}


def states_to_proxy(states, K):
    """Every state outside 1..K has no proxy value: NaN."""
    table = np.full(256, np.nan)
    for s, v in PROXY[K].items():
        table[s] = v
    return table[np.asarray(states, dtype=np.uint8)]


# ------------------------------------------------------------------ exact moments
def int_moments(x, cells, mean=None):
    """Over all genes of the listed cells (a cell listed twice counts twice): sum x, or sum (x - mean)^2 for an integer
    mean, as Python ints."""
    vals = [int(v) for c in cells for v in np.asarray(x)[:, c].tolist()]
    return sum(vals) if mean is None else sum((v - mean) ** 2 for v in vals)


def exact_mean_sd(values, scale_log2=0):
    """(mean, sd) of doubles that are integers after multiplication by 2^scale_log2, from exact integer sums: the mean is the
    rational rounded once; the sd is sqrt of the exact rational variance sum (x - mean)^2 / (N - 1) rounded once, then one
    correctly rounded square root (NaN for N = 1, like sd())."""
    sc = 2 ** scale_log2
    ints = [int(v * sc) for v in values]
    assert all(float(i) / sc == float(v) for i, v in zip(ints, values)), "values are not on the 2^-scale_log2 grid"
    N = len(ints)
    S, SS = sum(ints), sum(i * i for i in ints)
    mean = float(Fraction(S, N * sc))
    if N < 2:
        return mean, math.nan
    var = Fraction(SS * N - S * S, N * (N - 1) * sc * sc)
    return mean, math.sqrt(float(var))


def sd_bound(N):
    """Relative bound on sd = sqrt(sum_N (x - mean)^2 / (N - 1)) computed in doubles in any order: each term carries three
    roundings (the difference, the product -- (1 + u)^2 (1 + u)), the sum of N non-negative terms N - 1 more, the division
    one, which the square root halves before adding its own; the rounded mean moves the sum by N (mean - m)^2, second order.
    (N + 8) * 2^-53 covers all of it."""
    return (N + 8) * U


def grid_values(shape, seed=0, scale_log2=24):
    """Real-valued data around 1 (the level the chain's output sits at) on a 2^-24 grid: values are not integers, yet sums
    of up to 2^28 of them are exact in a double, so the mean's only roundings are those of the final division."""
    rng = np.random.default_rng(6000 + seed)
    v = np.clip(rng.normal(1.0, 0.25, size=shape), 0.05, 3.0)
    return np.round(v * 2.0 ** scale_log2) / 2.0 ** scale_log2


# ------------------------------------------------------------------ the shapes both test files run on
INGEST_SHAPES = ((1, 1), (255, 3), (256, 4), (257, 5), (300, 1030), (4113, 37), (5, 8195))
INGEST_CSC_WRAP = (4, 32771)                    # four columns to a block, 8 192 blocks: wraps beyond 32 768 cells
GENE_STATS_SHAPES = ((1, 1), (255, 2), (256, 3), (257, 1030), (4113, 37))
SCALE_SHAPES = ((1, 2), (256, 2), (257, 1030), (700, 37), (5, 8195))
SCALE_CONSTANT = {(1, 2): (), (256, 2): (17,), (257, 1030): (0, 256), (700, 37): (511,), (5, 8195): (4,)}
REDUCE_G = (1, 2, 255, 256, 257, 1025)
REDUCE_C = (1, 37)
WRAP_8192 = (5, 8195)
MOMENTS_G = (1, 2, 3, 255, 256, 257, 511, 512, 513, 1537, 2049, 3585, 3586, 3587, 4097, 7681, 7683, 10001)
MOMENTS_CELLS = (7, 2, 5, 0, 2, 8, 3)           # seven listed cells of nine: unsorted, cell 2 twice, odd and even indices
LIST_N_GENES = (1, 2, 255, 256, 257, 769, 1023, 1024, 1025, 2500)
LIST_G = 2600
LIST_CELLS = (4, 1, 6, 0, 3)


def moments_matrix(G, seed=0):
    """Integers with |v| <= 2^15 on nine cells, as doubles: sums of squares of 7 * 10 001 of them stay below 2^48."""
    rng = np.random.default_rng(7000 + seed)
    x = rng.integers(-(2 ** 15), 2 ** 15 + 1, size=(G, 9)).astype(np.float64)
    x[G - 1, :] = 2.0 ** 15                       # the odd-G leftover element is never a small one
    return x


def gene_list(n_genes, seed=0):
    """n_genes indices into LIST_G genes: with a repeat from two genes on, unsorted from three on."""
    rng = np.random.default_rng(8000 + seed)
    idx = rng.integers(0, LIST_G, size=n_genes)
    if n_genes >= 2:
        idx[-1] = idx[0]
    if n_genes >= 3:
        idx[1] = (idx[0] + 1) % LIST_G          # first == last and another value between them: not ascending
    return idx.astype(np.int32)
