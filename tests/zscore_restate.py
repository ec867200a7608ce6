"""Exact restatement of the K32 contract (include/icnv.h "reference z-score gene filter", DESIGN K32), written from the header
and R/inferCNV_tumor_subclusters.R:45-71, not from the kernels: every sum is taken over fractions.Fraction -- the exact real
sum -- and rounded to double once, to nearest with ties to even.

    mean      = RN(sum(v) / N)                              over the N = n_ref * G values of the listed cells
    sd        = RN(sqrt(sum((v - mean)^2) / (N - 1)))       around the ROUNDED mean; NaN when N < 2
    row_mean  = RN(sum_c z[g, c] / n_ref)  with  z = |RN(RN(v - mean) / sd)|   (two fp64 operations, as R's (ref - mean) / sd)

A non-finite value among the listed cells makes everything NaN (the header says so; R would say otherwise for infinities).
x is the (G, C) matrix as the object holds it; ref_cells are 0-based columns, duplicates count as often as they are listed.
"""
from fractions import Fraction
import math

import numpy as np


def round_fraction(q):
    """The double nearest to the Fraction q (ties to even); +-inf beyond the range.  CPython's int / int is correctly rounded."""
    try:
        return q.numerator / q.denominator
    except OverflowError:
        return math.inf if q > 0 else -math.inf


def round_sqrt_fraction(q):
    """The double nearest to sqrt(q) for a Fraction q >= 0: the integer square root with 128 spare bits brackets sqrt(q)
    between two rationals a step of 2^-t apart; they round to the same double unless a rounding boundary lies between them,
    and then the boundary's square is compared with q exactly."""
    if q == 0:
        return 0.0
    a, b = q.numerator, q.denominator
    t = max(0, 128 - (a.bit_length() - b.bit_length()) // 2)
    root = math.isqrt((a << (2 * t)) // b)                     # floor(sqrt(q) * 2^t)
    lo, hi = round_fraction(Fraction(root, 1 << t)), round_fraction(Fraction(root + 1, 1 << t))
    if lo == hi:
        return lo
    assert math.nextafter(lo, math.inf) == hi and math.isfinite(hi)
    mid = (Fraction(lo) + Fraction(hi)) / 2                     # the only boundary between two neighbouring doubles
    if mid * mid == q:                                          # a tie: to even
        return lo if (np.float64(lo).view(np.uint64) & 1) == 0 else hi
    return lo if q < mid * mid else hi


def zscore_gene_filter(x, ref_cells):
    """(mean, sd, row_mean[G]) of the contract above."""
    x = np.asarray(x, dtype=np.float64)
    ref_cells = np.asarray(ref_cells, dtype=np.int64)
    G = x.shape[0]
    ref = x[:, ref_cells]                                       # (G, n_ref)
    n_ref = ref_cells.size
    N = G * n_ref
    nan = float("nan")
    if not np.isfinite(ref).all():
        return nan, nan, np.full(G, nan)
    values = [Fraction(float(v)) for v in ref.ravel()]
    mean = round_fraction(sum(values, Fraction(0)) / N)
    if N < 2:
        return mean, nan, np.full(G, nan)
    fm = Fraction(mean)
    sd = round_sqrt_fraction(sum(((v - fm) ** 2 for v in values), Fraction(0)) / (N - 1))
    with np.errstate(all="ignore"):
        z = np.abs((ref - np.float64(mean)) / np.float64(sd))  # two correctly rounded fp64 operations per element
    row_mean = np.empty(G, dtype=np.float64)
    for g in range(G):
        if not np.isfinite(z[g]).all():
            row_mean[g] = nan
        else:
            row_mean[g] = round_fraction(sum((Fraction(float(v)) for v in z[g]), Fraction(0)) / n_ref)
    return mean, sd, row_mean
