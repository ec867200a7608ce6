"""Plain restatements of what the group-level HMM kernels of viterbi_kernels.hip promise (group means, the reference cells'
shifted moments, the i3 parameters, state consensus, proxy values), in exact or 50-digit arithmetic.  No GPU, no project code:
tests/test_group_hmm_host.py ties this file to independent references, tests/test_gpu_group_hmm.py holds the kernels to it.

Matrices are (G, C) numpy arrays, genes by cells, as in the oracles; groups are lists of cell indices.
"""
import math
from fractions import Fraction

import mpmath
import numpy as np

U = 2.0 ** -53           # unit roundoff of binary64


# ------------------------------------------------------------------ exact sums and means
def exact_sum(values):
    """The sum of finite doubles as a Fraction: every double is an integer multiple of 2^-1074."""
    m, e = np.frexp(np.asarray(values, dtype=np.float64))
    mant = (m * 2.0 ** 53).astype(np.int64).tolist()                     # exact: |m| < 1 has 53 significant bits
    exps = (e.astype(np.int64) - 53).tolist()
    if not mant:
        return Fraction(0)
    emin = min(exps)
    total = sum(a << (b - emin) for a, b in zip(mant, exps))
    return Fraction(total) * Fraction(2) ** emin


def r_nonfinite_mean(values):
    """rowMeans' answer for a row with a non-finite value (a long double sum, then one division): NaN if there is a NaN or
    infinities of both signs, the signed infinity otherwise."""
    v = np.asarray(values, dtype=np.float64)
    if np.isnan(v).any() or (np.isposinf(v).any() and np.isneginf(v).any()):
        return math.nan
    return math.inf if np.isposinf(v).any() else -math.inf


def exact_group_means(x, groups):
    """(G, n_groups): per gene and group the exact mean of the group's cells rounded ONCE (float(Fraction) rounds correctly,
    ties to even); r_nonfinite_mean where a value is not finite."""
    x = np.asarray(x, dtype=np.float64)
    out = np.empty((x.shape[0], len(groups)))
    for q, cells in enumerate(groups):
        sub = x[:, np.asarray(cells, dtype=np.int64)]
        finite = np.isfinite(sub).all(axis=1)
        for g in range(x.shape[0]):
            out[g, q] = float(exact_sum(sub[g]) / sub.shape[1]) if finite[g] else r_nonfinite_mean(sub[g])
    return out


def cancellation_ratio(values):
    """sum |x| / |sum x| as a float (inf for a zero sum): how many leading bits the summation cancels."""
    s = exact_sum(values)
    return math.inf if s == 0 else float(exact_sum(np.abs(values)) / abs(s))


def rounding_margin(mean):
    """How far the exact mean (a nonzero Fraction) is from the nearest point where its rounding to double changes -- the
    midpoint of two neighbouring doubles -- relative to |mean|.  An approximation of the mean whose relative error is below
    this margin rounds to the same double as the mean itself."""
    m = float(mean)
    mids = [(Fraction(m) + Fraction(math.nextafter(m, d))) / 2 for d in (math.inf, -math.inf)]
    return float(min(abs(mean - h) for h in mids) / abs(mean))


# ------------------------------------------------------------------ shifted moments and the i3 parameters
def exact_moments(x, ref_cells):
    """Over all genes of the reference cells: (S1, S2, n, A1, A2) with S1 = sum (x - 1), S2 = sum (x - 1)^2 as Fractions,
    n the number of values, and A1 = sum |x - 1|, A2 = sum (x - 1)^2 as floats for error bounds."""
    x = np.asarray(x, dtype=np.float64)
    vals = x[:, np.asarray(ref_cells, dtype=np.int64)].ravel(order="F")
    # every value as an integer on one grid 2^emin (emin <= 0, so that 1 is on the grid too): Python integers from there
    m, e = np.frexp(vals)
    mant = (m * 2.0 ** 53).astype(np.int64).tolist()
    exps = (e.astype(np.int64) - 53).tolist()
    emin = min(exps + [0])
    one = 1 << -emin
    d = [(a << (b - emin)) - one for a, b in zip(mant, exps)]
    scale = Fraction(2) ** emin
    S1, S2, A1 = Fraction(sum(d)) * scale, Fraction(sum(t * t for t in d)) * scale * scale, Fraction(sum(abs(t) for t in d)) * scale
    return S1, S2, len(d), float(A1), float(S2)


def i3_params(S1, S2, n, z, delta_abs=None):
    """(mu, sigma, delta, (mu - delta, mu, mu + delta)) from the exact shifted moments: mu = 1 + S1 / n,
    sigma = sqrt((S2 - S1^2 / n) / (n - 1)), delta = delta_abs if given, else sigma z.  Rational up to the square root, 50
    digits from there, each value rounded once at the end."""
    with mpmath.workdps(50):
        mu = 1 + Fraction(S1) / n
        var = (Fraction(S2) - Fraction(S1) ** 2 / n) / (n - 1)
        sigma = mpmath.sqrt(mpmath.mpf(var.numerator) / mpmath.mpf(var.denominator))
        delta = mpmath.mpf(float(delta_abs)) if delta_abs is not None else sigma * mpmath.mpf(float(z))
        mu_mp = mpmath.mpf(mu.numerator) / mpmath.mpf(mu.denominator)
        return float(mu), float(sigma), float(delta), (float(mu_mp - delta), float(mu), float(mu_mp + delta))


def sigma_condition(S1, S2, n):
    """kappa = S2 / (S2 - S1^2 / n): how much the subtraction in the variance amplifies a relative error of S1^2 / n."""
    return float(Fraction(S2) / (Fraction(S2) - Fraction(S1) ** 2 / n))


# ------------------------------------------------------------------ states
def consensus(states_u8, groups):
    """.get_state_consensus: t = table(x) lists the values present in ascending order (-1, stored 255, first);
    order(t, decreasing = TRUE)[1] is the first of the largest counts.  (G, n_groups) uint8."""
    st = np.asarray(states_u8, dtype=np.uint8)
    out = np.empty((st.shape[0], len(groups)), dtype=np.uint8)
    for q, cells in enumerate(groups):
        for g in range(st.shape[0]):
            vals = [-1 if s == 255 else s for s in st[g, np.asarray(cells, dtype=np.int64)].tolist()]
            table = [(v, vals.count(v)) for v in sorted(set(vals))]
            best = table[0]
            for entry in table[1:]:
                if entry[1] > best[1]:
                    best = entry
            out[g, q] = 255 if best[0] == -1 else best[0]
    return out


# assign_HMM_states_to_proxy_expr_vals: 1 -> 0, 2 -> 0.5, 3 -> 1, 4 -> 1.5, 5 -> 2, 6 -> 3;
# i3HMM_assign_HMM_states_to_proxy_expr_vals: 1 -> 0.5, 2 -> 1, 3 -> 1.5
PROXY = {6: {1: 0.0, 2: 0.5, 3: 1.0, 4: 1.5, 5: 2.0, 6: 3.0}, 3: {1: 0.5, 2: 1.0, 3: 1.5}}


def proxy(states_u8, K):
    """The proxy expression value of every state byte; a byte that is no state of the K-state model has none: NaN."""
    st = np.asarray(states_u8, dtype=np.uint8)
    out = np.full(st.shape, np.nan)
    for s, v in PROXY[K].items():
        out[st == s] = v
    return out


# ------------------------------------------------------------------ builders
def integer_matrix(G, C, seed, lo=-3, hi=6):
    """Integers lo .. hi as doubles: every x - 1, (x - 1)^2 and every sum of them is an integer far below 2^53, exact in
    any order of addition."""
    return np.random.default_rng(seed).integers(lo, hi + 1, size=(G, C)).astype(np.float64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# group_means_nsplit of viterbi_kernels.hip: the slices a group's cells are cut into
def nsplit(G, n_grp):
    tiles = (G + 255) // 256
    return max(1, min(64, -(-2048 // (tiles * n_grp))))


MEAN_SIZES = (1, 2, 3, 63, 64, 65, 129)
RATIO_CAP = 2.0 ** 40


def mean_groups(seed, sizes=MEAN_SIZES, extra=0):
    """Disjoint groups of the given sizes drawn from a permutation of sum(sizes) + extra cells, and the cells left over."""
    n = sum(sizes)
    perm = np.random.default_rng(seed).permutation(n + extra)
    groups, at = [], 0
    for s in sizes:
        groups.append(perm[at:at + s].astype(np.int32))
        at += s
    return groups, perm[at:].astype(np.int32)


def dd_margin_needed(n, ratio):
    """What the kernels' double-double arithmetic loses, relative to the group's sum, at most (first order in 2^-53).
    Two-sum is exact, so after every addition hi + (sum of the error terms) is the exact sum; the only loss is in adding the
    error terms into lo.  There are at most T = n + 2 * 64 + 2 such additions on the way to one mean (n in the slices' lanes,
    one when a lane joins its two accumulators, two per slice in the finish kernel, at most 64 slices), every error term is
    at most u * A (A = sum |x| bounds every partial sum), so |lo| <= T u A throughout and every addition into lo loses at most
    u |lo|: T^2 u^2 A in all, T^2 u^2 ratio relative to the sum.  The quotient from the pair adds less than 4 u^2 (remainder
    by fma exact; the correction (r + e) / n, itself below u |q0|, is rounded twice).  A mean whose rounding_margin exceeds
    this rounds to the same double from the pair as from the exact sum."""
    T = n + 2 * 64 + 2
    return U * U * (T * T * ratio + 4.0)


def means_matrix(G, groups, C, seed):
    """(G, C) matrix for the correctly-rounded-mean test, three kinds of genes in turn, gene g of kind (g + 2 G) mod 3:
      0  values near 1 (the HMM's input);
      1  magnitudes 1e-8 .. 1e8, log-uniform, random signs;
      2  values of 1e4 .. 4e4 with planted cancelling pairs +P, -P inside every group of three cells or more (two pairs in
         the group of 129, one elsewhere), P = 1e15 where the group's remaining sum keeps sum |x| / |sum x| below 2^31, a
         smaller P otherwise: between +P and -P the running sum carries no bit below 0.125 and the low word everything.
    Every (gene, group) meets two conditions that make "correctly rounded" decidable for double-double arithmetic, both
    asserted by the test that uses the matrix: sum |x| / |sum x| < 2^40 (RATIO_CAP), and, in a group of three cells or more,
    rounding_margin(mean) > dd_margin_needed(n, ratio) (gene_group_ok).  A gene that misses one is drawn again from the next
    sub-seed."""
    x = np.empty((G, C))
    for g in range(G):
        for attempt in range(100):
            rng = np.random.default_rng([seed, g, attempt])
            kind = (g + 2 * G) % 3                                               # (a matrix of one gene gets kind 2)
            if kind == 0:
                col = 1.0 + 0.1 * rng.standard_normal(C)
            elif kind == 1:
                col = rng.choice([-1.0, 1.0], size=C) * 10.0 ** rng.uniform(-8.0, 8.0, size=C)
            else:
                col = rng.uniform(1e4, 4e4, size=C)
                for cells in groups:
                    n = len(cells)
                    if n < 3:
                        continue
                    k = 1 if n < 129 else 2
                    where = rng.choice(n, size=2 * k, replace=False)
                    rest = float(np.delete(col[cells], where).sum())
                    P = min(1e15, 2.0 ** 31 * rest / (2 * k))
                    col[cells[where[:k]]] = P
                    col[cells[where[k:]]] = -P
            if all(gene_group_ok(col[cells]) for cells in groups):
                break
        else:
            raise AssertionError("no admissible column in 100 draws")
        x[g] = col
    return x


def gene_group_ok(values):
    """Both conditions of means_matrix for one (gene, group).  A group of one or two cells needs no margin: the only error
    term there is added into lo = 0, so the pair is the exact sum and the quotient is rounded once -- ties (half of all means
    of two doubles) included, to even."""
    ratio = cancellation_ratio(values)
    if not ratio < RATIO_CAP:
        return False
    return len(values) <= 2 or rounding_margin(exact_sum(values) / len(values)) > dd_margin_needed(len(values), ratio)
