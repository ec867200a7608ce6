"""Operating points shared by tests/test_gpu_de_edges.py and tests/test_de_host.py (DESIGN K12): inputs that steer the rank-sum
and Welch p-values into every branch of pnorm2 / pt2, the CPU-side classification of the branch a (comparison, gene) takes,
and an exact mean that is fast enough for matrices of millions of values.  Everything here is built from tests/de_restate.py."""
import math
from fractions import Fraction

import numpy as np

import de_restate as dr

PNORM_EDGES = (0.67448975, 5.656854249492380195206754896838, 37.5193)
PNORM_POINTS = (1e-9, 0.67448975, 0.6744898, 5.65685, 5.65686, 11.67, 27.0, 37.0)


def sized_groups(sizes):
    out, o = [], 0
    for s in sizes:
        out.append(np.arange(o, o + s))
        o += s
    return out, o


def wilcox_z(xv, yv):
    """The z that dr.wilcox hands to pnorm2, or None where it takes the exact table."""
    W, _, T = dr.wilcox(xv, yv)
    nx = sum(1 for v in xv if math.isfinite(v))
    ny = sum(1 for v in yv if math.isfinite(v))
    if nx <= dr.EXACT_MAX and ny <= dr.EXACT_MAX and T == 0:
        return None
    dx, dy = float(nx), float(ny)
    z0 = W - dx * dy / 2.0
    sigma = math.sqrt((dx * dy / 12.0) * ((dx + dy + 1.0) - float(T) / ((dx + dy) * (dx + dy - 1.0))))
    corr = 0.5 if z0 > 0 else (-0.5 if z0 < 0 else 0.0)
    return (z0 - corr) / sigma if sigma != 0.0 else math.nan


def pnorm_regime(z):
    """0: NaN; 1: |z| <= 0.674..; 2: <= 5.657; 3: < 37.5193; 4: beyond (p exactly 0)."""
    if z != z:
        return 0
    y = abs(z)
    if y <= PNORM_EDGES[0]:
        return 1
    if not (y < PNORM_EDGES[2]):
        return 4
    return 2 if y <= PNORM_EDGES[1] else 3


def wilcoxon_ladder():
    """(expr, groups, comparisons): one gene per rung -- same distribution, a 0.6 shift between the 60-cell groups, 50 vs 500
    fully separated, 1000 vs 1000 fully separated (compared both ways), all values equal.  The last two comparisons take
    the first 940 and the first 938 cells of the two 1000-cell groups: fully separated n vs n gives |z| = 37.539 and 37.4998,
    the two sides of pnorm's 37.5193 cut at a point where exp_lib has not yet underflowed (it does from |z| = 37.63), so only
    the cut itself makes the first one exactly 0."""
    groups, C = sized_groups([60, 60, 50, 500, 1000, 1000])
    rng = np.random.default_rng(41)
    expr = np.round(rng.normal(0.0, 1.0, size=(5, C)), 3)
    expr[1, groups[1]] += 0.6
    expr[2, groups[2]] += 100.0
    expr[3, groups[4]] -= 100.0
    expr[3, groups[5]] += 100.0
    expr[4, :] = 1.5
    groups += [groups[4][:940], groups[5][:940], groups[4][:938], groups[5][:938]]
    return expr, groups, [(0, 1), (2, 3), (4, 5), (5, 4), (6, 7), (8, 9)]


def wilcoxon_regimes(expr, groups, comparisons):
    """pnorm_regime of every (comparison, gene) (-1 for the exact table)."""
    out = np.full((len(comparisons), expr.shape[0]), -1)
    for k, (qx, qy) in enumerate(comparisons):
        for g in range(expr.shape[0]):
            z = wilcox_z(expr[g, groups[qx]].tolist(), expr[g, groups[qy]].tolist())
            if z is not None:
                out[k, g] = pnorm_regime(z)
    return out


def exact_ends():
    """(expr, groups, comparisons): distinct values, so every comparison below 50 takes the exact table; gene 0 ascending and
    gene 1 descending in cell order separate every pair of groups fully (W = 0 or n.x n.y), gene 2 is a permutation."""
    groups, C = sized_groups([1, 1, 49, 49, 50])
    expr = np.empty((3, C))
    expr[0] = np.arange(C) * 0.25 - 7.0
    expr[1] = expr[0, ::-1]
    expr[2] = np.random.default_rng(43).permutation(C) * 0.5
    return expr, groups, [(0, 1), (1, 0), (0, 2), (2, 0), (2, 3), (3, 2), (2, 4), (4, 2)]


WELCH_RUNGS = ("t0", "df_under_20", "df_over_20", "df_1", "tail", "zero")


def welch_ladder():
    """(expr, groups, comparisons): rung r is gene r and comparison r = (groups 2r, 2r + 1); the other cells of a gene hold
    plain normal data.
      t0           equal means, nonzero variance: t = 0 exactly, p = 1
      df_under_20  11 vs 11 with a variance ratio of 1.05^2: df a little below 20, the ratio loop of lgamma_diff_half runs
      df_over_20   12 vs 12 with a variance ratio of 0.724^2: df a little above 20, the loop does not run
      df_1         2 vs 2, one sample constant: df = 1
      tail         30 vs 30, means 8 sd apart: p between 1e-300 and 1e-10
      zero         1000 vs 1000, means 1000 sd apart: exp_lib underflows and p is exactly 0"""
    sizes = [3, 3, 11, 11, 12, 12, 2, 2, 30, 30, 1000, 1000]
    groups, C = sized_groups(sizes)
    rng = np.random.default_rng(47)
    expr = rng.normal(0.0, 1.0, size=(len(WELCH_RUNGS), C))
    expr[0, groups[0]] = [1.0, 2.0, 3.0]
    expr[0, groups[1]] = [0.0, 2.0, 4.0]
    b11 = rng.normal(0.0, 1.0, size=11)
    expr[1, groups[2]] = b11
    expr[1, groups[3]] = 1.05 * b11 + 0.2
    b12 = rng.normal(0.0, 1.0, size=12)
    expr[2, groups[4]] = b12
    expr[2, groups[5]] = 0.724 * b12 + 0.2
    expr[3, groups[6]] = [0.0, 1.0]
    expr[3, groups[7]] = [5.0, 5.0]
    expr[4, groups[9]] += 8.0
    expr[5, groups[11]] += 1000.0
    return expr, groups, [(2 * r, 2 * r + 1) for r in range(len(WELCH_RUNGS))]


def welch_points(expr, groups, comparisons):
    """(t, df, p) of dr.welch per (comparison, gene)."""
    out = np.empty((len(comparisons), expr.shape[0], 3))
    for k, (qx, qy) in enumerate(comparisons):
        for g in range(expr.shape[0]):
            t, p, df = dr.welch(expr[g, groups[qx]].tolist(), expr[g, groups[qy]].tolist())
            out[k, g] = (t, df, p)
    return out


def pt_side(t, df):
    """The continued fraction pt2 evaluates: "lower" I_x(a, b) directly, "upper" 1 - I_{1-x}(b, a)."""
    a, b = df * 0.5, 0.5
    return "lower" if df / (df + t * t) < (a + 1.0) / (a + b + 2.0) else "upper"


def check_wilcoxon_ladder(reg):
    """Every regime of pnorm2 holds a (comparison, gene) of wilcoxon_ladder(), the designed rungs where they were aimed."""
    assert (reg >= 0).all()                          # 50 cells and more: never the exact table
    assert set(reg.ravel().tolist()) == {0, 1, 2, 3, 4}
    assert reg[0, 1] == 2 and reg[1, 2] == 3 and reg[2, 3] == 4 and reg[3, 3] == 4 and (reg[:, 4] == 0).all()
    assert 1 in reg[:, 0].tolist()
    assert reg[4, 3] == 4 and reg[5, 3] == 3         # |z| = 37.539 and 37.4998 around the 37.5193 cut


def check_welch_ladder(pts):
    """Rung r of welch_ladder() -- gene r, comparison r -- sits where its name says; both continued fractions are taken."""
    t, df, p = (pts[range(len(WELCH_RUNGS)), range(len(WELCH_RUNGS)), i] for i in range(3))
    assert t[0] == 0.0 and p[0] == 1.0
    assert 19.5 < df[1] < 20.0 < df[2] < 20.5
    assert df[3] == 1.0
    assert 1e-300 < p[4] < 1e-10
    assert p[5] == 0.0 and math.isfinite(t[5])
    sides = [pt_side(a, b) for a, b in zip(t, df)]
    assert sides[0] == sides[1] == sides[2] == "upper" and sides[3] == sides[4] == sides[5] == "lower"
    return sides


_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _mulhilo(a, b):
    """(high, low) 64-bit halves of the 128-bit product of the uint64 constant a and the uint64 array b."""
    a = np.uint64(a)
    a0, a1 = a & _M32, a >> _S32
    b0, b1 = b & _M32, b >> _S32
    ll, lh, hl, hh = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (ll >> _S32) + (lh & _M32) + (hl & _M32)
    return hh + (lh >> _S32) + (hl >> _S32) + (mid >> _S32), a * b


def _horner(c, r):
    p = np.full_like(r, c[-1])
    for v in c[-2::-1]:
        p = p * r + v
    return p


def jitter_matrix(seed, G, C):
    """dr.jitter(seed, g, c) for every (gene, cell) at once: the first Philox4x64-10 block of counter [0, g, c, 0] + 1 in
    NumPy integers, then dr.qnorm_lib operation by operation on arrays.  The tests that use it compare a sample with
    dr.jitter itself, bit for bit."""
    import oracle_np
    with np.errstate(over="ignore"):
        x0 = np.ones((G, C), dtype=np.uint64)
        x1 = np.broadcast_to(np.arange(G, dtype=np.uint64)[:, None], (G, C)).copy()
        x2 = np.broadcast_to(np.arange(C, dtype=np.uint64)[None, :], (G, C)).copy()
        x3 = np.zeros((G, C), dtype=np.uint64)
        k0, k1 = np.uint64(seed), np.uint64(dr.JITTER_TOKEN)
        for rnd in range(10):
            if rnd:
                k0 = k0 + np.uint64(0x9E3779B97F4A7C15)
                k1 = k1 + np.uint64(0xBB67AE8584CAA73B)
            hi0, lo0 = _mulhilo(0xD2E7470EE14C6C93, x0)
            hi1, lo1 = _mulhilo(0xCA5A826395121157, x2)
            x0, x1, x2, x3 = hi1 ^ x1 ^ k0, lo1, hi0 ^ x3 ^ k1, lo0
    u1 = (x0 >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    u2 = (x1 >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    p = (np.floor(134217728.0 * u1) + u2) / 134217728.0
    q = p - 0.5
    r = 0.180625 - q * q
    z = q * _horner(dr._A, r) / _horner(dr._B, r)
    tail = ~(np.abs(q) <= 0.425)
    if tail.any():
        pt, qt = p[tail], q[tail]
        r = np.sqrt(-oracle_np.icnv_log(np.where(qt < 0, pt, 1.0 - pt)))
        mid = r <= 5.0
        val = np.where(mid, _horner(dr._C, r - 1.6) / _horner(dr._D, r - 1.6), _horner(dr._E, r - 5.0) / _horner(dr._F, r - 5.0))
        z[tail] = np.where(qt < 0, -val, val)
    return 1e-4 + 1e-4 * z


def jitter_sample_matches(J, seed, n=300):
    """J = jitter_matrix(seed, ...) against dr.jitter at n scattered positions and at the n smallest and largest entries
    (the tails of qnorm)."""
    G, C = J.shape
    rng = np.random.default_rng(seed + 1)
    flat = np.concatenate([rng.integers(0, G * C, size=n), np.argsort(J, axis=None)[:n], np.argsort(J, axis=None)[-n:]])
    return all(J[i // C, i % C] == dr.jitter(seed, int(i // C), int(i % C)) for i in flat)


def exact_mean_fast(expr):
    """dr.exact_mean for large matrices: the values' integer significands summed per binary exponent (in two 27-bit halves,
    so the int64 sums of up to 2^35 values cannot overflow), the total as one Fraction, one rounding at the end."""
    v = np.asarray(expr, dtype=np.float64).ravel()
    if not np.isfinite(v).all():
        raise ValueError("finite values only")
    m, e = np.frexp(v)
    M = np.ldexp(m, 53).astype(np.int64)            # exact: |m| < 1 has 53 significant bits
    hi, lo = M >> 27, M & ((1 << 27) - 1)           # M = hi 2^27 + lo, also for negative M
    total = Fraction(0)
    for ex in np.unique(e):
        sel = e == ex
        s = (int(hi[sel].sum()) << 27) + int(lo[sel].sum())
        total += Fraction(s) * Fraction(2) ** (int(ex) - 53)
    return float(total / v.size)
