"""Sequential restatement of the K12 contract of include/icnv.h (icnv_de_tests_dev / icnv_mask_non_de_dev, DESIGN K12): per
(comparison, gene), in the documented operation order, in Python floats (one IEEE rounding per operation).  The GPU is
held to it bit for bit; SciPy and mpmath hold it to the published tests.

  - jitter of (gene g, cell c): Generator(Philox(key=[seed, JITTER_TOKEN], counter=[0, g, c, 0])), u1, u2 = two random(),
    z = qnorm((floor(2^27 u1) + u2) / 2^27) by AS 241 with the library's table log, jitter = 1e-4 + 1e-4 z.
  - wilcoxon: midranks, 2W and T = sum(t^3 - t) exact; exact branch from integer counts, correctly rounded; else R's normal
    approximation with continuity correction and pnorm_both's non-log branches (exp = exp_lib).
  - t: Welch with correctly rounded moments and 2 pt(-|t|, df) by the incomplete-beta continued fraction.
  - BH: p.adjust(, "BH") with n = the non-NA count."""
import math
from fractions import Fraction
from functools import lru_cache

import numpy as np

import oracle_np

JITTER_TOKEN = 0x6E6F6E44456A6974
EXACT_MAX = 49
CF_MAX_ITER = 20000
EXP_MAX, EXP_MIN = 709.0, -708.0
INV_LN2, LN2_HI, LN2_LO = 1.4426950408889634, 6.93147180369123816490e-01, 1.90821492927058770002e-10
EXP_COEF = [1.0 / math.factorial(j) for j in range(12)]


def log_lib(x):
    return float(oracle_np.icnv_log(np.float64(x)))


def exp_lib(x):
    """K11's exp_lib, extended: x > 709 or NaN -> +inf, x < -708 -> 0."""
    x = float(x)
    if not (x <= EXP_MAX):
        return math.inf
    if x < EXP_MIN:
        return 0.0
    k = math.floor(x * INV_LN2 + 0.5)
    kd = float(k)
    t = (x - kd * LN2_HI) - kd * LN2_LO
    p = EXP_COEF[11]
    for j in range(10, -1, -1):
        p = p * t + EXP_COEF[j]
    return math.ldexp(p, k)


_A = (3.3871328727963666080e0, 1.3314166789178437745e+2, 1.9715909503065514427e+3, 1.3731693765509461125e+4,
      4.5921953931549871457e+4, 6.7265770927008700853e+4, 3.3430575583588128105e+4, 2.5090809287301226727e+3)
_B = (1.0, 4.2313330701600911252e+1, 6.8718700749205790830e+2, 5.3941960214247511077e+3, 2.1213794301586595867e+4,
      3.9307895800092710610e+4, 2.8729085735721942674e+4, 5.2264952788528545610e+3)
_C = (1.42343711074968357734e0, 4.63033784615654529590e0, 5.76949722146069140550e0, 3.64784832476320460504e0,
      1.27045825245236838258e0, 2.41780725177450611770e-1, 2.27238449892691845833e-2, 7.74545014278341407640e-4)
_D = (1.0, 2.05319162663775882187e0, 1.67638483018380384940e0, 6.89767334985100004550e-1, 1.48103976427480074590e-1,
      1.51986665636164571966e-2, 5.47593808499534494600e-4, 1.05075007164441684324e-9)
_E = (6.65790464350110377720e0, 5.46378491116411436990e0, 1.78482653991729133580e0, 2.96560571828504891230e-1,
      2.65321895265761230930e-2, 1.24266094738807843860e-3, 2.71155556874348757815e-5, 2.01033439929228813265e-7)
_F = (1.0, 5.99832206555887937690e-1, 1.36929880922735805310e-1, 1.48753612908506148525e-2, 7.86869131145613259100e-4,
      1.84631831751005468180e-5, 1.42151175831644588870e-7, 2.04426310338993978564e-15)


def _horner(c, r):
    p = c[-1]
    for v in c[-2::-1]:
        p = p * r + v
    return p


def qnorm_lib(p):
    q = p - 0.5
    if abs(q) <= 0.425:
        r = 0.180625 - q * q
        return q * _horner(_A, r) / _horner(_B, r)
    r = math.sqrt(-log_lib(p if q < 0 else 1.0 - p))
    if r <= 5.0:
        r = r - 1.6
        val = _horner(_C, r) / _horner(_D, r)
    else:
        r = r - 5.0
        val = _horner(_E, r) / _horner(_F, r)
    return -val if q < 0 else val


def jitter(seed, g, c):
    bg = np.random.Philox(key=np.array([seed, JITTER_TOKEN], dtype=np.uint64), counter=np.array([0, g, c, 0], dtype=np.uint64))
    u = np.random.Generator(bg).random(2)
    z = qnorm_lib((math.floor(134217728.0 * float(u[0])) + float(u[1])) / 134217728.0)
    return 1e-4 + 1e-4 * z


def pnorm2(z):
    """2 min(pnorm(z), pnorm(z, lower.tail=FALSE)) by pnorm_both's non-log branches, exp = exp_lib."""
    if z != z:
        return z
    y = abs(z)
    if y <= 0.67448975:
        q = y * y
        num, den = 0.065682337918207449113 * q, q
        for a, b in ((2.2352520354606839287, 47.20258190468824187), (161.02823106855587881, 976.09855173777669322),
                     (1067.6894854603709582, 10260.932208618978205)):
            num = (num + a) * q
            den = (den + b) * q
        t = y * (num + 18154.981253343561249) / (den + 45507.789335026729956)
        return 2.0 * (0.5 - t)
    if not (y < 37.5193):
        return 0.0
    if y <= 5.656854249492380195206754896838:
        num, den = 1.0765576773720192317e-8 * y, y
        for a, b in ((0.39894151208813466764, 22.266688044328115691), (8.8831497943883759412, 235.38790178262499861),
                     (93.506656132177855979, 1519.377599407554805), (597.27027639480026226, 6485.558298266760755),
                     (2494.5375852903726711, 18615.571640885098091), (6848.1904505362823326, 34900.952721145977266),
                     (11602.651437647350124, 38912.003286093271411)):
            num = (num + a) * y
            den = (den + b) * y
        t = (num + 9842.7148383839780218) / (den + 19685.429676859990727)
    else:
        q = 1.0 / (y * y)
        num, den = 0.02307344176494017303 * q, q
        for a, b in ((0.21589853405795699, 1.28426009614491121), (0.1274011611602473639, 0.468238212480865118),
                     (0.022235277870649807, 0.0659881378689285515), (0.001421619193227893466, 0.00378239633202758244)):
            num = (num + a) * q
            den = (den + b) * q
        t = q * (num + 2.9112874951168792e-5) / (den + 7.29751555083966205e-5)
        t = (0.398942280401432677939946059934 - t) / y
    xs = math.trunc(y * 16.0) / 16.0
    dl = (y - xs) * (y + xs)
    small = exp_lib(-xs * xs * 0.5) * exp_lib(-dl * 0.5) * t
    return 2.0 * min(small, 1.0 - small)


def log1p_lib(y):
    if not (y <= 0.5):
        return log_lib(1.0 + y)
    s = y / (2.0 + y)
    s2 = s * s
    h = 1.0 / 29.0
    for k in range(13, 0, -1):
        h = h * s2 + 1.0 / float(2 * k + 1)
    h = h * s2 + 1.0
    return (2.0 * s) * h


_CORR = (1.0 / 12.0, -1.0 / 360.0, 1.0 / 1260.0, -1.0 / 1680.0, 1.0 / 1188.0, -691.0 / 360360.0, 1.0 / 156.0, -3617.0 / 122400.0)


def stirling_corr(a):
    x = 1.0 / a
    x2 = x * x
    h = _CORR[7]
    for j in range(6, -1, -1):
        h = h * x2 + _CORR[j]
    return h * x


def lgamma_diff_half(a):
    """lgamma(a) - lgamma(a + 1/2)."""
    r = 1.0
    while a < 10.0:
        r = r * ((a + 0.5) / a)
        a = a + 1.0
    d = (((-0.5 * log_lib(a)) - (a * log1p_lib(0.5 / a))) + 0.5) + (stirling_corr(a) - stirling_corr(a + 0.5))
    return d if r == 1.0 else d + log_lib(r)


def betacf(a, b, x):
    FPMIN = 1e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c, d = 1.0, 1.0 - (qab * x) / qap
    if abs(d) < FPMIN:
        d = FPMIN
    d = 1.0 / d
    h = d
    for m in range(1, CF_MAX_ITER + 1):
        md = float(m)
        m2 = 2.0 * md
        aa = ((md * (b - md)) * x) / ((qam + m2) * (a + m2))
        d = 1.0 + aa * d
        if abs(d) < FPMIN:
            d = FPMIN
        c = 1.0 + aa / c
        if abs(c) < FPMIN:
            c = FPMIN
        d = 1.0 / d
        h = h * (d * c)
        aa = (((-(a + md)) * (qab + md)) * x) / ((a + m2) * (qap + m2))
        d = 1.0 + aa * d
        if abs(d) < FPMIN:
            d = FPMIN
        c = 1.0 + aa / c
        if abs(c) < FPMIN:
            c = FPMIN
        d = 1.0 / d
        dl = d * c
        h = h * dl
        if abs(dl - 1.0) <= 4.440892098500626e-16:
            break
    return h


def pt2(t, df):
    """2 pt(-|t|, df) = I_{df/(df+t^2)}(df/2, 1/2)."""
    if t != t or df != df:
        return t + df
    if math.isinf(t):
        return 0.0
    a, b = df * 0.5, 0.5
    t2 = t * t
    x, xc = df / (df + t2), t2 / (df + t2)
    lx, lxc = -log1p_lib(t2 / df), log_lib(xc)
    lfront = ((a * lx) + (b * lxc)) - (0.57236494292470008707 + lgamma_diff_half(a))
    front = exp_lib(lfront)
    if x < (a + 1.0) / (a + b + 2.0):
        return (front * betacf(a, b, x)) / a
    return 1.0 - (front * betacf(b, a, xc)) / b


# ---------------------------------------------------------------- the tests
@lru_cache(maxsize=None)
def wilcox_counts(m, n):
    """Arrangements of m x's and n y's by U = #(x > y): the Gaussian binomial [m + n choose m]_q, exact integers."""
    poly = [1]
    for i in range(1, m + 1):
        a = n + i
        new = poly + [0] * a
        for k in range(len(poly)):
            new[k + a] -= poly[k]
        for k in range(i, len(new)):
            new[k] += new[k - i]
        poly = new[:i * n + 1]
    return tuple(poly)


def exact_p(W2, m, n):
    """min(2 P, 1), P the exact tail on W's side, correctly rounded (W2 = 2W, no ties)."""
    w = W2 // 2
    c = wilcox_counts(m, n)
    total = sum(c)
    tail = (total - sum(c[:w])) if W2 > m * n else sum(c[:w + 1])
    return min(2.0 * (tail / total), 1.0)


def wilcox(xv, yv):
    """(W, p, T) of wilcox.test(x, y) on already jittered values; None for an empty sample."""
    x = sorted(0.0 if v == 0 else v for v in xv if math.isfinite(v))
    y = sorted(0.0 if v == 0 else v for v in yv if math.isfinite(v))
    nx, ny = len(x), len(y)
    if nx == 0 or ny == 0:
        return None
    i = j = r = sx2 = T = 0
    while i < nx or j < ny:
        v = min(x[i] if i < nx else math.inf, y[j] if j < ny else math.inf)
        cx = cy = 0
        while i < nx and x[i] == v:
            cx += 1
            i += 1
        while j < ny and y[j] == v:
            cy += 1
            j += 1
        t = cx + cy
        sx2 += cx * (2 * r + t + 1)
        r += t
        T += t * t * t - t
    w2 = sx2 - nx * (nx + 1)
    W = float(w2) * 0.5
    if nx <= EXACT_MAX and ny <= EXACT_MAX and T == 0:
        return W, exact_p(w2, nx, ny), T
    dx, dy = float(nx), float(ny)
    z0 = W - dx * dy / 2.0
    sigma = math.sqrt((dx * dy / 12.0) * ((dx + dy + 1.0) - float(T) / ((dx + dy) * (dx + dy - 1.0))))
    corr = 0.5 if z0 > 0 else (-0.5 if z0 < 0 else 0.0)
    z = (z0 - corr) / sigma if sigma != 0.0 else math.nan
    return W, pnorm2(z), T


def cr_mean(v):
    """Correctly rounded sum(v) / n."""
    return float(sum((Fraction(a) for a in v), Fraction(0)) / len(v))


def welch(xv, yv):
    """(t, p, df) of t.test(x, y); NaN where R's try() gives NA."""
    x = [a for a in xv if a == a]
    y = [a for a in yv if a == a]
    nan = math.nan
    if len(x) < 2 or len(y) < 2 or any(math.isinf(a) for a in x + y):
        return nan, nan, nan
    nx, ny = float(len(x)), float(len(y))
    mx, my = cr_mean(x), cr_mean(y)
    vx = math.fsum((a - mx) * (a - mx) for a in x) / (nx - 1.0)
    vy = math.fsum((a - my) * (a - my) for a in y) / (ny - 1.0)
    sx, sy = math.sqrt(vx / nx), math.sqrt(vy / ny)
    se = math.sqrt(sx * sx + sy * sy)
    if se < (10.0 * 2.220446049250313e-16) * max(abs(mx), abs(my)):
        return nan, nan, nan
    sx2, sy2, se2 = sx * sx, sy * sy, se * se
    df = (se2 * se2) / ((sx2 * sx2) / (nx - 1.0) + (sy2 * sy2) / (ny - 1.0))
    t = (mx - my) / se
    return t, pt2(-abs(t), df), df


def bh(p):
    """p.adjust(p, "BH") with R's NA rule (n = the non-NA count; NA stays NA)."""
    p = np.asarray(p, dtype=np.float64)
    out = p.copy()
    ok = ~np.isnan(p)
    q = p[ok]
    n = q.size
    if n <= 1:
        return out
    o = np.argsort(-q, kind="stable")
    res = np.empty(n)
    run = math.inf
    for pos, idx in enumerate(o):
        i = n - pos
        run = min(run, (float(n) / float(i)) * float(q[idx]))
        res[idx] = min(1.0, run)
    out[ok] = res
    return out


def de_tests(expr, groups, comparisons, test="wilcoxon", jitter_on=True, seed=0):
    """expr: genes x cells.  Returns (stat, p, padj) (n_cmp, G) as the library computes them."""
    expr = np.asarray(expr, dtype=np.float64)
    G = expr.shape[0]
    cache = {}

    def values(q, g):
        key = (q, g)
        if key not in cache:
            cells = np.asarray(groups[q], dtype=np.int64)
            v = [float(expr[g, c]) for c in cells]
            if test == "wilcoxon" and jitter_on:
                v = [a + jitter(seed, g, int(c)) for a, c in zip(v, cells)]
            cache[key] = v
        return cache[key]

    n = len(comparisons)
    stat = np.full((n, G), np.nan)
    p = np.full((n, G), np.nan)
    for k, (qx, qy) in enumerate(comparisons):
        for g in range(G):
            if test == "wilcoxon":
                r = wilcox(values(qx, g), values(qy, g))
                if r is None:
                    raise ValueError(f"comparison {k}, gene {g}: empty sample")
                stat[k, g], p[k, g] = r[0], r[1]
            else:
                stat[k, g], p[k, g], _ = welch(values(qx, g), values(qy, g))
    padj = np.vstack([bh(p[k]) for k in range(n)]) if n else p
    return stat, p, padj


def exact_mean(expr):
    return cr_mean(np.asarray(expr, dtype=np.float64).ravel().tolist())


def mask(expr, padj, thresh, base, cell_cmps, n_normal, rule, mask_val):
    """.mask_DE_genes: expr genes x cells, padj (n_cmp, G); returns the masked genes x cells matrix."""
    expr = np.asarray(expr, dtype=np.float64)
    G, C = expr.shape
    cnt = np.tile(np.asarray(base, dtype=np.int64), (G, 1))
    de = np.asarray(padj) < thresh if len(padj) else np.zeros((0, G), dtype=bool)
    for c in range(C):
        for k in cell_cmps[c]:
            cnt[:, c] += de[k]
    if rule == "any":
        m = cnt == 0
    elif rule == "most":
        m = cnt < n_normal / 2.0
    elif rule == "all":
        m = cnt != n_normal
    else:
        raise ValueError(f"Error, not recognizing require_DE_all_normals={rule}")
    out = expr.copy()
    out[m] = mask_val
    return out
