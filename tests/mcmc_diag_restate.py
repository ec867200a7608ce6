"""Sequential restatement of the K31 contract of include/icnv.h (icnv_mcmc_diag_dev, DESIGN K31), written from the header
alone: per series in Python floats (one IEEE rounding per operation), the long sums as np.add.accumulate from 0.0 (strictly
sequential, never pairwise).  The GPU and the host program of infercnv_amd/csrc/mcmc_diag_host_check.cpp are held to it bit for
bit; tests/test_mcmc_diag_host.py holds it to independent code.  The contract is the library's own, modelled on coda: believed,
not verified against coda."""
import math

import numpy as np

import oracle_np

CHAIN_FIELDS = ("mean", "var", "spec0", "order", "geweke", "acf1", "acf5", "acf10", "acf50")
POOLED_FIELDS = ("mean", "sd", "q2.5", "q50", "q97.5", "psrf", "ess")
MIN_KEEP, MIN_CHAINS, MAX_CHAINS, MAX_POOLED = 20, 2, 8, 8192
NAN = float("nan")


def log_lib(x):
    return float(oracle_np.icnv_log(np.float64(x)))


def refusal(n_regions, n_chains, n_keep, K):
    """None, or the error class ("ARG" / "UNSUPPORTED") the entry points return before any launch."""
    if n_regions < 1 or not (MIN_CHAINS <= K <= MAX_CHAINS) or not (MIN_CHAINS <= n_chains <= MAX_CHAINS) or n_keep < MIN_KEEP:
        return "ARG"
    if n_chains * n_keep > MAX_POOLED or n_regions * K > 2 ** 31 - 1:
        return "UNSUPPORTED"
    return None


def seq_sum(a):
    """((0 + a[0]) + a[1]) + .."""
    a = np.asarray(a, dtype=np.float64)
    return float(np.add.accumulate(np.concatenate(([0.0], a)))[-1])


def max_order(m):
    """min(m - 1, floor(10 log10 m)) in integers."""
    p = 0
    while 10 ** (p + 1) <= m ** 10:
        p += 1
    return min(p, m - 1)


def windows(n):
    """(lo, m) of the whole series, Geweke's A and Geweke's B."""
    a_end = -((-(n - 1)) // 10)
    b_lo = (n - 1) // 2
    return (0, n), (0, a_end + 1), (b_lo, n - b_lo)


def cross_sum(x, mean, lag):
    d = np.asarray(x, dtype=np.float64) - mean
    m = d.size
    return seq_sum(d[:m - lag] * d[lag:]) if lag < m else 0.0


def ar_fit(c, m):
    """(spec0, order, phi of the chosen order) from the autocovariances c[0 .. P] of a window of m draws."""
    c0 = c[0]
    if not c0 > 0.0:
        v = 0.0 if c0 == 0.0 else NAN
        return v, v, []
    md = float(m)
    v = c0
    phi = []
    vs, phis = [v], [phi]
    for p in range(1, len(c)):
        acc = c[p]
        for j in range(1, p):
            acc = acc - phi[j - 1] * c[p - j]
        k = _div(acc, v)
        phi = [phi[j - 1] - k * phi[p - j - 1] for j in range(1, p)] + [k]
        v = v * (1.0 - k * k)
        vs.append(v)
        phis.append(phi)
    with np.errstate(all="ignore"):            # crit_p = m * log_lib(v_p) + 2 * p, every order in one call of the table log
        crit = md * oracle_np.icnv_log(np.array(vs)) + 2.0 * np.arange(len(vs), dtype=np.float64)
    best = 0
    for p in range(1, len(vs)):
        if crit[p] < crit[best]:
            best = p
    best_v, best_phi = vs[best], phis[best]
    var_pred = _div(best_v * md, md - float(best + 1))
    s = 0.0
    for f in best_phi:
        s = s + f
    d = 1.0 - s
    return _div(var_pred, d * d), float(best), best_phi


def _div(a, b):
    """IEEE division (Python raises on a zero divisor)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _sqrt(a):
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(a)))


def window_fit(x, lo, m):
    """mean, c[0 .. P], spec0, order, phi of the window x[lo : lo + m]."""
    w = np.asarray(x, dtype=np.float64)[lo:lo + m]
    mean = seq_sum(w) / m
    c = [cross_sum(w, mean, l) / m for l in range(max_order(m) + 1)]
    spec0, order, phi = ar_fit(c, m)
    return mean, c, spec0, order, phi


def chain_stats(x):
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    full, wa, wb = windows(n)
    mean, c, spec0, order, _ = window_fit(x, *full)
    mean_a, _, spec_a, _, _ = window_fit(x, *wa)
    mean_b, _, spec_b, _, _ = window_fit(x, *wb)
    var = cross_sum(x, mean, 0) / (n - 1)
    geweke = _div(mean_a - mean_b, _sqrt(_div(spec_a, float(wa[1])) + _div(spec_b, float(wb[1]))))
    acf50 = _div(cross_sum(x, mean, 50) / n, c[0]) if n > 50 else NAN
    return [mean, var, spec0, order, geweke, _div(c[1], c[0]), _div(c[5], c[0]), _div(c[10], c[0]), acf50]


def quantile7(sorted_x, p):
    N = len(sorted_x)
    index = float(N - 1) * p
    lo, hi = math.floor(index), math.ceil(index)
    xl, xh = float(sorted_x[lo]), float(sorted_x[hi])
    if index == lo or xh == xl:
        return xl
    h = index - lo
    return (1.0 - h) * xl + h * xh


def psrf(mean, var, n):
    m = len(mean)
    md, nd, m1, n1 = float(m), float(n), float(m) - 1.0, float(n) - 1.0
    s = 0.0
    for v in var:
        s = s + v
    W = s / md
    if not W > 0.0:
        return NAN
    s = 0.0
    for v in mean:
        s = s + v
    mu = s / md
    s = 0.0
    for v in mean:
        d = v - mu
        s = s + d * d
    B = nd * (s / m1)
    s = 0.0
    for v in var:
        d = v - W
        s = s + d * d
    var_w = (s / m1) / md
    var_b = (2.0 * (B * B)) / m1
    s = 0.0
    for v in mean:
        s = s + v * v
    q = s / md
    s1 = s2 = 0.0
    for mi, vi in zip(mean, var):
        dv = vi - W
        s1 = s1 + dv * (mi * mi - q)
        s2 = s2 + dv * (mi - mu)
    cov_wb = (nd / md) * (s1 / m1 - (2.0 * mu) * (s2 / m1))
    f = 1.0 + 1.0 / md
    V = (n1 * W) / nd + (f * B) / nd
    var_V = (((n1 * n1) * var_w + (f * f) * var_b) + ((2.0 * n1) * f) * cov_wb) / (nd * nd)
    df = _div(2.0 * (V * V), var_V)
    with np.errstate(all="ignore"):
        adj = float(np.float64(df + 3.0) / np.float64(df + 1.0))
    R2 = n1 / nd + (f * (1.0 / nd)) * (B / W)
    return _sqrt(adj * R2)


def ess(var, spec0, n):
    s = 0.0
    for v, sp in zip(var, spec0):
        s = s + (0.0 if sp == 0.0 else _div(float(n) * v, sp))
    return s


def pooled_stats(X, cs):
    """X: (n_chains, n) draws of one (region, state); cs: its chains' nine fields."""
    X = np.asarray(X, dtype=np.float64)
    m, n = X.shape
    flat = X.ravel()
    N = flat.size
    mean = seq_sum(flat) / N
    sd = _sqrt(cross_sum(flat, mean, 0) / (N - 1))
    if np.isnan(flat).any():
        q = [NAN, NAN, NAN]
    else:
        srt = np.sort(flat + 0.0)              # -0.0 + 0.0 is +0.0
        q = [quantile7(srt, p) for p in (0.025, 0.5, 0.975)]
    cs = np.asarray(cs, dtype=np.float64)
    means, variances, specs = [float(v) for v in cs[:, 0]], [float(v) for v in cs[:, 1]], [float(v) for v in cs[:, 2]]
    return [mean, sd] + q + [psrf(means, variances, n), ess(variances, specs, n)]


def diag(samples):
    """samples: (n_regions, n_chains, n_keep, K) -> chain_stats (R, K, n_chains, 9), pooled (R, K, 7)."""
    s = np.asarray(samples, dtype=np.float64)
    R, m, n, K = s.shape
    cs = np.empty((R, K, m, len(CHAIN_FIELDS)))
    po = np.empty((R, K, len(POOLED_FIELDS)))
    for r in range(R):
        for k in range(K):
            X = np.ascontiguousarray(s[r, :, :, k])
            for ch in range(m):
                cs[r, k, ch] = chain_stats(X[ch])
            po[r, k] = pooled_stats(X, cs[r, k])
    return cs, po


TABLE_COLUMNS = ("Mean", "St.Dev", "2.5%", "50%", "97.5%", "Rhat", "ESS", "Geweke", "acf1", "acf5", "acf10", "acf50")


def table(cs, po):
    """The rows of CNV_MCMC_Diagnostics.dat, one per (region, state): the pooled fields, then chain 0's geweke and acf."""
    R, K = po.shape[:2]
    return np.concatenate([po.reshape(R * K, -1), cs[:, :, 0, 4:].reshape(R * K, -1)], axis=1)


# ---- seeded inputs shared by the tests, the corpus of the host program and the benchmark ----------------------------------
def make_series(kind, m, n, seed):
    """(m, n) draws: "ar1" (coefficient 0.1 .. 0.9 by chain), "white", "dirichlet" (one coordinate of a softmax of AR(1) paths:
    in (0, 1) and autocorrelated, as a kept theta is), "constant" (0.25: its sums are exact), "nan", "ties" (a few values,
    -0.0 among them)."""
    rng = np.random.default_rng(seed)
    if kind == "white":
        return rng.normal(0.3, 1.0, size=(m, n))
    if kind == "ar1":
        x = np.zeros((m, n))
        e = rng.normal(size=(m, n))
        rho = np.linspace(0.1, 0.9, m)
        for t in range(1, n):
            x[:, t] = rho * x[:, t - 1] + e[:, t]
        return x + 2.0
    if kind == "dirichlet":
        return make_samples(1, m, n, 3, seed)[0, :, :, 1]
    if kind == "constant":
        return np.full((m, n), 0.25)
    if kind == "nan":
        return np.full((m, n), np.nan)
    if kind == "ties":
        return rng.choice(np.array([-0.0, 0.0, 0.5, 0.5, 1.0, -1.0]), size=(m, n))
    raise ValueError(kind)


def make_samples(R, m, n, K, seed):
    """(R, m, n, K) theta-like samples: per (region, chain) the softmax over K AR(1) paths, rows summing to 1."""
    rng = np.random.default_rng(seed)
    z = np.zeros((R, m, n, K))
    e = rng.normal(size=(R, m, n, K))
    rho = rng.uniform(0.0, 0.9, size=(R, 1, K))
    for t in range(1, n):
        z[:, :, t] = rho * z[:, :, t - 1] + e[:, :, t]
    z = z + rng.normal(size=(R, 1, 1, K))
    w = np.exp(z - z.max(axis=3, keepdims=True))
    return w / w.sum(axis=3, keepdims=True)
