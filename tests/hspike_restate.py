"""Sequential restatement of the K15 contract (include/icnv.h "hidden spike-in", infercnv_amd/smooth_spline.py, DESIGN K15),
written from R/inferCNV_hidden_spike.R, R/inferCNV_meanVarSim.R, R/inferCNV_simple_sim.R and the contract, not from the
library's code.  The GPU is held to the tables and to the simulation bit for bit; the host smoother to the dense smoother
here within a measured tolerance.

  - tables: plain loops, math.fsum: m = the exactly summed values / n rounded once, v = fsum(round(round(x - m)^2)) / (n - 1).
  - smoother: dense -- scipy.interpolate.BSpline.design_matrix, a Gauss-Legendre penalty matrix, numpy.linalg.solve (and,
    to measure the conditioning of the problem, Cholesky against the QR of the augmented least-squares system).
  - simulation: element by element with numpy.random.Philox and the exp_lib / log_lib / qnorm_lib of tests/de_restate.py
    (simulate_elementwise); `simulate` is the same arithmetic on whole arrays with a NumPy restatement of Philox4x64-10, held
    to simulate_elementwise bit for bit in tests/test_hspike_host.py, for the shapes a Python loop cannot visit in time.
"""
import bisect
import math
from fractions import Fraction

import numpy as np
from scipy.interpolate import BSpline
from scipy.linalg import cho_factor, cho_solve, qr, solve_triangular

import oracle_np
from de_restate import exp_lib, log_lib, qnorm_lib, _A, _B, _C, _D, _E, _F

GENES_TOKEN = 0x6873706B67656E65   # "hspkgene"
CHR_INFO = (("chrA", 1), ("chr_0", 0.01), ("chr_B", 1), ("chr_0pt5", 0.5), ("chr_C", 1), ("chr_1pt5", 1.5),
            ("chr_D", 1), ("chr_2pt0", 2.0), ("chr_E", 1), ("chr_3pt0", 3), ("chr_F", 1))


# ---------------------------------------------------------------- tables
def exact_mean(vals):
    """sum(vals) / n rounded once: the exact sum as a list of doubles (each fsum is the correctly rounded remainder)."""
    parts = []
    while True:
        s = math.fsum(vals + [-p for p in parts])
        if s == 0.0:
            break
        parts.append(s)
    if not parts:
        return 0.0
    return float(sum((Fraction(p) for p in parts), Fraction(0)) / len(vals))


def group_gene_tables(expr, groups):
    """expr: genes x cells.  (m, v, nzero), each (n_groups, G)."""
    expr = np.asarray(expr, dtype=np.float64)
    G = expr.shape[0]
    m = np.empty((len(groups), G))
    v = np.empty((len(groups), G))
    nz = np.empty((len(groups), G), dtype=np.int32)
    for q, cells in enumerate(groups):
        cells = np.asarray(cells, dtype=np.int64)
        n = cells.size
        for g in range(G):
            row = expr[g, cells]
            vals = row.tolist()
            mean = exact_mean(vals)
            m[q, g] = mean
            d = row - mean                       # one rounding per element, then one per square
            ss = math.fsum((d * d).tolist())
            v[q, g] = ss / (n - 1.0) if n > 1 else math.nan
            nz[q, g] = sum(1 for a in vals if a == 0)
    return m, v, nz


# ---------------------------------------------------------------- smoother
def nknots(n):
    if n < 50:
        return n
    a1, a2, a3, a4 = math.log2(50), math.log2(100), math.log2(140), math.log2(200)
    if n < 200:
        v = 2 ** (a1 + (a2 - a1) * (n - 50) / 150)
    elif n < 800:
        v = 2 ** (a2 + (a3 - a2) * (n - 200) / 600)
    elif n < 3200:
        v = 2 ** (a3 + (a4 - a3) * (n - 800) / 2400)
    else:
        v = 200 + (n - 3200) ** 0.2
    return math.floor(v + 1e-9)                # the anchors 50, 200, 800, 3200 give 50, 100, 140, 200 on every platform


def type7_quantile(sorted_x, p):
    h = (len(sorted_x) - 1) * p
    lo = int(math.floor(h))
    hi = min(lo + 1, len(sorted_x) - 1)
    return sorted_x[lo] + (h - lo) * (sorted_x[hi] - sorted_x[lo])


class Dense:
    """The merged, scaled problem of one (x, y) input and its dense matrices."""

    def __init__(self, x, y, all_knots=False):
        x = [float(a) for a in x]
        y = [float(a) for a in y]
        if not all(math.isfinite(a) for a in x + y):
            raise ValueError("non-finite input")
        sx = sorted(x)
        tol = 1e-6 * (type7_quantile(sx, 0.75) - type7_quantile(sx, 0.25))
        if not tol > 0:
            raise ValueError("tol")
        mean = float(np.mean(np.asarray(x)))
        classes = {}
        for a, b in zip(x, y):
            k = round((a - mean) / tol)            # Python rounds half to even, as R >= 4
            if k not in classes:
                classes[k] = [a, []]
            classes[k][1].append(b)
        keys = sorted(classes)
        if len(keys) < 4:
            raise ValueError("fewer than 4 unique x")
        self.xbar = np.array([classes[k][0] for k in keys])
        self.wbar = np.array([float(len(classes[k][1])) for k in keys])
        self.ybar = np.array([sum(classes[k][1], 0.0) / len(classes[k][1]) for k in keys])     # summed in input order
        self.yssw = float(sum(sum((b - yb) ** 2 for b in classes[k][1]) for k, yb in zip(keys, self.ybar)))
        nx = self.nx = len(keys)
        self.xmin, self.range = float(self.xbar[0]), float(self.xbar[-1] - self.xbar[0])
        self.t = (self.xbar - self.xbar[0]) / self.range
        nkn = nx if all_knots else nknots(nx)
        by = (nx - 1) / (nkn - 1)
        idx = [int(math.floor(1.0 + i * by)) for i in range(nkn - 1)] + [nx]
        interior = self.t[np.array(idx) - 1]
        self.knots = np.concatenate([[interior[0]] * 3, interior, [interior[-1]] * 3])
        self.nk = nkn + 2
        self.w = self.wbar * nx / self.wbar.sum()
        self.X = BSpline.design_matrix(self.t, self.knots, 3).toarray()
        self.Omega, self.R = self._penalty()
        XW = self.X * self.w[:, None]
        self.XtWX = self.X.T @ XW
        self.XtWy = XW.T @ self.ybar
        sl = slice(2, self.nk - 3)
        self.ratio = float(np.trace(self.XtWX[sl, sl]) / np.trace(self.Omega[sl, sl]))

    def _penalty(self):
        """Omega by 3-point Gauss-Legendre per knot interval (exact: the integrand is piecewise quadratic), and its factor R
        with R'R = Omega (one row per quadrature node)."""
        nodes, weights = np.polynomial.legendre.leggauss(3)
        br = np.unique(self.knots)
        rows = []
        eye = np.eye(self.nk)
        d2 = BSpline(self.knots, eye, 3).derivative(2)
        for a, b in zip(br[:-1], br[1:]):
            pts = 0.5 * (b - a) * nodes + 0.5 * (a + b)
            rows.append(d2(pts) * np.sqrt(0.5 * (b - a) * weights)[:, None])
        R = np.vstack(rows)
        return R.T @ R, R

    def lam(self, spar):
        return self.ratio * 256.0 ** (3.0 * spar - 1.0)

    def solve(self, lam):
        return np.linalg.solve(self.XtWX + lam * self.Omega, self.XtWy)

    def solve_cholesky(self, lam):
        return cho_solve(cho_factor(self.XtWX + lam * self.Omega), self.XtWy)

    def solve_qr(self, lam):
        """min || [sqrt(W) X; sqrt(lam) R] c - [sqrt(W) ybar; 0] ||: the same minimiser without forming the normal equations."""
        sw = np.sqrt(self.w)
        A = np.vstack([self.X * sw[:, None], math.sqrt(lam) * self.R])
        b = np.concatenate([sw * self.ybar, np.zeros(self.R.shape[0])])
        Q, Rm = qr(A, mode="economic")
        return solve_triangular(Rm, Q.T @ b)

    def gcv(self, lam):
        A = self.XtWX + lam * self.Omega
        sol = np.linalg.solve(A, np.column_stack([self.XtWy, self.XtWX]))
        df = float(np.trace(sol[:, 1:]))
        res = self.ybar - self.X @ sol[:, 0]
        rss = float(np.sum(self.w * res * res)) + self.yssw
        sumw = float(self.w.sum())
        return (rss / sumw) / (1.0 - df / sumw) ** 2

    def fitted(self, coef):
        return self.X @ coef


def spline_eval(knots, coef, xmin, rng, x):
    """S(x) of the contract, one Python float operation at a time."""
    k = knots if isinstance(knots, list) else [float(a) for a in knots]
    c = coef if isinstance(coef, list) else [float(a) for a in coef]
    nk = len(c)
    t = (float(x) - xmin) / rng
    if t < 0.0:
        return c[0] + ((3.0 * (c[1] - c[0])) / (k[4] - k[3])) * t
    if t > 1.0:
        return c[nk - 1] + ((3.0 * (c[nk - 1] - c[nk - 2])) / (k[nk] - k[nk - 1])) * (t - 1.0)
    i = bisect.bisect_right(k, t, 4, nk) - 1   # the largest i in 3 .. nk - 1 with k[i] <= t
    d = [c[i - 3 + j] for j in range(4)]
    for r in range(1, 4):
        for j in range(3, r - 1, -1):
            kl = k[i - 3 + j]
            a = (t - kl) / (k[i + 1 + j - r] - kl)
            d[j] = (1.0 - a) * d[j - 1] + a * d[j]
    return d[3]


# ---------------------------------------------------------------- simulation
def _draws(seed, token, first, g, c, n):
    bg = np.random.Philox(key=np.array([seed, token], dtype=np.uint64), counter=np.array([first, g, c, 0], dtype=np.uint64))
    return [float(u) for u in np.random.Generator(bg).random(n)]


def simulate_elementwise(means, num_cells, var_spline, p0_spline, seed, token):
    """One matrix, genes x num_cells.  var_spline / p0_spline: (knots, coef, xmin, range)."""
    means = [float(a) for a in means]
    n = int(num_cells)
    out = np.zeros((len(means), n))
    for g, m in enumerate(means):
        if not m > 0.0:
            continue
        logm = log_lib(m + 1.0)
        var = exp_lib(spline_eval(*var_spline, logm)) - 1.0
        var = var if var > 0.0 else 0.0
        sd = math.sqrt(var)
        total, nz = 0.0, 0
        for c in range(n):
            u1, u2 = _draws(seed, token, 0, g, c, 2)
            z = qnorm_lib((math.floor(134217728.0 * u1) + u2) / 134217728.0)
            w = m + sd * z
            w = w if w > 0.0 else 0.0
            val = float(round(w))               # half to even
            out[g, c] = val
            total += val
            nz += val == 0.0
        if nz == n:
            continue
        p = spline_eval(*p0_spline, log_lib(total / float(n)))
        padj = (p * float(n) - float(nz)) / (float(n) - float(nz))
        if not padj > 0.0:
            continue
        for c in range(n):
            if _draws(seed, token, 1, g, c, 1)[0] <= padj:
                out[g, c] = 0.0
    return out


_M32 = np.uint64(0xFFFFFFFF)


def _mulhilo(a, b):
    """(high, low) 64-bit halves of the constant a times the uint64 array b."""
    a_lo, a_hi = np.uint64(a & 0xFFFFFFFF), np.uint64(a >> 32)
    b_lo, b_hi = b & _M32, b >> np.uint64(32)
    p0, p1, p2, p3 = a_lo * b_lo, a_lo * b_hi, a_hi * b_lo, a_hi * b_hi
    mid = (p0 >> np.uint64(32)) + (p1 & _M32) + (p2 & _M32)
    hi = p3 + (p1 >> np.uint64(32)) + (p2 >> np.uint64(32)) + (mid >> np.uint64(32))
    return hi, np.uint64(a) * b


def philox_block(seed, token, first, g, c):
    """The first block NumPy's Philox(key = [seed, token], counter = [first, g, c, 0]) hands out: four uint64 arrays
    (Philox4x64-10 of the counter plus one, as NumPy increments before it generates)."""
    with np.errstate(over="ignore"):
        g, c = np.broadcast_arrays(np.asarray(g, dtype=np.uint64), np.asarray(c, dtype=np.uint64))
        x0 = np.full(g.shape, first + 1, dtype=np.uint64)
        x1, x2, x3 = g.copy(), c.copy(), np.zeros(g.shape, dtype=np.uint64)
        k0, k1 = int(seed) & (2**64 - 1), int(token) & (2**64 - 1)
        for rnd in range(10):
            if rnd:
                k0 = (k0 + 0x9E3779B97F4A7C15) & (2**64 - 1)
                k1 = (k1 + 0xBB67AE8584CAA73B) & (2**64 - 1)
            hi0, lo0 = _mulhilo(0xD2E7470EE14C6C93, x0)
            hi1, lo1 = _mulhilo(0xCA5A826395121157, x2)
            x0, x1, x2, x3 = hi1 ^ x1 ^ np.uint64(k0), lo1, hi0 ^ x3 ^ np.uint64(k1), lo0
    return x0, x1, x2, x3


def _u(word):
    return (word >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def _horner(c, r):
    p = np.full(r.shape, c[-1])
    for v in c[-2::-1]:
        p = p * r + v
    return p


def qnorm_vec(p):
    q = p - 0.5
    out = np.empty(p.shape)
    cen = np.abs(q) <= 0.425
    r = 0.180625 - q[cen] * q[cen]
    out[cen] = q[cen] * _horner(_A, r) / _horner(_B, r)
    tail = ~cen
    pt, qt = p[tail], q[tail]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.sqrt(-oracle_np.icnv_log(np.where(qt < 0, pt, 1.0 - pt)))
        near = r <= 5.0
        val = np.where(near, _horner(_C, r - 1.6) / _horner(_D, r - 1.6), _horner(_E, r - 5.0) / _horner(_F, r - 5.0))
    out[tail] = np.where(qt < 0, -val, val)
    return out


def simulate(means, num_cells, var_spline, p0_spline, seed, token):
    """simulate_elementwise on whole arrays (module docstring); the per-gene spline values stay scalar restatements."""
    means = np.asarray(means, dtype=np.float64)
    var_spline, p0_spline = (([float(a) for a in s[0]], [float(a) for a in s[1]], float(s[2]), float(s[3])) for s in (var_spline, p0_spline))
    G, n = means.size, int(num_cells)
    out = np.zeros((G, n))
    pos = np.nonzero(means > 0.0)[0]
    if pos.size == 0:
        return out
    sd = np.empty(pos.size)
    logm = oracle_np.icnv_log(means[pos] + 1.0)          # log_lib on the whole vector
    for k in range(pos.size):
        var = exp_lib(spline_eval(*var_spline, float(logm[k]))) - 1.0
        sd[k] = math.sqrt(var if var > 0.0 else 0.0)
    gg, cc = pos[:, None], np.arange(n)[None, :]
    w0, w1, _, _ = philox_block(seed, token, 0, gg, cc)
    z = qnorm_vec((np.floor(134217728.0 * _u(w0)) + _u(w1)) / 134217728.0)
    w = means[pos][:, None] + sd[:, None] * z
    val = np.rint(np.where(w > 0.0, w, 0.0))
    total = np.zeros(pos.size)
    for c in range(n):                           # the sequential double sum over c
        total = total + val[:, c]
    nz = (val == 0.0).sum(axis=1)
    u = _u(philox_block(seed, token, 1, gg, cc)[0])
    with np.errstate(divide="ignore"):
        logmean = oracle_np.icnv_log(total / float(n))
    for k in range(pos.size):
        if nz[k] == n:
            continue
        p = spline_eval(*p0_spline, float(logmean[k]))
        padj = (p * float(n) - float(nz[k])) / (float(n) - float(nz[k]))
        if padj > 0.0:
            val[k, u[k] <= padj] = 0.0
    out[pos] = val
    return out


# ---------------------------------------------------------------- the build
def fnv1a64(name):
    h = 0xCBF29CE484222325
    for b in str(name).encode("utf-8"):
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def chr_info(num_genes_each, num_total):
    rem = num_total - 10 * num_genes_each
    if rem < num_genes_each:
        rem = num_genes_each
    return [(name, cnv, rem if k == len(CHR_INFO) - 1 else num_genes_each) for k, (name, cnv) in enumerate(CHR_INFO)]


def genes_use_idx(G, num_genes, seed):
    return np.array([int(math.floor(float(G) * _draws(seed, GENES_TOKEN, 2, j, 0, 1)[0])) for j in range(num_genes)], dtype=np.int64)


def table_groups(ref_groups, obs_groups):
    """Ordered dicts name -> cells.  c(observation, reference); reference-less: the one group of all observation cells."""
    if not ref_groups:
        return [np.concatenate([np.asarray(v) for v in obs_groups.values()])]
    return [np.asarray(v) for v in obs_groups.values()] + [np.asarray(v) for v in ref_groups.values()]


def normal_groups(ref_groups, obs_groups, aggregate_normals=False):
    if not ref_groups:
        return {"normalsToUse": np.concatenate([np.asarray(v) for v in obs_groups.values()])}
    if aggregate_normals:
        return {"normalsToUse": np.concatenate([np.asarray(v) for v in ref_groups.values()])}
    return {k: np.asarray(v) for k, v in ref_groups.items()}


def build_hspike(expr, ref_groups, obs_groups, var_spline, p0_spline, seed=0, aggregate_normals=False, simulate_fn=simulate,
                 num_cells=100, num_genes_each=400):
    """.build_and_add_hspike from the normalised genes x cells matrix and GIVEN splines (knots, coef, xmin, range): returns
    (counts genes x cells, normalised matrix, chr names per gene, reference groups, observation groups, cell names)."""
    expr = np.asarray(expr, dtype=np.float64)
    G = expr.shape[0]
    info = chr_info(num_genes_each, G)
    chrs = [name for name, _, n in info for _ in range(n)]
    cnv = np.array([float(c) for _, c, n in info for _ in range(n)])
    num_genes = len(chrs)
    use = genes_use_idx(G, num_genes, seed)
    normals = normal_groups(ref_groups, obs_groups, aggregate_normals)
    blocks, refs, obs, names = [], {}, {}, []
    counter = 0
    cells = None
    for normal_type, cells in normals.items():
        orig = np.array([exact_mean(expr[g, cells].tolist()) for g in range(G)])
        gm = orig[use]
        gm[gm == 0] = 1e-3
        spiked = gm.copy()
        spiked[cnv != 1] = spiked[cnv != 1] * cnv[cnv != 1]
        for prefix, mu, dest in (("simnorm_cell_", gm, refs), ("spike_tumor_cell_", spiked, obs)):
            name = prefix + normal_type
            blocks.append(simulate_fn(mu, num_cells, var_spline, p0_spline, seed, fnv1a64(name)))
            names += [f"{name}{i}" for i in range(1, num_cells + 1)]
            dest[name] = np.arange(counter, counter + num_cells)
            counter += num_cells
    counts = np.hstack(blocks)
    last_sums = np.array([math.fsum(expr[:, c].tolist()) for c in cells])      # colSums of the LAST normal type's cells
    target = float(np.median(last_sums))
    cs = np.array([math.fsum(counts[:, c].tolist()) for c in range(counts.shape[1])])
    with np.errstate(invalid="ignore", divide="ignore"):
        norm = counts / cs[None, :] * target
    return counts, norm, chrs, refs, obs, names


# ---------------------------------------------------------------- inputs of the end-to-end tests
def synthetic_counts(seed=20):
    """Seeded integer counts with dropout, 6 000 genes x 1 200 cells: two reference groups of 200 cells, one observation
    group of 800; in the observation cells genes 900 .. 1 499 are duplicated (x 1.5) and genes 3 300 .. 3 899 deleted
    (x 0.5).  Returns (counts genes x cells, chr per gene, reference groups, observation groups, duplicated gene numbers,
    deleted gene numbers)."""
    rng = np.random.default_rng(seed)
    G, C = 6000, 1200
    chrs = np.array([f"chr{1 + g // 300}" for g in range(G)])
    refs = {"normA": np.arange(0, 200), "normB": np.arange(200, 400)}
    obs = {"tumor": np.arange(400, C)}
    mu = np.exp(rng.normal(math.log(4.0), 1.0, size=G))
    lib = np.exp(rng.normal(0.0, 0.2, size=C))
    dup, dele = np.arange(900, 1500), np.arange(3300, 3900)
    factor = np.ones((G, C))
    factor[np.ix_(dup, obs["tumor"])] = 1.5
    factor[np.ix_(dele, obs["tumor"])] = 0.5
    lam = mu[:, None] * lib[None, :] * factor * rng.gamma(8.0, 1.0 / 8.0, size=(G, C))
    counts = rng.poisson(lam).astype(np.float64)
    p_drop = 1.0 / (1.0 + np.exp(1.5 * (np.log(mu) - math.log(0.8))))
    counts[rng.random((G, C)) < p_drop[:, None]] = 0.0
    return np.asfortranarray(counts), chrs, refs, obs, dup, dele
