"""The smoothing spline of the hidden spike-in (DESIGN K15): the host-side fit behind `smooth.spline(logv ~ logm)` and
`smooth.spline(log(m), p0)` of R/inferCNV_meanVarSim.R:30 and R/inferCNV_simple_sim.R:218.  Pure NumPy, like the parameter
preparation in hmm.py; the device only evaluates the fitted spline (include/icnv.h "spline evaluation").

The smoother is the library's own contract, modelled on R's `smooth.spline` defaults.  There is no R to run here, so agreement
with R's numbers cannot be checked; tests/hspike_restate.py restates the contract with dense SciPy algebra.

  input      x, y finite (ValueError otherwise: R stops there too), at least 4 points.
  merging    tol = 1e-6 IQR(x) (type-7 quantiles; tol <= 0 is an error); points with equal rint((x - mean(x)) / tol) merge;
             the merged abscissa is the class's FIRST occurrence in the input, its weight wbar the count, ybar the mean of y
             (np.bincount sums in input order, divided by the count); classes sorted by abscissa; fewer than 4 is an error.
             yssw = sum over all points of (y - ybar of its class)^2.
  scaling    t = (xbar - xbar[0]) / (xbar[-1] - xbar[0]).
  knots      nknots = nknots_smspl(nx) (nx with all_knots=True; its truncation is floor(v + 1e-9)); interior knots
             t[idx_i - 1] with the 1-based idx_i = floor(1 + i by), by = (nx - 1) / (nknots - 1) in double arithmetic, i = 0 .. nknots - 2, and idx = nx for
             the last one (R's seq.int leaves the rounding of its last elements to the platform); both end knots three more
             times; nk = nknots + 2 cubic B-spline coefficients.
  objective  sum w_i (ybar_i - f(t_i))^2 + lambda int f''(t)^2 dt, w = wbar nx / sum(wbar).  The penalty Gram matrix is exact:
             f'' is the linear spline with coefficients D2 D1 c (two difference steps of the B-spline derivative rule), and
             the Gram matrix of the hat functions is tridiagonal in closed form, Omega = (D2 D1)' M (D2 D1).
  lambda     r 256^(3 spar - 1), r = tr(X'WX) / tr(Omega), both over the coefficient indices 3 .. nk - 3 (1-based).
  spar       given, or the minimiser of GCV = (RSS / sum w) / (1 - df / sum w)^2 over [-1.5, 1.5] by Brent's golden-section
             search with parabolic steps (Forsythe, Malcolm and Moler's fmin: tol = 1e-4, eps = 2e-8, at most 500 steps);
             RSS = sum w_i (ybar_i - f(t_i))^2 + yssw (yssw is not rescaled, as in R), df = tr of the hat matrix.
  solve      the dense normal equations (X'WX + lambda Omega) c = X'W ybar by numpy.linalg.solve.
  predict    the operation order of include/icnv.h "spline evaluation", element by element: the B-spline by de Boor's
             recurrence inside [xmin, xmin + range], the boundary value plus the boundary derivative times the distance IN t
             outside -- as predict.smooth.spline.fit extends linearly.

The `nls` logistic fit of .get_logistic_params (R/inferCNV_simple_sim.R:203-210) is computed by R but never read on the
meanvar route (only the spline is): it is not built here.
"""
from __future__ import annotations

import math

import numpy as np

SPAR_LOW, SPAR_HIGH, SPAR_TOL, SPAR_EPS, SPAR_MAXIT = -1.5, 1.5, 1e-4, 2e-8, 500


def nknots_smspl(n):
    """.nknots.smspl (R stats): n below 50, log2-linear through 50 -> 50, 200 -> 100, 800 -> 140, 3200 -> 200 (truncated),
    200 + (n - 3200)^0.2 beyond.  Truncation is floor(v + 1e-9): 2^log2(50) lands just below 50 in double arithmetic, and
    the pieces go through their anchors on every platform this way."""
    n = int(n)
    if n < 50:
        return n
    a1, a2, a3, a4 = math.log2(50), math.log2(100), math.log2(140), math.log2(200)
    if n < 200:
        v = 2.0 ** (a1 + (a2 - a1) * (n - 50) / 150)
    elif n < 800:
        v = 2.0 ** (a2 + (a3 - a2) * (n - 200) / 600)
    elif n < 3200:
        v = 2.0 ** (a3 + (a4 - a3) * (n - 800) / 2400)
    else:
        v = 200 + (n - 3200) ** 0.2
    return int(math.floor(v + 1e-9))


def knot_indices(nx, nknots):
    """0-based indices into the sorted unique abscissae of the interior knots (module docstring, "knots")."""
    by = (nx - 1) / (nknots - 1) if nknots > 1 else 0.0
    idx = np.floor(1.0 + np.arange(nknots, dtype=np.float64) * by).astype(np.int64)
    idx[-1] = nx
    return idx - 1


def _intervals(knots, t):
    """The index i in 3 .. nk - 1 with knots[i] <= t < knots[i + 1] (t = 1 in the last interval)."""
    nk = knots.size - 4
    return np.clip(np.searchsorted(knots, t, side="right") - 1, 3, nk - 1)


def basis_values(knots, t):
    """(i, N): the interval of every t in [0, 1] and the values N[:, r] of the four cubic B-splines i - 3 + r that are not
    zero there (Cox - de Boor)."""
    t = np.asarray(t, dtype=np.float64)
    i = _intervals(knots, t)
    N = np.zeros((t.size, 4))
    N[:, 0] = 1.0
    left = np.zeros((t.size, 4))
    right = np.zeros((t.size, 4))
    for j in range(1, 4):
        left[:, j] = t - knots[i + 1 - j]
        right[:, j] = knots[i + j] - t
        saved = np.zeros(t.size)
        for r in range(j):
            temp = N[:, r] / (right[:, r + 1] + left[:, j - r])
            N[:, r] = saved + right[:, r + 1] * temp
            saved = left[:, j - r] * temp
        N[:, j] = saved
    return i, N


def penalty_matrix(knots):
    """Omega[i, j] = int B_i''(t) B_j''(t) dt over [0, 1], exact (module docstring, "objective")."""
    knots = np.asarray(knots, dtype=np.float64)
    nk = knots.size - 4
    D1 = np.zeros((nk - 1, nk))
    for j in range(nk - 1):
        s = 3.0 / (knots[j + 4] - knots[j + 1])
        D1[j, j], D1[j, j + 1] = -s, s
    D2 = np.zeros((nk - 2, nk - 1))
    for j in range(nk - 2):
        s = 2.0 / (knots[j + 4] - knots[j + 2])
        D2[j, j], D2[j, j + 1] = -s, s
    u = knots[2:-2]                       # the knots of the linear spline f'': hat j peaks at u[j + 1]
    h = np.diff(u)
    M = np.zeros((nk - 2, nk - 2))
    for j in range(nk - 2):
        M[j, j] = (h[j] + h[j + 1]) / 3.0
        if j + 1 < nk - 2:
            M[j, j + 1] = M[j + 1, j] = h[j + 1] / 6.0
    D = D2 @ D1
    return D.T @ M @ D


def spline_eval(knots, coef, xmin, rng, x):
    """S(x) in the operation order of include/icnv.h "spline evaluation" (what the device computes, bit for bit)."""
    knots = np.asarray(knots, dtype=np.float64)
    c = np.asarray(coef, dtype=np.float64)
    nk = c.size
    x = np.asarray(x, dtype=np.float64)
    t = ((x - xmin) / rng).ravel()
    out = np.empty(t.size)
    lo_side, hi_side = t < 0.0, t > 1.0
    out[lo_side] = c[0] + ((3.0 * (c[1] - c[0])) / (knots[4] - knots[3])) * t[lo_side]
    out[hi_side] = c[nk - 1] + ((3.0 * (c[nk - 1] - c[nk - 2])) / (knots[nk] - knots[nk - 1])) * (t[hi_side] - 1.0)
    mid = ~(lo_side | hi_side)
    tm = t[mid]
    i = _intervals(knots, tm)
    nan = np.isnan(tm)
    i[nan] = 3
    d = [c[i - 3], c[i - 2], c[i - 1], c[i]]
    for r in range(1, 4):
        for j in range(3, r - 1, -1):
            kl = knots[i - 3 + j]
            a = (tm - kl) / (knots[i + 1 + j - r] - kl)
            d[j] = (1.0 - a) * d[j - 1] + a * d[j]
    out[mid] = d[3]
    return out.reshape(x.shape)


class SmoothSpline:
    """A fitted smoothing spline: knots [nk + 4], coef [nk], xmin and range are what the device needs."""

    def __init__(self, knots, coef, xmin, rng, **info):
        self.knots = np.ascontiguousarray(knots, dtype=np.float64)
        self.coef = np.ascontiguousarray(coef, dtype=np.float64)
        self.nk = int(self.coef.size)
        self.xmin = float(xmin)
        self.range = float(rng)
        self.__dict__.update(info)

    def predict(self, x):
        return spline_eval(self.knots, self.coef, self.xmin, self.range, x)


def fmin_brent(f, a, b, tol=SPAR_TOL, eps=SPAR_EPS, maxit=SPAR_MAXIT):
    """Forsythe, Malcolm and Moler's fmin on [a, b]: returns (x, f(x))."""
    c = 0.5 * (3.0 - math.sqrt(5.0))
    v = w = x = a + c * (b - a)
    d = e = 0.0
    fv = fw = fx = f(x)
    for _ in range(maxit):
        xm = 0.5 * (a + b)
        tol1 = eps * abs(x) + tol / 3.0
        tol2 = 2.0 * tol1
        if abs(x - xm) <= tol2 - 0.5 * (b - a):
            break
        golden = True
        if abs(e) > tol1:
            r = (x - w) * (fx - fv)
            q = (x - v) * (fx - fw)
            p = (x - v) * q - (x - w) * r
            q = 2.0 * (q - r)
            if q > 0.0:
                p = -p
            q = abs(q)
            r, e = e, d
            if abs(p) < abs(0.5 * q * r) and p > q * (a - x) and p < q * (b - x):
                d = p / q
                u = x + d
                if (u - a) < tol2 or (b - u) < tol2:
                    d = math.copysign(tol1, xm - x)
                golden = False
        if golden:
            e = (b - x) if x < xm else (a - x)
            d = c * e
        u = x + d if abs(d) >= tol1 else x + math.copysign(tol1, d)
        fu = f(u)
        if fu <= fx:
            if u >= x:
                a = x
            else:
                b = x
            v, fv, w, fw, x, fx = w, fw, x, fx, u, fu
        else:
            if u < x:
                a = u
            else:
                b = u
            if fu <= fw or w == x:
                v, fv, w, fw = w, fw, u, fu
            elif fu <= fv or v == x or v == w:
                v, fv = u, fu
    return x, fx


def merge_points(x, y):
    """(xbar, wbar, ybar, yssw) of the merging rule (module docstring)."""
    x = np.asarray(x, dtype=np.float64).ravel()
    y = np.asarray(y, dtype=np.float64).ravel()
    if x.size != y.size:
        raise ValueError("smooth_spline: x and y differ in length")
    if not (np.isfinite(x).all() and np.isfinite(y).all()):
        raise ValueError("smooth_spline: missing or infinite values in inputs are not allowed")
    if x.size < 4:
        raise ValueError("smooth_spline: need at least four points")
    q1, q3 = np.quantile(x, [0.25, 0.75])
    tol = 1e-6 * (q3 - q1)
    if not (np.isfinite(tol) and tol > 0.0):
        raise ValueError("smooth_spline: 'tol' must be strictly positive and finite")
    xx = np.rint((x - x.mean()) / tol)
    _, first, inv = np.unique(xx, return_index=True, return_inverse=True)
    inv = inv.ravel()
    xbar = x[first]                       # classes ascend with xx, hence with x
    if xbar.size < 4:
        raise ValueError("smooth_spline: need at least four unique 'x' values")
    wbar = np.bincount(inv, minlength=xbar.size).astype(np.float64)
    ybar = np.bincount(inv, weights=y, minlength=xbar.size) / wbar
    yssw = float(np.sum((y - ybar[inv]) ** 2))
    return xbar, wbar, ybar, yssw


class _Problem:
    def __init__(self, x, y, all_knots=False):
        self.xbar, self.wbar, self.ybar, self.yssw = merge_points(x, y)
        nx = self.xbar.size
        self.nx = nx
        self.xmin = float(self.xbar[0])
        self.range = float(self.xbar[-1] - self.xbar[0])
        self.t = (self.xbar - self.xbar[0]) / self.range
        nknots = nx if all_knots else nknots_smspl(nx)
        interior = self.t[knot_indices(nx, nknots)]
        self.knots = np.concatenate([np.repeat(interior[0], 3), interior, np.repeat(interior[-1], 3)])
        self.nk = nk = nknots + 2
        self.w = self.wbar * nx / self.wbar.sum()
        i, N = basis_values(self.knots, self.t)
        X = np.zeros((nx, nk))
        rows = np.arange(nx)
        for r in range(4):
            X[rows, i - 3 + r] = N[:, r]
        self.X = X
        XW = X * self.w[:, None]
        self.XtWX = X.T @ XW
        self.XtWy = XW.T @ self.ybar
        self.Omega = penalty_matrix(self.knots)
        sl = slice(2, nk - 3)             # coefficient indices 3 .. nk - 3, 1-based
        self.ratio = float(np.trace(self.XtWX[sl, sl]) / np.trace(self.Omega[sl, sl]))
        self.sumw = float(self.w.sum())

    def lam(self, spar):
        return self.ratio * 256.0 ** (3.0 * spar - 1.0)

    def solve(self, lam):
        """(coef, df, gcv) at one lambda."""
        A = self.XtWX + lam * self.Omega
        sol = np.linalg.solve(A, np.column_stack([self.XtWy, self.XtWX]))
        coef = sol[:, 0]
        df = float(np.trace(sol[:, 1:]))
        res = self.ybar - self.X @ coef
        rss = float(np.sum(self.w * res * res)) + self.yssw
        gcv = (rss / self.sumw) / (1.0 - df / self.sumw) ** 2
        return coef, df, gcv


def smooth_spline(x, y, spar=None, lam=None, all_knots=False):
    """Fit the smoothing spline of the module docstring.  spar: fixed smoothing parameter (default: the GCV search); lam: a
    fixed lambda on the scaled abscissa instead (spar is then not used); all_knots: every unique x a knot.  Returns a
    SmoothSpline with knots, coef, nk, xmin, range and spar, lam, df, gcv, nx."""
    P = _Problem(x, y, all_knots)
    if lam is None:
        if spar is None:
            spar, _ = fmin_brent(lambda s: P.solve(P.lam(s))[2], SPAR_LOW, SPAR_HIGH)
        lam = P.lam(float(spar))
    coef, df, gcv = P.solve(float(lam))
    return SmoothSpline(P.knots, coef, P.xmin, P.range, spar=None if spar is None else float(spar), lam=float(lam), df=df, gcv=gcv,
                        nx=P.nx, ratio=P.ratio)
