"""The mean-variance trend of the PCA route's variable-feature selection (FindVariableFeatures, selection.method = "vst",
loess.span = 0.3; .leiden_seurat_preprocess_routine, R/inferCNV_tumor_subclusters.R:706; DESIGN K18), on the host in float64.

R's `loess(log10(var) ~ log10(mean), span = 0.3)` fits local quadratics at the vertices of a kd-tree and blends them
(surface = "interpolate"); that cannot be restated.  This module is the library's contract instead: the same local quadratic
fit with tricube weights over the q nearest points, evaluated DIRECTLY at every point's own x.  Believed close to R's curve,
not verified against it.

Evaluation order (every operation rounded by itself; `seq` is the sequential sum in ascending order of the sorted x):
  1. the points are sorted by x, stably (ties keep their input order); q = floor(span m + 1e-5).
  2. for point i the window is the q consecutive sorted points that minimise the larger of the two end distances, the
     leftmost such window: lo = max(0, i - q + 1), then lo advances while lo + q < m and x[lo + q] - x[i] < x[i] - x[lo].
     h = max(x[i] - x[lo], x[lo + q - 1] - x[i]) is the distance of the q-th nearest point.
  3. u_j = (x_j - x_i) / h, a_j = |u_j|, w_j = ((1 - (a a) a)^2)(1 - (a a) a) where a_j < 1, else 0 (h = 0: every weight 0).
  4. S0 = seq(w), S1 = seq(w u), S2 = seq((w u) u), S3 = seq(((w u) u) u), S4 = seq((((w u) u) u) u),
     T0 = seq(w y), T1 = seq((w u) y), T2 = seq(((w u) u) y).
  5. the fitted value is the intercept of the weighted least-squares quadratic in u, by Cramer's rule:
     c00 = S2 S4 - S3 S3, c01 = S1 S4 - S2 S3, c02 = S1 S3 - S2 S2, det = (S0 c00 - S1 c01) + S2 c02,
     num = (T0 c00 - T1 c01) + T2 c02, fit = num / det.
A window with fewer than 3 distinct x of positive weight has no quadratic: `ok` is False there (fit NaN)."""
from __future__ import annotations

import numpy as np

SPAN = 0.3   # FindVariableFeatures' loess.span


def window_points(m: int, span: float = SPAN) -> int:
    """q = floor(span m + 1e-5): the points of a window (R's lowesd)."""
    return int(np.floor(span * m + 1e-5))


def _seq(v):
    return float(np.cumsum(v)[-1])


def loess_fit(x, y, span: float = SPAN):
    """(fit, ok): the local quadratic fit of y on x at every x, in input order, and whether every window had 3 distinct x of
    positive weight (and q >= 1)."""
    x = np.asarray(x, dtype=np.float64).ravel()
    y = np.asarray(y, dtype=np.float64).ravel()
    if x.shape != y.shape:
        raise ValueError("x and y must have the same length")
    m = x.size
    q = window_points(m, span)
    fit = np.full(m, np.nan)
    if q < 1 or q > m:
        return fit, False
    order = np.argsort(x, kind="stable")
    xs, ys = x[order], y[order]
    ok = True
    lo = 0
    for i in range(m):
        lo = max(lo, i - q + 1, 0)
        while lo + q < m and xs[lo + q] - xs[i] < xs[i] - xs[lo]:
            lo += 1
        xi = xs[i]
        h = max(xi - xs[lo], xs[lo + q - 1] - xi)
        xw = xs[lo:lo + q]
        if not h > 0:
            ok = False
            continue
        u = (xw - xi) / h
        a = np.abs(u)
        t = 1.0 - (a * a) * a
        w = np.where(a < 1.0, (t * t) * t, 0.0)
        pos = xw[w > 0]
        if pos.size < 3 or 1 + int(np.count_nonzero(np.diff(pos) > 0)) < 3:
            ok = False
            continue
        yw = ys[lo:lo + q]
        wu = w * u
        wuu = wu * u
        wuuu = wuu * u
        S0, S1, S2, S3, S4 = _seq(w), _seq(wu), _seq(wuu), _seq(wuuu), _seq(wuuu * u)
        T0, T1, T2 = _seq(w * yw), _seq(wu * yw), _seq(wuu * yw)
        c00 = S2 * S4 - S3 * S3
        c01 = S1 * S4 - S2 * S3
        c02 = S1 * S3 - S2 * S2
        det = (S0 * c00 - S1 * c01) + S2 * c02
        num = (T0 * c00 - T1 * c01) + T2 * c02
        fit[order[i]] = num / det
    return fit, ok
