"""Sequential restatement of the K16 contract (include/icnv.h "window smoothers of step 10", DESIGN K16), written from
R/inferCNV_ops.R:2534-2704 and the contract -- NOT through the window tables of infercnv_amd/smooth_windows.py.  Matrices are
genes x cells; every output is a sum that starts at 0.0 and takes one product and one add per window row, in row order, then
one division.  The cells are carried as a vector: the operations of one (gene, cell) are still the scalar ones, in order.

  - runmeans: caTools::runmean(k, endrule = "mean") with K10's alignment (k2 = k // 2, window [o - (k - 1 - k2), o + k2]
    clipped to the chromosome), per chromosome of more than one gene.
  - coordinates: .smooth_helper_by_coordinates line by line: the index set, the always-taken padding branch, R's recycling of
    a weight vector that is shorter than the index range, sum(obs * weights) / sum(weights).
"""
import numpy as np

from infercnv_amd import smooth_windows as sw


def runmean_chr(X, window):
    """One chromosome (n x C).  Term j of every window is added in pass j: the genes whose window has a row j are a head part
    (windows clipped at row 0, they all read row j) and an interior part (window o reads row o - left + j)."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    k = min(int(window), n)
    if n <= 1 or k <= 1:
        return X.copy()
    k2 = k // 2
    left = k - 1 - k2
    S = np.zeros_like(X)
    for j in range(k):
        a = max(0, j - k2)                       # head: o < left, lo = 0, row j is in the window iff j <= o + k2
        b = min(left, n)
        if a < b and j <= n - 1:
            S[a:b] = S[a:b] + X[j]
        o_max = min(n - 1, n - 1 + left - j)     # interior: o >= left, row o - left + j <= n - 1
        if left <= o_max:
            S[left:o_max + 1] = S[left:o_max + 1] + X[j:j + o_max + 1 - left]
    o = np.arange(n)
    length = np.minimum(n - 1, o + k2) - np.maximum(0, o - left) + 1
    return S / length.astype(np.float64)[:, None]


def runmeans(X, chr_start, window):
    X = np.asarray(X, dtype=np.float64)
    out = X.copy()
    for a, b in zip(chr_start[:-1], chr_start[1:]):
        if b - a > 1:
            out[a:b] = runmean_chr(X[a:b], window)
    return out


def coordinates_chr(X, start, stop, window_length, info=None):
    """One chromosome (n x C) through .smooth_helper_by_coordinates; 1-based R indices are 0-based here.  info (a dict)
    counts the genes that took the empty-set fallback and those whose index set was not contiguous."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    start = np.asarray(start, dtype=np.float64)
    stop = np.asarray(stop, dtype=np.float64)
    if n <= 1 or window_length < 2:
        return X.copy()
    end = X.copy()
    for i in range(n):
        current_pos = (start[i] + stop[i]) / 2
        around = [j for j in range(n) if start[j] > current_pos - window_length and stop[j] < current_pos + window_length]
        if len(around) == 0:
            around = [i]
            if info is not None:
                info["fallback"] = info.get("fallback", 0) + 1
        weights = [1 - abs((stop[j] + start[j]) / 2 - current_pos) / window_length for j in around]
        # length(around_indices < 10) is the length of a logical vector: always true
        to_add = len(around) // 2
        new_low = max(0, min(around) - to_add)
        new_high = min(n - 1, max(around) + to_add)
        weights = [0.1] * (min(around) - new_low) + weights + [0.1] * (new_high - max(around))
        idx = list(range(new_low, new_high + 1))
        if len(weights) != len(idx) and info is not None:
            info["noncontiguous"] = info.get("noncontiguous", 0) + 1
        num = np.zeros(X.shape[1])
        for t, j in enumerate(idx):                       # obs_data[around_indices] * weights, weights recycled
            num = num + X[j] * weights[t % len(weights)]
        den = 0.0
        for wt in weights:                                # sum(weights): the unrecycled vector
            den = den + wt
        end[i] = num / den
    return end


def coordinates(X, chr_start, start, stop, window_length, info=None):
    X = np.asarray(X, dtype=np.float64)
    out = X.copy()
    for a, b in zip(chr_start[:-1], chr_start[1:]):
        if b - a > 1:
            out[a:b] = coordinates_chr(X[a:b], start[a:b], stop[a:b], window_length, info)
    return out


def layout60(seed=20):
    """The 60-gene chromosome of the tests: sorted random starts in 1 .. 3e6, lengths 1e3 .. 6e4, three genes of 9e5."""
    rng = np.random.default_rng(seed)
    start = np.sort(rng.integers(1, 3_000_001, size=60)).astype(np.float64)
    length = rng.integers(1_000, 60_001, size=60).astype(np.float64)
    length[[7, 29, 48]] = 900_000.0
    return start, start + length


def on_object(obj, method, window_length):
    """The restated smoother applied per chromosome of an InfercnvObject's own (possibly interleaved) gene order."""
    chrs = np.asarray(obj.gene_order.chr)
    out = np.asarray(obj.expr_data, dtype=np.float64).copy()
    seen = []
    for c in chrs:
        if c not in seen:
            seen.append(c)
    for c in seen:
        idx = np.nonzero(chrs == c)[0]
        if idx.size > 1:
            if method == "runmeans":
                out[idx] = runmean_chr(obj.expr_data[idx], window_length)
            else:
                out[idx] = coordinates_chr(obj.expr_data[idx], np.asarray(obj.gene_order.start)[idx],
                                           np.asarray(obj.gene_order.stop)[idx], window_length)
    return out


def pyramid_windows(chr_start, window_length):
    """The generic table of the pyramidinal smoother for chromosomes longer than the window: weights T + 1 - |q - o| over
    [o - T, o + T] clipped to the chromosome, divided by the sum of the included weights (R/inferCNV_ops.R:2410-2440)."""
    T = (int(window_length) - 1) // 2
    lo, ln, den, rows = [], [], [], []
    for a, b in zip(chr_start[:-1], chr_start[1:]):
        n = b - a
        assert n > window_length
        for o in range(n):
            q0, q1 = max(0, o - T), min(n - 1, o + T)
            wts = np.array([T + 1 - abs(q - o) for q in range(q0, q1 + 1)], dtype=np.float64)
            lo.append(a + q0)
            ln.append(q1 - q0 + 1)
            den.append(float(wts.sum()))
            rows.append(wts)
    ln = np.array(ln, dtype=np.int32)
    return sw.WindowTable(np.array(lo, dtype=np.int32), ln, np.array(den), np.concatenate([[0], np.cumsum(ln, dtype=np.int64)]),
                          np.concatenate(rows))
