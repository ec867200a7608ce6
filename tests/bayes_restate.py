"""Sequential restatement of the K13 contract of include/icnv.h (icnv_bayes_loglik / icnv_bayes_sample, DESIGN K13): the
mixture model of the HMM-predicted CNV regions, in the documented operation order, one IEEE rounding per operation.  The GPU
is held to it bit for bit; tests/test_bayes_host.py holds it to mathematics (exact categorical / Dirichlet moments, the exact
posterior by enumeration, mpmath).

Streams: every draw is the start of Generator(Philox(key=[seed, token], counter=[0, w1, t, w3])).random():
  cell i of chain ch, iteration t:            w1 = i, w3 = ch 2^40
  attempt j of the gamma of state k:          w1 = k, w3 = ch 2^40 + 2^32 + j     (two draws: u1, u2)
philox_uniforms() is NumPy's Philox4x64-10 restated on uint64 arrays so that a whole iteration's cell draws are one call;
test_bayes_host.py checks it against numpy.random.Philox itself."""
import math

import numpy as np

from de_restate import exp_lib, log_lib, qnorm_lib

GAMMA_ATTEMPTS = 64
_M0, _M1 = 0xD2E7470EE14C6C93, 0xCA5A826395121157
_W0, _W1 = 0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B
_MASK32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def fnv1a64(name):
    h = 0xCBF29CE484222325
    for b in str(name).encode("utf-8"):
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def _mulhilo(a, b):
    """(high, low) 64-bit halves of the 128-bit product of the constant a and the uint64 array b."""
    a_lo, a_hi = np.uint64(a & 0xFFFFFFFF), np.uint64(a >> 32)
    b_lo, b_hi = b & _MASK32, b >> _S32
    ll = a_lo * b_lo
    lh = a_lo * b_hi
    hl = a_hi * b_lo
    hh = a_hi * b_hi
    mid = (ll >> _S32) + (lh & _MASK32) + (hl & _MASK32)
    hi = hh + (lh >> _S32) + (hl >> _S32) + (mid >> _S32)
    return hi, np.uint64(a) * b


_M64 = 0xFFFFFFFFFFFFFFFF


def philox_scalar(seed, token, w1, w2, w3, n_draws=1):
    """The same for ONE stream in Python integers: a list of n_draws (<= 4) floats."""
    x0, x1, x2, x3 = 1, int(w1) & _M64, int(w2) & _M64, int(w3) & _M64
    k0, k1 = int(seed) & _M64, int(token) & _M64
    for rnd in range(10):
        if rnd:
            k0 = (k0 + _W0) & _M64
            k1 = (k1 + _W1) & _M64
        p0, p1 = _M0 * x0, _M1 * x2
        x0, x1, x2, x3 = (p1 >> 64) ^ x1 ^ k0, p1 & _M64, (p0 >> 64) ^ x3 ^ k1, p0 & _M64
    return [float(w >> 11) * (1.0 / 9007199254740992.0) for w in (x0, x1, x2, x3)[:n_draws]]


def philox_uniforms(seed, token, w1, w2, w3, n_draws=1):
    """The first n_draws (<= 4) random() of the streams with counter [0, w1, w2, w3]; w1 may be an array.  [len(w1), n_draws]."""
    w1 = np.atleast_1d(np.asarray(w1, dtype=np.uint64))
    with np.errstate(over="ignore"):
        x0 = np.full(w1.shape, 1, dtype=np.uint64)          # counter word 0 is incremented before the first block
        x1 = w1.copy()
        x2 = np.full(w1.shape, w2, dtype=np.uint64)
        x3 = np.full(w1.shape, w3, dtype=np.uint64)
        k0, k1 = int(seed) & 0xFFFFFFFFFFFFFFFF, int(token) & 0xFFFFFFFFFFFFFFFF
        for rnd in range(10):
            if rnd:
                k0 = (k0 + _W0) & 0xFFFFFFFFFFFFFFFF
                k1 = (k1 + _W1) & 0xFFFFFFFFFFFFFFFF
            hi0, lo0 = _mulhilo(_M0, x0)
            hi1, lo1 = _mulhilo(_M1, x2)
            x0, x1, x2, x3 = hi1 ^ x1 ^ np.uint64(k0), lo1, hi0 ^ x3 ^ np.uint64(k1), lo0
    words = np.stack([x0, x1, x2, x3], axis=-1)[:, :n_draws]
    return (words >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def loglik(expr, regions, mu, tau):
    """expr: G x C; regions: list of (gene index run (0-based, contiguous), cell index vector).  Returns ll, L [rows x K]."""
    expr = np.asarray(expr, dtype=np.float64)
    K = len(mu)
    rows = sum(len(c) for _, c in regions)
    ll = np.empty((rows, K))
    L = np.empty((rows, K))
    row = 0
    for genes, cells in regions:
        ng = len(genes)
        for c in cells:
            for k in range(K):
                m, t = float(mu[k]), float(tau[k])
                ssq = 0.0
                for g in genes:
                    d = float(expr[g, c]) - m
                    ssq = ssq + d * d
                ll[row, k] = (float(ng) * 0.5) * log_lib(t) - (t * 0.5) * ssq
            mx = ll[row, 0]
            for k in range(1, K):
                if ll[row, k] > mx:
                    mx = ll[row, k]
            for k in range(K):
                L[row, k] = exp_lib(ll[row, k] - mx)
            row += 1
    return ll, L


def gamma_draw(shape, seed, token, k, t, ch):
    d = shape - 1.0 / 3.0
    c = 1.0 / math.sqrt(9.0 * d)
    for att in range(GAMMA_ATTEMPTS):
        u1, u2 = philox_scalar(seed, token, k, t, (ch << 40) + (1 << 32) + att, 2)
        if u1 == 0.0:
            continue
        x = qnorm_lib(u1)
        v = 1.0 + c * x
        if not v > 0.0:
            continue
        v = (v * v) * v
        x2 = x * x
        if u2 < 1.0 - 0.0331 * (x2 * x2):
            return d * v
        if log_lib(u2) < 0.5 * x2 + d * ((1.0 - v) + log_lib(v)):
            return d * v
    return d


def theta_step(n, seed, token, t, ch):
    g = [gamma_draw(1.0 + float(nk), seed, token, k, t, ch) for k, nk in enumerate(n)]
    S = 0.0
    for v in g:
        S = S + v
    return np.array([v / S for v in g])


def cell_step(theta, L, seed, token, t, ch, cells=None):
    """eps of the rows `cells` (default all) of L.  NumPy's elementwise double operations are the contract's roundings."""
    n, K = L.shape
    idx = np.arange(n) if cells is None else np.asarray(cells)
    Lr = L[idx]
    if len(idx) <= 8:
        u = np.array([philox_scalar(seed, token, i, t, ch << 40)[0] for i in idx])
    else:
        u = philox_uniforms(seed, token, idx, t, ch << 40)[:, 0]
    w = theta[None, :] * Lr
    cum = np.zeros(len(idx))
    cums = np.empty_like(w)
    for k in range(K):
        cum = cum + w[:, k]
        cums[:, k] = cum
    thr = u * cum
    eps = np.full(len(idx), -1)
    for k in range(K - 1, -1, -1):
        eps[cums[:, k] > thr] = k
    none = eps < 0
    if none.any():
        for j in np.nonzero(none)[0]:
            last_w = [k for k in range(K) if w[j, k] > 0.0]
            last_l = [k for k in range(K) if Lr[j, k] > 0.0]
            eps[j] = last_w[-1] if last_w else (last_l[-1] if last_l else 0)
    return eps


def sample_region(L, token, K, n_adapt=500, n_burn=200, n_keep=1000, seed=0, final_state=False):
    """One region: theta_sum [K chains x K], theta_samples [K chains x n_keep x K], freq [cells x K] (int).
    final_state: also the last theta and eps of every chain (the host tests' independent draws)."""
    L = np.asarray(L, dtype=np.float64).reshape(-1, K)
    n = L.shape[0]
    theta_sum = np.full((K, K), np.nan)
    samples = np.full((K, n_keep, K), np.nan)
    freq = np.zeros((n, K), dtype=np.int32)
    finals = []
    if n == 0:
        return (theta_sum, samples, freq, finals) if final_state else (theta_sum, samples, freq)
    rows = np.arange(n)
    for ch in range(K):
        counts = np.zeros(K, dtype=np.int64)
        counts[ch] = n
        tsum = np.zeros(K)
        theta = eps = None
        for t in range(n_adapt + n_burn + n_keep):
            theta = theta_step(counts, seed, token, t, ch)
            eps = cell_step(theta, L, seed, token, t, ch)
            counts = np.bincount(eps, minlength=K)
            if t >= n_adapt + n_burn:
                samples[ch, t - n_adapt - n_burn] = theta
                tsum = tsum + theta
                freq[rows, eps] += 1
        theta_sum[ch] = tsum
        finals.append((theta, eps))
    return (theta_sum, samples, freq, finals) if final_state else (theta_sum, samples, freq)


def sample(L, cell_off, tokens, K, n_adapt=500, n_burn=200, n_keep=1000, seed=0):
    """Every region of a call: theta_sum [R x K x K], theta_samples [R x K x n_keep x K], freq [rows x K]."""
    L = np.asarray(L, dtype=np.float64).reshape(-1, K)
    R = len(tokens)
    theta_sum = np.empty((R, K, K))
    samples = np.empty((R, K, n_keep, K))
    freq = np.zeros((L.shape[0], K), dtype=np.int32)
    for r in range(R):
        a, b = int(cell_off[r]), int(cell_off[r + 1])
        theta_sum[r], samples[r], freq[a:b] = sample_region(L[a:b], tokens[r], K, n_adapt, n_burn, n_keep, seed)
    return theta_sum, samples, freq


def theta_mean(theta_sum, n_keep):
    """colMeans of the K n_keep kept samples of a region: the chain sums added in chain order, divided once."""
    K = theta_sum.shape[-1]
    tot = np.zeros(theta_sum.shape[:-2] + (K,))
    for ch in range(K):
        tot = tot + theta_sum[..., ch, :]
    return tot / float(K * n_keep)
