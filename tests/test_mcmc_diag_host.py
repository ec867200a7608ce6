"""The K31 diagnostics without a GPU: the sequential restatement of tests/mcmc_diag_restate.py against independent code (SciPy's
Toeplitz solver, numpy.quantile, vectorised NumPy in another summation order) on seeded AR(1), white-noise and Dirichlet-like
series; the degenerate cases, the refusals, the window formulas; the .dat writer byte for byte; the run() hooks.

The tolerances are 10 x the largest relative difference measured over THIS file's inputs on the CPU it was written on (the
measured value stands beside each constant).  They bound rounding differences between two evaluation orders, not the method."""
import ctypes as ct
import math
import os

import numpy as np
import pytest

import mcmc_diag_restate as mr

KINDS = ("ar1", "white", "dirichlet")
SHAPES = ((3, 20), (3, 21), (6, 64), (2, 100), (6, 1000), (6, 1365))

TOL_AR = 3.0e-15         # measured 2.99e-16: phi of the chosen order (orders 1 .. 8 occur) vs solve_toeplitz, relative to max |phi|
TOL_SPEC0 = 8.6e-15      # measured 8.56e-16: spec0 rebuilt from solve_toeplitz's coefficients
TOL_QUANTILE = 2.2e-15   # measured 2.12e-16: numpy.quantile(method="linear") on the same values
TOL_AUTOCOV = 2.3e-14    # measured 2.30e-15: c[l] by a dot product about numpy.mean, relative to c[0]
TOL_MOMENTS = 5.6e-14    # measured 5.52e-15: means, variances, pooled mean and sd vs numpy's pairwise sums
TOL_PSRF = 2.2e-15       # measured 2.17e-16: psrf by coda's formulas on numpy.var / numpy.cov


def cases():
    for kind in KINDS:
        for i, (m, n) in enumerate(SHAPES):
            yield kind, m, n, mr.make_series(kind, m, n, 1000 + 7 * i)


def rel(a, b, scale=None):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    s = np.max(np.abs(b)) if scale is None else scale
    return float(np.max(np.abs(a - b)) / s) if a.size else 0.0


def test_ar_coefficients_against_solve_toeplitz(capsys):
    from scipy.linalg import solve_toeplitz
    worst_phi = worst_spec = 0.0
    orders = set()
    for kind, m, n, X in cases():
        for x in X:
            for lo, w in mr.windows(n):
                mean, c, spec0, order, phi = mr.window_fit(x, lo, w)
                p = int(order)
                orders.add(p)
                assert len(phi) == p and 0 <= p <= mr.max_order(w)
                if p == 0 or p + 1 >= w:
                    continue
                ref = solve_toeplitz(np.array(c[:p]), np.array(c[1:p + 1]))
                worst_phi = max(worst_phi, rel(phi, ref))
                v = c[0] - float(np.dot(ref, c[1:p + 1]))
                ref_spec = v * w / (w - (p + 1)) / (1.0 - ref.sum()) ** 2
                worst_spec = max(worst_spec, abs(spec0 - ref_spec) / abs(ref_spec))
    with capsys.disabled():
        print(f"\n[mcmc_diag] phi vs solve_toeplitz: {worst_phi:.3g}; spec0: {worst_spec:.3g}; orders seen: {sorted(orders)}")
    assert len(orders) >= 4 and 0 in orders                     # white noise picks 0, the AR(1) paths pick more
    assert worst_phi <= TOL_AR and worst_spec <= TOL_SPEC0


def test_quantiles_against_numpy(capsys):
    worst = 0.0
    for kind, m, n, X in cases():
        srt = np.sort(X.ravel())
        for p in (0.025, 0.5, 0.975, 0.0, 1.0, 1.0 / 3.0):
            got, want = mr.quantile7(srt, p), float(np.quantile(X.ravel(), p, method="linear"))
            worst = max(worst, abs(got - want) / max(abs(want), 1e-300))
    with capsys.disabled():
        print(f"\n[mcmc_diag] quantile7 vs numpy.quantile: {worst:.3g}")
    assert worst <= TOL_QUANTILE
    ties = mr.make_series("ties", 4, 37, 3)
    po = mr.pooled_stats(ties, [mr.chain_stats(x) for x in ties])
    for q, p in zip(po[2:5], (0.025, 0.5, 0.975)):
        want = float(np.quantile(ties.ravel() + 0.0, p, method="linear"))
        assert abs(q - want) <= TOL_QUANTILE * abs(want)
    assert not any(math.copysign(1.0, q) < 0 for q in po[2:5] if q == 0.0)      # -0.0 is reported as +0.0


def coda_psrf(X):
    """gelman.diag's point estimate (transform = FALSE, autoburnin = FALSE) as coda's source writes it, on numpy's moments."""
    m, n = X.shape
    xbar, s2 = X.mean(axis=1), X.var(axis=1, ddof=1)
    W, B = s2.mean(), n * xbar.var(ddof=1)
    muhat = xbar.mean()
    var_w, var_b = s2.var(ddof=1) / m, 2 * B ** 2 / (m - 1)
    cov_wb = (n / m) * (np.cov(s2, xbar ** 2)[0, 1] - 2 * muhat * np.cov(s2, xbar)[0, 1])
    V = (n - 1) * W / n + (1 + 1 / m) * B / n
    var_V = ((n - 1) ** 2 * var_w + (1 + 1 / m) ** 2 * var_b + 2 * (n - 1) * (1 + 1 / m) * cov_wb) / n ** 2
    df = 2 * V ** 2 / var_V
    return math.sqrt((df + 3) / (df + 1) * ((n - 1) / n + (1 + 1 / m) * (1 / n) * (B / W)))


def test_autocovariances_moments_and_psrf_in_another_order(capsys):
    worst_c = worst_m = worst_r = 0.0
    for kind, m, n, X in cases():
        cs = [mr.chain_stats(x) for x in X]
        for x, row in zip(X, cs):
            mean, c, _, _, _ = mr.window_fit(x, 0, n)
            d = x - x.mean()
            ref = np.array([np.dot(d[:n - l], d[l:]) / n for l in range(len(c))])
            worst_c = max(worst_c, rel(c, ref, scale=ref[0]))
            worst_m = max(worst_m, abs(row[0] - x.mean()) / abs(x.mean()), abs(row[1] - x.var(ddof=1)) / x.var(ddof=1))
            for j, lag in zip((5, 6, 7, 8), (1, 5, 10, 50)):
                if lag < n:
                    assert abs(row[j] - np.dot(d[:n - lag], d[lag:]) / np.dot(d, d)) < 1e-12
                else:
                    assert math.isnan(row[j])
        po = mr.pooled_stats(X, cs)
        worst_m = max(worst_m, abs(po[0] - X.mean()) / abs(X.mean()), abs(po[1] - X.std(ddof=1)) / X.std(ddof=1))
        worst_r = max(worst_r, abs(po[5] - coda_psrf(X)) / coda_psrf(X))
        assert po[6] > 0 and po[2] <= po[3] <= po[4]
    with capsys.disabled():
        print(f"\n[mcmc_diag] autocov: {worst_c:.3g}; moments: {worst_m:.3g}; psrf: {worst_r:.3g}")
    assert worst_c <= TOL_AUTOCOV and worst_m <= TOL_MOMENTS and worst_r <= TOL_PSRF


def test_statistics_say_what_they_should():
    """Not a tolerance: the numbers mean what their names say on series whose answer is known."""
    white = mr.make_series("white", 6, 1000, 5)
    cs = [mr.chain_stats(x) for x in white]
    po = mr.pooled_stats(white, cs)
    assert 0.99 < po[5] < 1.01 and 4000 < po[6] < 8000 and all(abs(r[4]) < 4 for r in cs)
    ar = mr.make_series("ar1", 2, 4096, 6)                      # chain 1: rho = 0.9, ess about n (1 - rho) / (1 + rho)
    r = mr.chain_stats(ar[1])
    assert 0.85 < r[5] < 0.95 and 1 <= r[3] <= 36 and 100 < 4096 * r[1] / r[2] < 450
    shifted = white.copy()
    shifted[0] += 3.0                                           # one chain sits elsewhere: not converged
    assert mr.pooled_stats(shifted, [mr.chain_stats(x) for x in shifted])[5] > 1.5
    drift = white[0] + np.linspace(0, 3, 1000)                  # a trend: Geweke's windows disagree
    assert abs(mr.chain_stats(drift)[4]) > 5


def test_degenerate_series():
    nan = np.full((3, 20), np.nan)
    cs = [mr.chain_stats(x) for x in nan]
    assert np.isnan(np.array(cs)).all() and np.isnan(np.array(mr.pooled_stats(nan, cs))).all()
    const = np.full((3, 64), 0.25)                              # sums of 0.25 are exact: c[0] == 0
    cs = [mr.chain_stats(x) for x in const]
    for row in cs:
        assert row[:4] == [0.25, 0.0, 0.0, 0.0] and all(math.isnan(v) for v in row[4:])
    po = mr.pooled_stats(const, cs)
    assert po[:5] == [0.25, 0.0, 0.25, 0.25, 0.25] and math.isnan(po[5]) and po[6] == 0.0
    const[1] = mr.make_series("white", 1, 64, 2)[0]             # one chain moves: W > 0, the constant chains add no ess
    cs = [mr.chain_stats(x) for x in const]
    po = mr.pooled_stats(const, cs)
    assert po[5] > 0 and po[6] == 64 * cs[1][1] / cs[1][2]
    same = np.tile(mr.make_series("white", 1, 40, 3), (3, 1))   # equal chains: var_V == 0, psrf NaN as in coda's formula
    assert math.isnan(mr.pooled_stats(same, [mr.chain_stats(x) for x in same])[5])
    assert mr.psrf([0.1, 0.2], [0.0, 0.0], 50) != mr.psrf([0.1, 0.2], [0.0, 0.0], 50)    # W == 0


def test_windows_and_orders():
    assert mr.windows(20) == ((0, 20), (0, 3), (9, 11))
    assert mr.windows(21) == ((0, 21), (0, 3), (10, 11))
    assert mr.windows(100) == ((0, 100), (0, 11), (49, 51))
    assert mr.windows(1000) == ((0, 1000), (0, 101), (499, 501))
    for n in (20, 21, 100, 1000):                               # A: t in [0, ceil(0.1 (n - 1))], B: t in [floor(0.5 (n - 1)), n - 1]
        full, a, b = mr.windows(n)
        assert a[1] - 1 == math.ceil((n - 1) / 10) and b[0] == math.floor((n - 1) / 2) and b[0] + b[1] == n
    assert [mr.max_order(m) for m in (2, 3, 11, 20, 21, 64, 100, 101, 501, 1000, 1365, 4096)] == [1, 2, 10, 13, 13, 18, 20, 20, 26, 30, 31, 36]
    for m in range(2, 4097):
        if round(10 * math.log10(m), 9) != round(10 * math.log10(m)):          # away from the integers the float formula is safe
            assert mr.max_order(m) == min(m - 1, math.floor(10 * math.log10(m)))


def test_refusals_need_no_gpu():
    from infercnv_amd import _lib
    L = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "icnv.h")).read()
    for name in ("icnv_mcmc_diag_dev", "icnv_mcmc_diag"):
        assert name in _lib.PROTOTYPES and hasattr(L, name) and name + "(" in header
    assert "believed, not verified against coda" in header
    buf = np.zeros(8)
    p = ct.c_void_p(buf.ctypes.data)          # never dereferenced: every call below fails before any device work
    code = {"ARG": _lib.ERR_ARG, "UNSUPPORTED": _lib.ERR_UNSUPPORTED}
    for R, m, n, K in ((1, 6, 19, 6), (1, 6, 0, 6), (1, 1, 100, 6), (1, 9, 100, 6), (1, 6, 100, 1), (1, 6, 100, 9), (0, 6, 100, 6),
                       (1, 6, 1366, 6), (1, 8, 1025, 3), (1, 2, 4097, 2), (2 ** 30, 2, 20, 8)):
        want = mr.refusal(R, m, n, K)
        assert want is not None
        assert L.icnv_mcmc_diag_dev(p, R, m, n, K, p, p, None) == code[want], (R, m, n, K)
        assert L.icnv_mcmc_diag(p, R, m, n, K, p, p) == code[want], (R, m, n, K)
    assert b"8192" in L.icnv_last_error() or b"pairs" in L.icnv_last_error()
    assert L.icnv_mcmc_diag_dev(None, 1, 6, 100, 6, p, p, None) == _lib.ERR_ARG
    for ok in ((1, 6, 1365, 6), (7, 3, 20, 3), (1, 8, 1024, 2), (1, 2, 4096, 8)):
        assert mr.refusal(*ok) is None


def hand_record():
    from infercnv_amd import bayes_net
    cs = np.zeros((2, 2, 2, 9))
    po = np.zeros((2, 2, 7))
    po[0, 0] = [0.5, 0.125, 1e-05, 1.0 / 3.0, 0.75, 1.0, 6000.0]
    po[0, 1] = [0.5, 0.25, 0.0, -0.25, 100000.0, 1.25, 1234567.0]
    po[1, 0] = [np.nan] * 7
    po[1, 1] = [2.0, 0.0, 2.0, 2.0, 2.0, np.nan, 0.0]
    cs[0, 0, 0, 4:] = [-1.5, 0.5, 0.25, 0.125, 0.0625]
    cs[0, 0, 1, 4:] = [9.0, 9.0, 9.0, 9.0, 9.0]                 # chain 1 is in the record, not in the file
    cs[0, 1, 0, 4:] = [2.5, -0.5, 1e-300, 12345.678, np.nan]
    cs[1, 0, 0, 4:] = [np.nan] * 5
    cs[1, 1, 0, 4:] = [np.nan, np.nan, np.nan, np.nan, np.inf]
    return bayes_net.McmcDiagnostics(regions=["chr1-region_1", "chr2-region_12"], chain_stats=cs, pooled=po)


HAND_TEXT = ("Mean\tSt.Dev\t2.5%\t50%\t97.5%\tRhat\tESS\tGeweke\tacf1\tacf5\tacf10\tacf50\n"
             "chr1-region_1:State:1\t0.5\t0.125\t1e-05\t0.333333333333333\t0.75\t1\t6000\t-1.5\t0.5\t0.25\t0.125\t0.0625\n"
             "chr1-region_1:State:2\t0.5\t0.25\t0\t-0.25\t1e+05\t1.25\t1234567\t2.5\t-0.5\t1e-300\t12345.678\tNaN\n"
             "chr2-region_12:State:1\tNaN\tNaN\tNaN\tNaN\tNaN\tNaN\tNaN\tNaN\tNaN\tNaN\tNaN\tNaN\n"
             "chr2-region_12:State:2\t2\t0\t2\t2\t2\tNaN\t0\tNaN\tNaN\tNaN\tNaN\tInf\n")


def test_dat_writer_byte_for_byte(tmp_path):
    from infercnv_amd import bayes_net
    d = hand_record()
    assert d.chain_fields == mr.CHAIN_FIELDS and d.pooled_fields == mr.POOLED_FIELDS and bayes_net.MCMC_TABLE_COLUMNS == mr.TABLE_COLUMNS
    assert np.array_equal(d.table(), mr.table(d.chain_stats, d.pooled), equal_nan=True)
    path = bayes_net.write_mcmc_diagnostics(d, str(tmp_path / "sub"))
    assert os.path.basename(path) == "CNV_MCMC_Diagnostics.dat"
    assert open(path, "rb").read() == HAND_TEXT.encode()


def test_chain_hooks_calls_every_hook_in_order():
    from infercnv_amd import pipeline
    seen = []
    hook = pipeline.chain_hooks(lambda s, l, o: seen.append(("a", s, l, o)), None, lambda s, l, o: seen.append(("b", s, l, o)))
    hook(3, "label", "obj")
    hook(18, "mcmc", "m")
    assert seen == [("a", 3, "label", "obj"), ("b", 3, "label", "obj"), ("a", 18, "mcmc", "m"), ("b", 18, "mcmc", "m")]
    pipeline.chain_hooks()(1, "x", None)


def test_mcmc_diagnostics_hook_ignores_every_step_but_18(monkeypatch, tmp_path):
    from infercnv_amd import bayes_net, pipeline
    calls = []
    monkeypatch.setattr(bayes_net, "mcmc_diagnostics", lambda obj, **kw: calls.append((obj, kw)) or "record")
    args = dict(HMM=True, HMM_type="i6", analysis_mode="samples", BayesMaxPNormal=0.5, cutoff=1, denoise=True)
    hook = pipeline.mcmc_diagnostics_hook(str(tmp_path), max_sample_bytes=12345, **args)
    want_dir = os.path.join(str(tmp_path), pipeline.file_tokens(True, "i6", "samples", "leiden", 0.5)["bayes_dir"])
    assert hook.out_dir == want_dir and os.path.basename(want_dir) == "BayesNetOutput.HMMi6.hmm_mode-samples"
    for step in list(range(1, 18)) + [19, 20, 21, 22]:
        hook(step, "label", object())
    assert calls == [] and hook.diagnostics is None
    hook(18, "Run Bayesian Network Model on HMM predicted CNVs", "the mcmc object")
    assert calls == [("the mcmc object", {"max_sample_bytes": 12345, "out_dir": want_dir})] and hook.diagnostics == "record"
    assert "diagnostics" in pipeline.IGNORED_OPTIONS            # run()'s own argument stays accepted and ignored
    with pytest.raises(ValueError):
        pipeline.mcmc_diagnostics_hook(str(tmp_path), HMM_type="i7")
