"""Host checks of the K12 restatement (tests/de_restate.py, DESIGN K12) against the published tests: SciPy's mannwhitneyu /
ttest_ind / false_discovery_control, mpmath for pt, NumPy's Philox for the jitter stream, and the mask rules of
.mask_DE_genes (R/inferCNV_mask_non_DE.R:77-134) on hand-built tables.  No GPU needed."""
import math

import numpy as np
import pytest

import de_edge_cases as ec
import de_restate as dr

stats = pytest.importorskip("scipy.stats")


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


@pytest.mark.parametrize("nx,ny", [(1, 1), (2, 7), (10, 10), (49, 49), (49, 50), (50, 49), (30, 120)])
def test_wilcox_matches_scipy(nx, ny):
    rng = np.random.default_rng(nx * 1000 + ny)
    x = rng.normal(size=nx)
    y = rng.normal(size=ny) + 0.4
    W, p, T = dr.wilcox(x, y)
    exact = nx < 50 and ny < 50
    r = stats.mannwhitneyu(x, y, method="exact" if exact else "asymptotic", use_continuity=True)
    assert W == r.statistic and T == 0
    assert rel(p, r.pvalue) <= 1e-12


@pytest.mark.parametrize("nx,ny", [(5, 8), (49, 49), (60, 80), (300, 40)])
def test_wilcox_ties_and_signed_zero(nx, ny):
    rng = np.random.default_rng(nx + ny)
    x = rng.integers(-3, 4, size=nx) * 0.5
    y = rng.integers(-2, 5, size=ny) * 0.5
    x = np.where(x == 0, -0.0, x)                  # -0 and +0 are one tie group
    W, p, T = dr.wilcox(x, y)
    assert T > 0
    r = stats.mannwhitneyu(x, y, method="asymptotic", use_continuity=True)
    assert W == r.statistic
    assert rel(p, r.pvalue) <= 1e-12


def test_wilcox_drops_nonfinite_and_empty():
    x = [1.0, np.nan, 3.0, np.inf]
    y = [2.0, -np.inf, 0.5]
    assert dr.wilcox(x, y)[:2] == dr.wilcox([1.0, 3.0], [2.0, 0.5])[:2]
    assert dr.wilcox([np.nan], [1.0]) is None


def test_exact_tail_counts():
    for m, n in ((1, 1), (3, 4), (7, 5)):
        c = dr.wilcox_counts(m, n)
        assert sum(c) == math.comb(m + n, m) and len(c) == m * n + 1
    assert sum(dr.wilcox_counts(49, 49)) == math.comb(98, 49)


def test_welch_matches_scipy_and_mpmath():
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 40
    rng = np.random.default_rng(2)
    for nx, ny, shift in ((2, 2, 1.0), (5, 40, 0.5), (300, 20, 0.1), (2500, 500, 0.05), (11250, 2500, 0.02), (30, 30, 8.0)):
        x = rng.normal(0.0, 1.0, size=nx)
        y = rng.normal(shift, 2.0, size=ny)
        t, p, df = dr.welch(x, y)
        r = stats.ttest_ind(x, y, equal_var=False)
        assert rel(t, r.statistic) <= 1e-12 and rel(df, r.df) <= 1e-12
        ref = 2 * mpmath.betainc(df / 2, 0.5, 0, df / (df + mpmath.mpf(t) ** 2), regularized=True) / 2
        assert rel(p, float(ref)) <= 1e-12


def test_pt_tail_against_mpmath():
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 50
    for t, df in ((0.3, 1.0), (2.0, 3.5), (10.0, 7.0), (40.0, 120.0), (1e3, 4.0), (37.0, 2000.0), (4.0, 20000.0), (80.0, 6000.0)):
        p = dr.pt2(-t, df)
        ref = float(mpmath.betainc(mpmath.mpf(df) / 2, 0.5, 0, mpmath.mpf(df) / (df + mpmath.mpf(t) ** 2), regularized=True))
        if ref >= 1e-300:
            assert rel(p, ref) <= 1e-12, (t, df, p, ref)


@pytest.mark.parametrize("z", ec.PNORM_POINTS)
def test_pnorm2_regimes_against_mpmath(z):
    # both sides of the 0.674 and 5.657 switches, the fully separated 50 vs 500 ladder rung (11.67) and the deep tail up to
    # the last |z| whose p is still above 1e-300
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 50
    ref = float(mpmath.erfc(mpmath.mpf(z) / mpmath.sqrt(2)))
    assert ref >= 1e-300
    for s in (z, -z):
        assert rel(dr.pnorm2(s), ref) <= 1e-12, (s, dr.pnorm2(s), ref)


def test_pnorm2_points_cover_the_regimes():
    assert {ec.pnorm_regime(z) for z in ec.PNORM_POINTS} == {1, 2, 3}
    assert ec.pnorm_regime(0.67448975) == 1 and ec.pnorm_regime(0.6744898) == 2
    assert ec.pnorm_regime(5.65685) == 2 and ec.pnorm_regime(5.65686) == 3
    for z in (37.5193, 38.7, math.inf):              # from here on R's pnorm returns 0 (2 pnorm(-37.5193) would be about 4e-308)
        assert ec.pnorm_regime(z) == 4 and dr.pnorm2(z) == 0.0 and dr.pnorm2(-z) == 0.0
    assert dr.pnorm2(0.0) == 1.0 and math.isnan(dr.pnorm2(math.nan))


def test_wilcoxon_ladder_reaches_every_regime():
    expr, groups, cmps = ec.wilcoxon_ladder()
    reg = ec.wilcoxon_regimes(expr, groups, cmps)
    ec.check_wilcoxon_ladder(reg)
    _, p, _ = dr.de_tests(expr, groups, cmps, jitter_on=False)
    assert (p[reg == 4] == 0.0).all() and np.isnan(p[reg == 0]).all() and (p[(reg > 0) & (reg < 4)] > 0.0).all()
    z = [ec.wilcox_z(expr[3, groups[a]].tolist(), expr[3, groups[b]].tolist()) for a, b in cmps[4:]]
    assert 37.5193 <= -z[0] < 37.6 and 37.4 < -z[1] < 37.5193
    assert p[4, 3] == 0.0 and 2.3e-308 < p[5, 3] < 2e-307     # the formula would not underflow at either: the cut decides


def test_exact_table_ends():
    expr, groups, cmps = ec.exact_ends()
    W, p, _ = dr.de_tests(expr, groups, cmps, jitter_on=False)
    for k, (qx, qy) in enumerate(cmps):
        full = float(len(groups[qx]) * len(groups[qy]))
        assert {W[k, 0], W[k, 1]} == {0.0, full}
        if full < 50 * 49:                           # the exact table: the two ends are one arrangement out of choose(n, n.x)
            assert ec.wilcox_z(expr[0, groups[qx]].tolist(), expr[0, groups[qy]].tolist()) is None
            end = min(1.0, 2.0 / math.comb(len(groups[qx]) + len(groups[qy]), len(groups[qx])))
            assert rel(p[k, 0], end) <= 1e-15 and p[k, 0] == p[k, 1]
        else:
            assert ec.wilcox_z(expr[0, groups[qx]].tolist(), expr[0, groups[qy]].tolist()) is not None


def test_pt2_ladder_against_mpmath():
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 50
    expr, groups, cmps = ec.welch_ladder()
    pts = ec.welch_points(expr, groups, cmps)
    ec.check_welch_ladder(pts)
    for r in range(len(ec.WELCH_RUNGS)):
        t, df, p = pts[r, r]
        assert p == dr.pt2(-abs(t), df)
        ref = float(mpmath.betainc(mpmath.mpf(df) / 2, 0.5, 0, mpmath.mpf(df) / (df + mpmath.mpf(t) ** 2), regularized=True))
        if ref >= 1e-300:
            assert rel(p, ref) <= 1e-12, (ec.WELCH_RUNGS[r], t, df, p, ref)


def test_exact_mean_fast_is_exact_mean():
    rng = np.random.default_rng(8)
    for v in (rng.normal(1.0, 0.3, size=5000), rng.normal(0.0, 1.0, size=4097) * 10.0 ** rng.integers(-3, 4, size=4097),
              np.array([1e16, 1.0, -1e16, 3.0]), np.array([-0.0, 5e-324, -2.5])):
        assert ec.exact_mean_fast(v) == dr.exact_mean(v)


def test_welch_na_rules():
    nan = math.nan
    assert math.isnan(dr.welch([1.0], [1.0, 2.0])[1])
    assert math.isnan(dr.welch([1.0, 2.0, np.inf], [1.0, 2.0])[1])
    assert math.isnan(dr.welch([3.0, 3.0, 3.0], [3.0, 3.0])[1])
    assert not math.isnan(dr.welch([1.0, 2.0, nan], [1.0, 2.5])[1])


def test_bh_matches_scipy_with_na():
    rng = np.random.default_rng(4)
    p = rng.uniform(size=200) ** 3
    p[::7] = p[3]                                  # ties
    got = dr.bh(p)
    ref = stats.false_discovery_control(p, method="bh")
    assert np.allclose(got, ref, rtol=1e-15, atol=0)
    q = p.copy()
    q[[5, 50, 120]] = np.nan
    got = dr.bh(q)
    ok = ~np.isnan(q)
    assert np.isnan(got[~ok]).all()
    assert np.allclose(got[ok], stats.false_discovery_control(q[ok], method="bh"), rtol=1e-15, atol=0)
    assert np.array_equal(dr.bh([0.3]), [0.3])


def test_jitter_stream_is_numpy_philox():
    seed, g, c = 12345, 7, 42
    bg = np.random.Philox(key=np.array([seed, dr.JITTER_TOKEN], dtype=np.uint64), counter=np.array([0, g, c, 0], dtype=np.uint64))
    u = np.random.Generator(bg).random(2)
    z = dr.qnorm_lib((math.floor(2.0 ** 27 * u[0]) + u[1]) / 2.0 ** 27)
    assert dr.jitter(seed, g, c) == 1e-4 + 1e-4 * z
    for pp in (1e-12, 0.01, 0.3, 0.5, 0.9, 0.999999):
        assert rel(dr.qnorm_lib(pp), stats.norm.ppf(pp)) <= 1e-14 or abs(stats.norm.ppf(pp)) < 1e-300
    assert rel(dr.pnorm2(1.7), 2 * stats.norm.sf(1.7)) <= 1e-14
    assert rel(dr.pnorm2(-9.0), 2 * stats.norm.sf(9.0)) <= 1e-13
    assert dr.exp_lib(-800.0) == 0.0 and rel(dr.exp_lib(-700.0), math.exp(-700.0)) <= 1e-15


def test_jitter_matrix_is_the_jitter_of_every_gene_and_cell():
    for seed, G, C in ((0, 3, 700), (2**63 + 5, 9, 130)):
        J = ec.jitter_matrix(seed, G, C)
        assert all(J[g, c] == dr.jitter(seed, g, c) for g in range(G) for c in range(C))
        assert ec.jitter_sample_matches(J, seed) and not ec.jitter_sample_matches(J, seed + 1)


def test_mask_rules_hand_built():
    # 2 genes x 7 cells: 0-1 reference, 2-3 a 2-cell subcluster, 4-6 a large subcluster with comparisons 0 and 1, N = 2
    expr = np.arange(14, dtype=np.float64).reshape(2, 7)
    padj = np.array([[0.01, 0.5], [0.01, 0.01]])       # gene 0 DE vs both normals, gene 1 vs one
    base = [2, 2, 2, 2, 0, 0, 0]
    cell_cmps = [[], [], [], [], [0, 1], [0, 1], [0, 1]]
    got = dr.mask(expr, padj, 0.05, base, cell_cmps, 2, "any", -1.0)
    assert np.array_equal(got, expr)
    got = dr.mask(expr, padj, 0.05, base, cell_cmps, 2, "all", -1.0)
    assert np.array_equal(got[0], expr[0]) and np.array_equal(got[1], [7, 8, 9, 10, -1, -1, -1])
    got = dr.mask(expr, padj, 0.05, base, cell_cmps, 2, "most", -1.0)
    assert np.array_equal(got, expr)                    # 1 < 2 / 2 is false
    got = dr.mask(expr, np.array([[0.5, 0.5], [0.5, 0.5]]), 0.05, base, cell_cmps, 2, "most", -1.0)
    assert np.array_equal(got[:, 4:], np.full((2, 3), -1.0)) and np.array_equal(got[:, :4], expr[:, :4])
    got = dr.mask(expr, np.array([[np.nan, np.nan]]).T.repeat(2, 1), 0.05, base, [[], [], [], [], [], [], [0]], 2, "any", -1.0)
    assert np.array_equal(got[:, 6], [-1.0, -1.0])      # NA is never DE
    with pytest.raises(ValueError):
        dr.mask(expr, padj, 0.05, base, cell_cmps, 2, "some", -1.0)


def test_mean_is_correctly_rounded():
    v = [1e16, 1.0, -1e16, 3.0]
    assert dr.exact_mean(np.array(v)) == 1.0


def test_perm_and_bad_rules_raise():
    from infercnv_amd import GeneOrder, InfercnvObject
    from infercnv_amd.mask_non_de import get_DE_genes_basic, mask_non_DE_genes_basic
    obj = InfercnvObject(expr_data=np.zeros((3, 4)), gene_order=GeneOrder(chr=np.array(["1"] * 3)),
                         reference_grouped_cell_indices={"n": np.array([0, 1])}, observation_grouped_cell_indices={"t": np.array([2, 3])})
    with pytest.raises(NotImplementedError):
        mask_non_DE_genes_basic(obj, test_use="perm")
    with pytest.raises(NotImplementedError):
        get_DE_genes_basic(obj, test_use="perm")
    with pytest.raises(ValueError):
        mask_non_DE_genes_basic(obj, require_DE_all_normals="some")
    with pytest.raises(ValueError):
        mask_non_DE_genes_basic(obj, test_use="ks")
