"""Host side of the hidden spike-in (DESIGN K15) without a GPU: the fake chromosomes, the smoothing spline against SciPy and
against the dense restatement of tests/hspike_restate.py, the object build_and_add_hspike assembles (its two device calls
replaced by the restatement), and the statistics of the restated simulation at a fixed seed."""
import math

import numpy as np
import pytest

import hspike_restate as hr
from infercnv_amd import hmm
from infercnv_amd import smooth_spline as ss

torch = pytest.importorskip("torch")


# ---------------------------------------------------------------- fake chromosomes
@pytest.mark.parametrize("G,last,total", [(10000, 6000, 10000), (4400, 400, 4400), (4399, 400, 4400), (1000, 400, 4400)])
def test_hspike_chr_info(G, last, total):
    from infercnv_amd.hidden_spike import get_hspike_chr_info
    info = get_hspike_chr_info(400, G)
    assert [(n, c) for n, c, _ in info] == list(hmm.HSPIKE_CHR_INFO)
    assert [n for _, _, n in info] == [400] * 10 + [last]
    assert sum(n for _, _, n in info) == total
    assert info == hr.chr_info(400, G)


# ---------------------------------------------------------------- smoother
def smoother_inputs():
    rng = np.random.default_rng(7)
    x = rng.uniform(0, 5, 300)
    yield "300 points", x, np.sin(x) + 0.1 * rng.standard_normal(300)
    x = np.round(rng.uniform(0, 8, 5000), 2)                       # 5 000 points on 801 distinct abscissae
    yield "5 000 points with ties", x, 1.5 * x - 0.05 * x ** 2 + 0.3 * rng.standard_normal(5000)
    m = np.exp(rng.normal(1.0, 1.5, 20000))                         # a mean-variance cloud: over-dispersed counts, some zero rows
    m[rng.random(20000) < 0.02] = 0.0
    v = m * (1 + 0.4 * m) * np.exp(0.3 * rng.standard_normal(20000))
    yield "mean-variance cloud of 20 000", np.log(m + 1), np.log(v + 1)


def test_smoother_against_scipy_all_knots_fixed_lambda():
    """Every point a knot, lambda = 1e-4 on the scaled abscissa: the fitted values against scipy's make_smoothing_spline.
    Tolerance: 10 x the disagreement of the dense restatement with itself, Cholesky of the normal equations against QR of the
    augmented least-squares system, on these inputs (both routes share the conditioning of the problem).  Measured here:
    route gap 3.2e-11, library against scipy 1.3e-10 (values of size 1)."""
    from scipy.interpolate import make_smoothing_spline
    rng = np.random.default_rng(1)
    x = np.sort(rng.uniform(0, 5, 300))
    y = np.sin(x) + 0.1 * rng.standard_normal(300)
    lam = 1e-4
    D = hr.Dense(x, y, all_knots=True)
    gap = np.abs(D.fitted(D.solve_cholesky(lam)) - D.fitted(D.solve_qr(lam))).max()
    f = ss.smooth_spline(x, y, lam=lam, all_knots=True)
    assert f.nk == 302 and np.array_equal(f.knots, D.knots)
    err = np.abs(make_smoothing_spline(D.t, D.ybar, lam=lam)(D.t) - f.predict(x)).max()
    print(f"route gap {gap:.3e}, library against scipy {err:.3e}")
    assert 0 < gap < 1e-6
    assert err <= 10 * gap


@pytest.mark.parametrize("case", [0, 1, 2])
def test_smoother_default_settings_against_restatement(case):
    """Measured (coefficient gap Cholesky against QR / library against the restatement at the library's spar): 300 points
    2.5e-12 / 1.3e-12, 5 000 with ties 2.1e-10 / 1.5e-10, the cloud 3.1e-12 / 3.4e-12."""
    name, x, y = list(smoother_inputs())[case]
    D = hr.Dense(x, y)
    f = ss.smooth_spline(x, y)
    assert f.nx == D.nx and f.nk == D.nk == hr.nknots(D.nx) + 2
    assert np.array_equal(f.knots, D.knots)                         # the knot vector is identical
    assert f.xmin == D.xmin and f.range == D.range
    assert ss.SPAR_LOW < f.spar < ss.SPAR_HIGH
    lam = D.lam(f.spar)
    assert abs(f.lam - lam) <= 1e-12 * lam
    gap = np.abs(D.solve_cholesky(lam) - D.solve_qr(lam)).max()
    err = np.abs(f.coef - D.solve(lam)).max()
    print(f"{name}: nx {D.nx}, nk {D.nk}, spar {f.spar:.6f}, coefficient route gap {gap:.3e}, library against restatement {err:.3e}")
    assert 0 < gap < 1e-6
    assert err <= 10 * gap
    scale = np.abs(f.coef).max()
    grid = np.array([D.gcv(D.lam(s)) for s in np.linspace(-1.5, 1.5, 301)])
    print(f"  GCV: library {f.gcv:.12g}, grid minimum {grid.min():.12g}")
    assert f.gcv <= grid.min() * (1 + 10 * gap / scale)
    assert abs(f.gcv - D.gcv(lam)) <= 1e-9 * f.gcv


def test_merging_rule():
    x = np.array([0.0, 1.0, 1.0 + 1e-9, 2.0, 3.0, 3.0, 4.0, 1.0])
    y = np.array([1.0, 2.0, 4.0, 0.0, 5.0, 7.0, 1.0, 9.0])
    xbar, wbar, ybar, yssw = ss.merge_points(x, y)
    assert xbar.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]                # the first occurrence stands for its class
    assert wbar.tolist() == [1, 3, 1, 2, 1] and ybar.tolist() == [1.0, 5.0, 0.0, 6.0, 1.0]
    assert yssw == (9 + 1 + 16) + (1 + 1)
    D = hr.Dense(x, y)
    assert D.xbar.tolist() == xbar.tolist() and D.ybar.tolist() == ybar.tolist() and D.yssw == yssw
    with pytest.raises(ValueError):
        ss.smooth_spline([0, 1, 1, 2, 2, 1], [1, 2, 3, 4, 5, 6])    # three unique x
    with pytest.raises(ValueError):
        ss.smooth_spline([0, 1, 2, 3, np.nan], [1, 2, 3, 4, 5])
    with pytest.raises(ValueError):
        ss.smooth_spline([0, 1, 2, 3, 4], [1, 2, np.inf, 4, 5])
    assert [ss.nknots_smspl(n) for n in (4, 49, 50, 51, 200, 800, 3200, 20000)] == [4, 49, 50, 50, 100, 140, 200, 206]
    assert [hr.nknots(n) for n in (4, 49, 50, 51, 200, 800, 3200, 20000)] == [4, 49, 50, 50, 100, 140, 200, 206]


def test_spar_upper_limit_is_the_weighted_line():
    """spar = 1.5: lambda = r 256^3.5.  With P = int f''^2 of the fit, lambda P <= the fit's objective <= the objective of
    the weighted least-squares line L = RSS_L, so P <= RSS_L / lambda.  Taylor about t = 1/2: f = line + rem,
    |rem(t)| <= sqrt(|t - 1/2|^3 P / 3) <= sqrt(P / 24).  The residual of the fit is w-orthogonal to lines (a line added to f
    leaves the penalty alone), so f - L = rem - (projection of rem on lines) and its weighted root mean square is at most
    sup |rem| <= sqrt(RSS_L / (24 lambda))."""
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(0, 4, 500), np.repeat([1.0, 2.5], 30)])       # unequal weights after merging
    y = 2.0 - 0.7 * x + 0.5 * np.sin(2 * x) + 0.2 * rng.standard_normal(x.size)
    f = ss.smooth_spline(x, y, spar=1.5)
    xbar, wbar, ybar, _ = ss.merge_points(x, y)
    w = wbar * xbar.size / wbar.sum()
    A = np.column_stack([np.ones(xbar.size), xbar]) * np.sqrt(w)[:, None]
    beta, *_ = np.linalg.lstsq(A, ybar * np.sqrt(w), rcond=None)
    line = beta[0] + beta[1] * xbar
    rss_line = float(np.sum(w * (ybar - line) ** 2))
    assert f.lam == f.ratio * 256.0 ** 3.5
    bound = math.sqrt(rss_line / (24.0 * f.lam))
    rms = math.sqrt(float(np.sum(w * (f.predict(xbar) - line) ** 2) / w.sum()))
    print(f"lambda {f.lam:.4g}, bound {bound:.3e}, weighted rms distance from the line {rms:.3e}, df {f.df:.6f}")
    assert rms <= bound


def test_prediction_outside_the_range_is_linear():
    from scipy.interpolate import BSpline
    _, x, y = next(smoother_inputs())
    f = ss.smooth_spline(x, y)
    k, c, nk = f.knots, f.coef, f.nk
    lo, hi = f.xmin, f.xmin + f.range
    assert f.predict(np.array([lo]))[0] == c[0] and f.predict(np.array([hi]))[0] == c[-1]
    left = (3.0 * (c[1] - c[0])) / (k[4] - k[3])                   # f'(0) and f'(1) in t: the B-spline derivative rule
    right = (3.0 * (c[nk - 1] - c[nk - 2])) / (k[nk] - k[nk - 1])
    b = BSpline(k, c, 3)
    assert abs(left - b.derivative()(0.0)) <= 1e-9 * abs(left) and abs(right - b.derivative()(1.0)) <= 1e-9 * abs(right)
    for xo in (lo - 0.37, lo - 1e3, hi + 2.5, hi + 1e-9, lo - 1e-12):
        t = (xo - f.xmin) / f.range
        want = c[0] + left * t if t < 0 else c[-1] + right * (t - 1.0)
        assert f.predict(np.array([xo]))[0] == want
        assert hr.spline_eval(k, c, f.xmin, f.range, xo) == want
    xs = np.concatenate([np.linspace(lo - 1, hi + 1, 501), x[:50]])
    got = f.predict(xs)
    assert all(hr.spline_eval(k, c, f.xmin, f.range, v) == g for v, g in zip(xs, got))     # the vector form is the scalar one
    inside = (xs >= lo) & (xs <= hi)
    assert np.abs(got[inside] - b((xs[inside] - f.xmin) / f.range)).max() < 1e-12


# ---------------------------------------------------------------- the restatement's own pieces
def test_array_restatement_is_the_elementwise_one():
    rng = np.random.default_rng(2)
    for first, g, c in ((0, 0, 0), (1, 4399, 99), (2, 17, 0), (0, 2 ** 40, 3)):
        bg = np.random.Philox(key=np.array([9, 77], dtype=np.uint64), counter=np.array([first, g, c, 0], dtype=np.uint64))
        want = bg.random_raw(4)
        got = hr.philox_block(9, 77, first, np.array([g]), np.array([c]))
        assert [int(w[0]) for w in got] == [int(v) for v in want]
    x = np.sort(rng.uniform(0.5, 6.0, 200))
    fv = ss.smooth_spline(x, 1.1 * x - 0.5 + 0.05 * rng.standard_normal(200))
    x2 = np.sort(rng.uniform(-3.0, 5.0, 200))
    fp = ss.smooth_spline(x2, 1.0 / (1.0 + np.exp(1.5 * (x2 - 1.0))))
    means = np.concatenate([[0.0, 1e-3, 0.3, 0.6, 2e4, 2.0 ** 40], np.exp(rng.uniform(-3, 8, 24))])
    sv, sp = (fv.knots, fv.coef, fv.xmin, fv.range), (fp.knots, fp.coef, fp.xmin, fp.range)
    a = hr.simulate_elementwise(means, 21, sv, sp, 3, 41)
    b = hr.simulate(means, 21, sv, sp, 3, 41)
    assert np.array_equal(a, b)
    assert (a[:3] == 0).all() and (a[4:6] > 0).all() and (a == np.rint(a)).all()
    assert (hr.simulate(means, 21, sv, sp, 3, 42) != b).any() and (hr.simulate(means, 21, sv, sp, 4, 41) != b).any()


def constant_spline(c):
    return (np.array([0.0, 0, 0, 0, 0.5, 1, 1, 1, 1]), np.full(5, float(c)), 0.0, 10.0)


def test_statistics_of_the_restated_simulation():
    """Constant variance spline (var = e^c - 1 = 400 at every mean), m = 1 000, 10 000 x 100 values at a fixed seed."""
    c = math.log(401.0)
    m, N = 1000.0, 10000 * 100
    no_drop = hr.simulate(np.full(10000, m), 100, constant_spline(c), constant_spline(-1.0), 1, 2)
    var = math.exp(c) - 1.0 + 1.0 / 12.0                            # rounding to integers adds 1 / 12
    sd = math.sqrt(var)
    print(f"mean {no_drop.mean():.6f} (m {m}), variance {no_drop.var(ddof=1):.4f} (expected {var:.4f})")
    assert abs(no_drop.mean() - m) <= 5 * sd / math.sqrt(N)
    assert abs(no_drop.var(ddof=1) - var) <= 5 * var * math.sqrt(2.0 / (N - 1))
    assert (no_drop > 0).all()
    drop = hr.simulate(np.full(10000, m), 100, constant_spline(c), constant_spline(0.3), 1, 2)
    frac = float((drop == 0).mean())
    print(f"zero fraction {frac:.6f}")
    assert abs(frac - 0.3) <= 5 * math.sqrt(0.3 * 0.7 / N)
    assert np.array_equal(drop[drop != 0], no_drop[drop != 0])      # the dropout only zeroes


# ---------------------------------------------------------------- build_and_add_hspike
class Patched:
    """The device calls of hidden_spike replaced by the restatement, on CPU tensors; records what it was asked."""

    def __init__(self, monkeypatch):
        from infercnv_amd import device, hidden_spike, ops
        self.table_groups, self.mean_groups, self.sim, self.factor, self.colsum_rows = None, None, None, None, None
        monkeypatch.setattr(hidden_spike, "_device_matrix", lambda e: torch.from_numpy(np.ascontiguousarray(np.asarray(e, dtype=np.float64).T)))
        monkeypatch.setattr(device, "group_gene_tables", self.tables)
        monkeypatch.setattr(device, "group_means", self.means)
        monkeypatch.setattr(device, "hspike_simulate", self.simulate)
        monkeypatch.setattr(device, "col_sums", self.col_sums)
        monkeypatch.setattr(ops, "normalize_counts_by_seq_depth", self.normalize)

    def tables(self, x, groups):
        self.table_groups = [np.asarray(g) for g in groups]
        m, v, nz = hr.group_gene_tables(x.numpy().T, groups)
        return torch.from_numpy(m), torch.from_numpy(v), torch.from_numpy(nz)

    def means(self, x, groups):
        self.mean_groups = [np.asarray(g) for g in groups]
        return torch.from_numpy(hr.group_gene_tables(x.numpy().T, groups)[0])

    def simulate(self, means, num_cells, var_spline, p0_spline, seed, tokens, device=None):
        self.sim = dict(means=np.array(means), num_cells=num_cells, seed=seed, tokens=list(tokens), var=var_spline, p0=p0_spline)
        mats = [hr.simulate(mu, num_cells, (var_spline.knots, var_spline.coef, var_spline.xmin, var_spline.range),
                            (p0_spline.knots, p0_spline.coef, p0_spline.xmin, p0_spline.range), seed, tok).T
                for mu, tok in zip(np.atleast_2d(means), tokens)]
        return torch.from_numpy(np.ascontiguousarray(np.stack(mats)))

    def col_sums(self, x):
        self.colsum_rows = x.numpy().copy()
        return torch.from_numpy(x.numpy().sum(axis=1))

    def normalize(self, obj, factor=None):
        self.factor = factor
        new = obj.copy()
        cs = obj.expr_data.sum(axis=0)
        with np.errstate(invalid="ignore", divide="ignore"):
            new.expr_data = np.asfortranarray(obj.expr_data / cs[None, :] * factor)
        return new


def small_object(with_refs=True):
    from infercnv_amd.infercnv_object import GeneOrder, InfercnvObject
    rng = np.random.default_rng(11)
    G, C = 60, 90
    mu = np.exp(rng.normal(1.0, 1.2, G))
    expr = rng.poisson(mu[:, None] * rng.uniform(0.7, 1.3, (1, C))).astype(np.float64)
    expr[rng.random((G, C)) < 0.15] = 0.0
    expr[5, 0:20] = 0.0                                              # gene 5 is never seen in the first reference group
    expr = np.asfortranarray(expr / expr.sum(axis=0)[None, :] * 500.0)
    refs = {"normA": np.arange(0, 20), "normB": np.arange(20, 50)} if with_refs else {}
    obs = {"tumA": np.arange(50, 75), "tumB": np.arange(75, 90)} if with_refs else {"tumA": np.arange(0, 50), "tumB": np.arange(50, 90)}
    return InfercnvObject(expr_data=expr, gene_order=GeneOrder(np.repeat(["chr1", "chr2"], 30)), reference_grouped_cell_indices=refs,
                          observation_grouped_cell_indices=obs)


def check_layout(hs, types):
    n_cells = 200 * len(types)
    assert hs.expr_data.shape == (4400, n_cells) and hs.count_data.shape == (4400, n_cells)
    assert list(hs.gene_names) == [f"gene_{j}" for j in range(1, 4401)]
    chrs = [name for name, _ in hmm.HSPIKE_CHR_INFO for _ in range(400)]
    assert list(hs.gene_order.chr) == chrs
    assert np.array_equal(hs.gene_order.start, np.tile(np.arange(1, 401), 11)) and np.array_equal(hs.gene_order.stop, hs.gene_order.start)
    names, refs, obs = [], {}, {}
    for k, t in enumerate(types):
        names += [f"simnorm_cell_{t}{i}" for i in range(1, 101)] + [f"spike_tumor_cell_{t}{i}" for i in range(1, 101)]
        refs[f"simnorm_cell_{t}"] = np.arange(200 * k, 200 * k + 100)
        obs[f"spike_tumor_cell_{t}"] = np.arange(200 * k + 100, 200 * k + 200)
    assert list(hs.cell_names) == names
    assert list(hs.reference_grouped_cell_indices) == list(refs) and list(hs.observation_grouped_cell_indices) == list(obs)
    assert all(np.array_equal(hs.reference_grouped_cell_indices[k], v) for k, v in refs.items())
    assert all(np.array_equal(hs.observation_grouped_cell_indices[k], v) for k, v in obs.items())
    assert (hs.count_data == np.rint(hs.count_data)).all() and (hs.count_data >= 0).all()


def test_build_and_add_hspike_layout_and_rules(monkeypatch):
    from infercnv_amd.hidden_spike import build_and_add_hspike
    P = Patched(monkeypatch)
    obj = small_object()
    out = build_and_add_hspike(obj, seed=3)
    assert out is not obj and obj.hspike is None and out.expr_data is obj.expr_data
    hs = out.hspike
    check_layout(hs, ["normA", "normB"])
    # tables over c(observation groups, reference groups); the normals are the reference groups
    assert [g.tolist() for g in P.table_groups] == [list(range(50, 75)), list(range(75, 90)), list(range(0, 20)), list(range(20, 50))]
    assert [g.tolist() for g in P.mean_groups] == [list(range(0, 20)), list(range(20, 50))]
    # one simulation call: normal and spiked means per type, in cell order; tokens from the name prefixes
    use = hr.genes_use_idx(60, 4400, 3)
    assert use.min() >= 0 and use.max() < 60 and len(set(use.tolist())) > 30
    cnv = np.repeat([c for _, c in hmm.HSPIKE_CHR_INFO], 400).astype(np.float64)
    m = hr.group_gene_tables(obj.expr_data, [np.arange(0, 20), np.arange(20, 50)])[0]
    assert m[0, 5] == 0.0 and (use == 5).any()
    want = []
    for k in range(2):
        gm = m[k][use].copy()
        gm[gm == 0] = 1e-3                                           # the 1e-3 rule
        want += [gm, gm * cnv]
    assert P.sim["means"].shape == (4, 4400) and np.array_equal(P.sim["means"], np.vstack(want))
    assert (P.sim["means"][0][use == 5] == 1e-3).all() and (P.sim["means"][1][(use == 5) & (cnv == 3)] == 3e-3).all()
    assert P.sim["tokens"] == [hr.fnv1a64(n) for n in ("simnorm_cell_normA", "spike_tumor_cell_normA", "simnorm_cell_normB", "spike_tumor_cell_normB")]
    assert P.sim["num_cells"] == 100 and P.sim["seed"] == 3
    # the splines come from the tables, once
    rm, rv, rn = hr.group_gene_tables(obj.expr_data, P.table_groups)
    n = np.array([25, 15, 20, 30], dtype=np.float64)[:, None]
    fv = ss.smooth_spline(np.log(rm.ravel() + 1), np.log(rv.ravel() + 1))
    pos = rm.ravel() > 0
    fp = ss.smooth_spline(np.log(rm.ravel()[pos]), (rn / n).ravel()[pos])
    assert np.array_equal(P.sim["var"].coef, fv.coef) and np.array_equal(P.sim["p0"].coef, fp.coef)
    assert np.array_equal(P.sim["var"].knots, fv.knots) and np.array_equal(P.sim["p0"].knots, fp.knots)
    # the whole object against the restated build
    r_counts, r_norm, r_chrs, r_refs, r_obs, r_names = hr.build_hspike(obj.expr_data, obj.reference_grouped_cell_indices,
                                                                       obj.observation_grouped_cell_indices,
                                                                       (fv.knots, fv.coef, fv.xmin, fv.range), (fp.knots, fp.coef, fp.xmin, fp.range), seed=3)
    assert np.array_equal(hs.count_data, r_counts) and list(hs.cell_names) == r_names
    # normalised to the median column sum of the LAST normal type's cells
    assert np.array_equal(P.colsum_rows, obj.expr_data[:, 20:50].T)
    assert P.factor == float(np.median(obj.expr_data[:, 20:50].sum(axis=0)))
    assert np.allclose(hs.expr_data, r_norm, rtol=1e-12, atol=0, equal_nan=True)
    assert build_and_add_hspike(obj, seed=3).hspike.count_data.tobytes() == hs.count_data.tobytes()
    assert (build_and_add_hspike(obj, seed=4).hspike.count_data != hs.count_data).any()


def test_build_and_add_hspike_group_handling(monkeypatch):
    from infercnv_amd.hidden_spike import build_and_add_hspike
    P = Patched(monkeypatch)
    obj = small_object()
    hs = build_and_add_hspike(obj, aggregate_normals=True).hspike       # merges the normals, not the tables
    check_layout(hs, ["normalsToUse"])
    assert [g.tolist() for g in P.table_groups] == [list(range(50, 75)), list(range(75, 90)), list(range(0, 20)), list(range(20, 50))]
    assert [g.tolist() for g in P.mean_groups] == [list(range(0, 50))]
    assert P.factor == float(np.median(obj.expr_data[:, 0:50].sum(axis=0)))
    bare = small_object(with_refs=False)                                # reference-less: all observation cells, for both
    hs = build_and_add_hspike(bare).hspike
    check_layout(hs, ["normalsToUse"])
    assert [g.tolist() for g in P.table_groups] == [list(range(0, 90))] and [g.tolist() for g in P.mean_groups] == [list(range(0, 90))]
    assert P.factor == float(np.median(bare.expr_data.sum(axis=0)))
    for method in ("simple", "splatter"):
        with pytest.raises(NotImplementedError):
            build_and_add_hspike(obj, sim_method=method)
    with pytest.raises(ValueError):
        build_and_add_hspike(obj, sim_method="other")
    lone = small_object()
    lone.observation_grouped_cell_indices = {"tumA": np.arange(50, 89), "tumB": np.array([89])}
    with pytest.raises(ValueError):                                     # a one-cell group: NaN variances, R stops in smooth.spline
        build_and_add_hspike(lone)
