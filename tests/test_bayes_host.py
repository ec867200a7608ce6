"""The restatement of the Bayesian region filter (tests/bayes_restate.py, DESIGN K13) held to mathematics, without a GPU.
All seeds are fixed, so every test is deterministic.  Every statistical tolerance is 5 standard errors, the standard error
computed from the EXACT distribution (never from the sampler's own spread)."""
import itertools
import math
import os

import numpy as np
import pytest

import bayes_restate as br

mpmath = pytest.importorskip("mpmath")


def test_philox_restated_against_numpy():
    for seed, tok, w1, w2, w3 in [(0, 5, 3, 7, 0), (2 ** 63 + 5, br.fnv1a64("chr1-region_2"), 12345, 1699, (5 << 40) + (1 << 32) + 3),
                                  (2 ** 64 - 1, 2 ** 64 - 1, 2 ** 31, 0, 7 << 40)]:
        bg = np.random.Philox(key=np.array([seed, tok], dtype=np.uint64), counter=np.array([0, w1, w2, w3], dtype=np.uint64))
        want = np.random.Generator(bg).random(4)
        assert np.array_equal(want, br.philox_scalar(seed, tok, w1, w2, w3, 4))
        assert np.array_equal(want, br.philox_uniforms(seed, tok, [w1, w1 + 1], w2, w3, 4)[0])
    assert br.fnv1a64("") == 0xCBF29CE484222325 and br.fnv1a64("a") == 0xAF63DC4C8601EC8C


def test_cell_step_exact_categorical():
    """One cell step at fixed theta: N cells with the same L row are N independent draws of one categorical."""
    N = 40000
    theta = np.array([0.05, 0.1, 0.3, 0.25, 0.2, 0.1])
    row = np.array([1.0, 0.6, 0.0, 1e-3, 0.4, 0.9])
    eps = br.cell_step(theta, np.tile(row, (N, 1)), seed=3, token=br.fnv1a64("chr7-region_9"), t=11, ch=2)
    p = theta * row / (theta * row).sum()
    got = np.bincount(eps, minlength=6) / N
    se = np.sqrt(p * (1 - p) / N)
    assert got[2] == 0
    for k in (0, 1, 3, 4, 5):
        print(f"state {k}: p {p[k]:.5f} got {got[k]:.5f} ({abs(got[k] - p[k]) / se[k]:.2f} se)")
        assert abs(got[k] - p[k]) <= 5 * se[k]


def test_cell_step_edges():
    theta = np.array([0.2, 0.3, 0.5])
    L = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, 0.0]])
    for t in range(20):                          # one non-zero L: that state whatever the draw; none: state 0
        assert list(br.cell_step(theta, L, 1, 2, t, 0)) == [1, 0, 2, 0]
    assert list(br.cell_step(np.array([0.0, 0.0, 1.0]), np.array([[1.0, 0.5, 0.0]]), 1, 2, 0, 0)) == [1]   # no w > 0: the last L > 0


def beta_moments(a, b):
    """mean, variance and fourth central moment of Beta(a, b) from its raw moments."""
    raw = [1.0]
    for r in range(4):
        raw.append(raw[-1] * (a + r) / (a + b + r))
    m = raw[1]
    var = raw[2] - m * m
    mu4 = raw[4] - 4 * m * raw[3] + 6 * m * m * raw[2] - 3 * m ** 4
    return m, var, mu4


def test_theta_step_exact_dirichlet():
    """One theta step at fixed counts (gamma shapes 1, 2, 1 + 3 000): N independent draws of Dirichlet(1, 2, 3001)."""
    N = 4000
    counts = [0, 1, 3000]
    th = np.array([br.theta_step(counts, seed=9, token=br.fnv1a64("chr2-region_5"), t=t, ch=1) for t in range(N)])
    assert np.abs(th.sum(axis=1) - 1.0).max() < 1e-15
    A = 3004.0
    for k, a in enumerate((1.0, 2.0, 3001.0)):
        m, var, mu4 = beta_moments(a, A - a)
        se_mean = math.sqrt(var / N)
        se_var = math.sqrt((mu4 - var * var * (N - 3) / (N - 1)) / N)
        gm, gv = th[:, k].mean(), th[:, k].var(ddof=1)
        print(f"theta[{k}]: mean {gm:.6g} vs {m:.6g} ({abs(gm - m) / se_mean:.2f} se), var {gv:.6g} vs {var:.6g} "
              f"({abs(gv - var) / se_var:.2f} se)")
        assert abs(gm - m) <= 5 * se_mean
        assert abs(gv - var) <= 5 * se_var


def exact_posterior(L):
    """theta mean / variance and the cell marginals of the mixture's posterior by enumeration of all K^C assignments:
    p(eps | x) ~ prod_c L[c, eps_c] prod_k n_k!, theta | eps ~ Dirichlet(1 + n)."""
    C, K = L.shape
    A = float(K + C)
    Z = 0.0
    m1, m2, cell = np.zeros(K), np.zeros(K), np.zeros((C, K))
    for eps in itertools.product(range(K), repeat=C):
        n = np.bincount(eps, minlength=K)
        w = math.prod(L[c, e] for c, e in enumerate(eps)) * math.prod(math.factorial(int(v)) for v in n)
        Z += w
        m1 += w * (1.0 + n) / A
        m2 += w * (1.0 + n) * (2.0 + n) / (A * (A + 1.0))
        for c, e in enumerate(eps):
            cell[c, e] += w
    m1, m2, cell = m1 / Z, m2 / Z, cell / Z
    return m1, m2 - m1 * m1, cell


@pytest.mark.parametrize("K,C,M", [(6, 5, 150), (3, 4, 300)])
def test_sampler_against_exact_posterior(K, C, M):
    """The whole sampler against the exact posterior.  Likelihoods deliberately ambiguous.  Only the LAST theta and eps of
    each chain of M independent seeds after 30 iterations are used, so the N = M K draws are independent."""
    rng = np.random.default_rng(K)
    L = rng.uniform(0.2, 1.0, size=(C, K))
    L /= L.max(axis=1, keepdims=True)
    mean, var, cell = exact_posterior(L)
    thetas, eps = [], []
    for seed in range(M):
        *_, finals = br.sample_region(L, br.fnv1a64("chr3-region_4"), K, 20, 9, 1, seed=1000 + seed, final_state=True)
        for th, e in finals:
            thetas.append(th)
            eps.append(e)
    thetas, eps = np.array(thetas), np.array(eps)
    N = M * K
    worst_t = np.abs(thetas.mean(axis=0) - mean) / np.sqrt(var / N)
    got_cell = np.stack([(eps == k).mean(axis=0) for k in range(K)], axis=1)
    worst_c = np.abs(got_cell - cell) / np.sqrt(cell * (1 - cell) / N)
    print(f"K {K} C {C} N {N}: theta within {worst_t.max():.2f} se, cell marginals within {worst_c.max():.2f} se")
    assert worst_t.max() <= 5
    assert worst_c.max() <= 5


def fixture_regions(golden_dir):
    cg = np.load(os.path.join(golden_dir, "mcmc_cell_gene.npz"))
    return [(str(n), cg[f"genes_{i}"].astype(np.int64) - 1, cg[f"cells_{i}"].astype(np.int64) - 1) for i, n in enumerate(cg["names"])]


def test_loglik_against_mpmath(golden_dir):
    """The likelihood matrix of the fixture's nine regions: ll to 1e-12 relative of the exact value of the formula on the
    stored doubles; L to 1e-12 relative of exp of the restated difference."""
    mpmath.mp.dps = 50
    expr = np.load(os.path.join(golden_dir, "infercnv_object_example.npz"))["expr_data"]
    hs = np.load(os.path.join(golden_dir, "hmm_states_example.npz"))
    mu, tau = hs["mu"], hs["sig"]
    regs = fixture_regions(golden_dir)
    ll, L = br.loglik(expr, [(g, c) for _, g, c in regs], mu, tau)
    row, worst, worst_L = 0, 0.0, 0.0
    for _, genes, cells in regs:
        for c in cells:
            for k in range(6):
                ssq = mpmath.fsum((mpmath.mpf(float(expr[g, c])) - mpmath.mpf(float(mu[k]))) ** 2 for g in genes)
                want = mpmath.mpf(len(genes)) / 2 * mpmath.log(mpmath.mpf(float(tau[k]))) - mpmath.mpf(float(tau[k])) / 2 * ssq
                worst = max(worst, float(abs(mpmath.mpf(float(ll[row, k])) - want) / abs(want)))
                d = float(ll[row, k]) - float(ll[row].max())
                if d >= -708.0:
                    wl = mpmath.exp(mpmath.mpf(d))
                    worst_L = max(worst_L, float(abs(mpmath.mpf(float(L[row, k])) - wl) / wl))
                else:
                    assert L[row, k] == 0.0
            assert L[row].max() == 1.0
            row += 1
    print(f"ll worst relative error {worst:.3g}, L {worst_L:.3g}")
    assert worst <= 1e-12 and worst_L <= 1e-12


def test_stored_run_is_the_dirichlet_posterior_mean(golden_dir):
    """The reference's stored run (data/mcmc_obj.rda -> mcmc_probabilities.npz): its theta means equal
    (1 + sum_c cell_probabilities[k, c]) / (K + |Cells|), the mean of Dirichlet(1 + n) averaged over its own eps samples, up
    to Monte-Carlo error: 5 sqrt(p (1 - p) / 17 / 6000) per entry (the Dirichlet's variance at K + C = 16, 6 000 samples).
    This pins the reading of the model and the fixture, not the kernels."""
    z = np.load(os.path.join(golden_dir, "mcmc_probabilities.npz"))
    tm, cp = z["theta_means"], z["cell_probabilities"]
    assert tm.shape == (6, 9) and cp.shape == (9, 6, 10)
    assert np.abs(cp * 6000 - np.rint(cp * 6000)).max() < 1e-9
    pred = ((1.0 + cp.sum(axis=2)) / 16.0).T
    se = np.sqrt(pred * (1 - pred) / 17.0 / 6000.0)
    print(f"worst entry {np.abs(tm - pred).max():.4f}, {(np.abs(tm - pred) / se).max():.2f} se")
    assert (np.abs(tm - pred) <= 5 * se).all()


def test_filter_on_the_stored_probabilities(golden_dir, tmp_path):
    """removeCNV / reassignCNV on the stored probabilities and HMM states with BayesMaxPNormal = 0.5 (the example of
    man/filterHighPNormals.Rd) against the rule itself."""
    from infercnv_amd import bayes_net
    tm = np.load(os.path.join(golden_dir, "mcmc_probabilities.npz"))["theta_means"]
    states = np.load(os.path.join(golden_dir, "hmm_states_example.npz"))["HMM_states"]
    regs = fixture_regions(golden_dir)
    m = bayes_net.MCMCInferCNV(infercnv_obj=None)
    m.cnv_regions = [n for n, _, _ in regs]
    m.cell_gene = [{"cnv_regions": n, "Genes": g, "Cells": c, "State": int(states[g[0], c[0]])} for n, g, c in regs]
    m.cnv_means = tm.copy()
    m.cnv_probabilities = [None] * 9
    m.cell_probabilities = [None] * 9
    m.args = {"HMM_type": "i6", "postMcmcMethod": "removeCNV", "reassignCNVs": True, "out_dir": str(tmp_path)}
    f, new_states = bayes_net.filterHighPNormals(m, states, 0.5)
    want = states.copy()
    for i, (_, g, c) in enumerate(regs):
        want[np.ix_(g, c)] = 3 if tm[2, i] > 0.5 else int(np.argmax(tm[:, i])) + 1
    assert np.array_equal(new_states, want) and (new_states != states).any()
    assert [cg["cnv_regions"] for cg in f.cell_gene] == [n for i, (n, _, _) in enumerate(regs) if not tm[2, i] > 0.5]
    assert len(f.cell_gene) == 8 and len(m.cell_gene) == 9
    lines = open(tmp_path / "CNV_State_Probabilities.dat").read().splitlines()
    assert len(lines) == 7 and len(lines[0].split("\t")) == 8 and lines[3].startswith("State:3\t")
