"""tests/group_hmm_restate.py against references it does not share code with (numpy long double, math.fsum, the statistics
module, the oracles), and its builders against what tests/test_gpu_group_hmm.py assumes of them.  CPU only.

Tolerances: equality for anything exact or table-like; one ulp where a long-double mean is rounded twice; for the statistics
module, whose fmean / stdev are correctly rounded from exact rationals, equality of the mean and one ulp of the sd.
"""
import math
import statistics
from fractions import Fraction

import numpy as np
import pytest

import oracle_c as oc
import oracle_np as onp
import group_hmm_restate as gh


def ulps(a, b):
    ia, ib = (int(np.float64(v).view(np.int64)) for v in (a, b))
    return abs(ia - ib)


def test_exact_sum_is_the_fraction_sum_and_rounds_like_fsum():
    rng = np.random.default_rng(1)
    for v in (rng.standard_normal(50), 10.0 ** rng.uniform(-300, 300, 40) * rng.choice([-1, 1], 40), np.array([5e-324, -1e308, 1e308, 0.0]),
              np.zeros(0)):
        want = sum((Fraction(t) for t in v.tolist()), Fraction(0))
        assert gh.exact_sum(v) == want                                          # equality: both exact
        assert float(gh.exact_sum(v)) == math.fsum(v.tolist())                  # equality: fsum is the correctly rounded sum


def test_exact_group_means_against_long_double_row_means():
    assert np.finfo(np.longdouble).nmant >= 63
    rng = np.random.default_rng(2)
    x = 1.0 + 0.1 * rng.standard_normal((40, 30))
    groups = [np.arange(0, 7), np.arange(7, 8), np.arange(8, 30), np.array([3, 29, 11, 0])]
    got = gh.exact_group_means(x, groups)
    for q, cells in enumerate(groups):
        want = (x[:, cells].astype(np.longdouble).sum(axis=1) / np.longdouble(len(cells))).astype(np.float64)
        assert max(ulps(a, b) for a, b in zip(got[:, q], want)) <= 1            # one ulp: a 64-bit sum and quotient rounded again to 53
    assert np.array_equal(got[:, 1], x[:, 7])                                   # a group of one cell: the cell


def test_exact_group_means_cancelling_column():
    x = np.array([[1e16, 1.0, -1e16, 3.0]])
    assert gh.exact_group_means(x, [np.arange(4)])[0, 0] == 1.0                 # (1 + 3) / 4; plain summation left to right gives 0.75
    assert gh.cancellation_ratio(x[0]) == 2e16 / 4 + 1.0
    assert gh.cancellation_ratio([1.0, -1.0]) == math.inf


def test_non_finite_rules_are_numpy_means():
    inf, nan = math.inf, math.nan
    rows = [[1.0, inf, 2.0], [1.0, -inf, 2.0], [inf, -inf, 1.0], [nan, 1.0, 2.0], [nan, inf, 1.0], [-inf, -inf, 5.0], [inf], [nan, -inf, inf]]
    for row in rows:
        got = gh.exact_group_means(np.array([row]), [np.arange(len(row))])[0, 0]
        with np.errstate(invalid="ignore"):
            want = float(np.mean(np.array(row)))
        assert (math.isnan(got) and math.isnan(want)) or got == want, (row, got, want)
    x = np.array([[1.0, inf, 2.0, 4.0]])
    assert np.array_equal(gh.exact_group_means(x, [np.array([0, 2, 3]), np.array([1, 0])])[0], [7.0 / 3.0, inf])


def test_rounding_margin_and_needed_margin():
    one_up = math.nextafter(1.0, 2.0)
    assert gh.rounding_margin(Fraction(1)) == 2.0 ** -54                        # next midpoint below 1: 1 - 2^-54
    assert gh.rounding_margin((Fraction(1) + Fraction(one_up)) / 2) == 0.0      # a tie
    third = Fraction(1, 3)
    m = gh.rounding_margin(third)
    err = float(abs(third - Fraction(float(third))))
    assert err + m / 3.0 == pytest.approx(2.0 ** -55, rel=1e-12)                # rounding error + distance to the midpoint = half an ulp, ulp(1/3) = 2^-54
    assert gh.dd_margin_needed(129, 1.0) < 2.0 ** -89 and gh.dd_margin_needed(129, 2.0 ** 30) < 2.0 ** -59


def test_moments_and_i3_params_against_the_statistics_module():
    rng = np.random.default_rng(3)
    for x in (gh.integer_matrix(7, 12, seed=4), 1.0 + 0.1 * rng.standard_normal((7, 12))):
        ref = np.array([0, 5, 11, 3])
        S1, S2, n, A1, A2 = gh.exact_moments(x, ref)
        vals = x[:, ref].ravel(order="F").tolist()
        assert n == len(vals) == 28
        assert S1 == sum(Fraction(v) - 1 for v in vals) and S2 == sum((Fraction(v) - 1) ** 2 for v in vals) and A2 == float(S2)
        assert A1 == pytest.approx(sum(abs(v - 1.0) for v in vals), rel=1e-14)
        z = 1.6448536269514722
        mu, sigma, delta, means = gh.i3_params(S1, S2, n, z)
        assert mu == statistics.fmean(vals)                                     # equality: fmean rounds the exact mean once
        assert ulps(sigma, statistics.stdev(vals)) <= 1                         # stdev: exact variance, one rounded square root
        assert ulps(delta, sigma * z) <= 1 and means[1] == mu
        assert ulps(means[0], mu - delta) <= 1 and ulps(means[2], mu + delta) <= 1
        mu2, sigma2, delta2, means2 = gh.i3_params(S1, S2, n, z, delta_abs=0.07)
        assert (mu2, sigma2, delta2) == (mu, sigma, 0.07) and ulps(means2[2], mu + 0.07) <= 1
        kappa = gh.sigma_condition(S1, S2, n)
        assert kappa == pytest.approx(float(S2) / (float(S2) - float(S1) ** 2 / n), rel=1e-12) and kappa >= 1.0


def test_integer_matrix_keeps_the_moments_exact():
    x = gh.integer_matrix(512, 700, seed=5)
    assert x.min() == -3 and x.max() == 6 and np.array_equal(x, np.rint(x))
    assert 700 * 512 * 25 < 2 ** 53                                            # the largest S2 a test can reach: (x - 1)^2 <= 25


def test_consensus_against_the_oracle_and_hand_built_ties():
    rng = np.random.default_rng(6)
    st = rng.integers(1, 7, size=(30, 40)).astype(np.uint8)
    st[rng.random(st.shape) < 0.2] = 255
    groups = [np.arange(0, 13), np.arange(13, 14), np.arange(14, 40), np.array([2, 39])]
    signed = st.astype(np.int64)
    signed[st == 255] = -1
    want = onp.state_consensus(signed, groups)
    got = gh.consensus(st, groups).astype(np.int64)
    got[got == 255] = -1
    assert np.array_equal(got, want)
    rows = {(255, 255, 255): 255, (255, 1, 1, 255): 255, (4, 3, 3, 4): 3, (6, 5, 4, 3, 2, 1): 1, (5,): 5, (6, 6, 1, 6, 2): 6, (2, 255, 2): 2,
            (1, 6, 6, 255): 6}
    for row, winner in rows.items():
        assert gh.consensus(np.array([row], dtype=np.uint8), [np.arange(len(row))])[0, 0] == winner, row


def test_proxy_against_the_oracles():
    st6 = np.arange(1, 7, dtype=np.uint8).reshape(2, 3)
    assert np.array_equal(gh.proxy(st6, 6), onp.assign_HMM_states_to_proxy_expr_vals(st6))
    assert np.array_equal(gh.proxy(st6, 6), oc.states_to_proxy(st6, 6))
    st3 = np.array([[1, 2, 3]], dtype=np.uint8)
    assert np.array_equal(gh.proxy(st3, 3), oc.states_to_proxy(st3, 3)) and gh.proxy(st3, 3).tolist() == [[0.5, 1.0, 1.5]]
    odd = np.array([[0, 7, 255, 4, 5, 6]], dtype=np.uint8)
    assert np.isnan(gh.proxy(odd, 3)).all() and np.isnan(gh.proxy(odd, 6)[0, :3]).all() and gh.proxy(odd, 6)[0, 3:].tolist() == [1.5, 2.0, 3.0]


def test_nsplit_values_the_gpu_tests_rely_on():
    assert [gh.nsplit(G, 7) for G in (1, 255, 256, 257, 513)] == [64] * 5
    assert gh.nsplit(1, 2048) == 1 and gh.nsplit(1, 2047) == 2 and gh.nsplit(257, 1024) == 1 and gh.nsplit(513, 683) == 1
    assert gh.nsplit(513, 40) == 18


@pytest.mark.parametrize("G", (1, 257))
def test_means_matrix_meets_its_two_conditions(G):
    groups, rest = gh.mean_groups(seed=G)
    assert sorted(len(g) for g in groups) == sorted(gh.MEAN_SIZES) and rest.size == 0
    C = sum(gh.MEAN_SIZES)
    x = gh.means_matrix(G, groups, C, seed=G)
    assert np.isfinite(x).all()
    worst, ties = 0.0, 0
    for g in range(G):
        for cells in groups:
            ratio = gh.cancellation_ratio(x[g, cells])
            worst = max(worst, ratio)
            assert ratio < gh.RATIO_CAP == 2.0 ** 40
            margin = gh.rounding_margin(gh.exact_sum(x[g, cells]) / len(cells))
            assert len(cells) <= 2 or margin > gh.dd_margin_needed(len(cells), ratio)
            ties += margin == 0.0
    if G > 2:
        assert worst > 2.0 ** 30 and np.abs(x).max() == 1e15                    # the planted pairs are there
        assert ties > 20                                                        # means of two cells that are exact ties (round half to even)
