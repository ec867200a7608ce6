"""CPU tests of the window tables of step 10's "runmeans" and "coordinates" smoothers (infercnv_amd/smooth_windows.py, DESIGN
K16): the sequential restatement of tests/smooth_windows_restate.py against K10's restated running mean, the builders' tables
against the restatement bit for bit -- on inputs that are asserted to reach the reference's corners -- and the restatement
against exact rational arithmetic within the forward error bound of a sequential dot product."""
import logging
from fractions import Fraction

import numpy as np
import pytest

import oracle_np as onp
import random_trees_restate as rtr
import smooth_windows_restate as swr
from infercnv_amd import smooth_windows as sw


def same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    bad = a.view(np.uint64) != b.view(np.uint64)
    assert not bad.any(), f"{int(bad.sum())} differ, first at {np.argwhere(bad)[0]}: {a[bad][0]!r} vs {b[bad][0]!r}"


@pytest.mark.parametrize("n,k", [(2, 101), (100, 101), (101, 101), (257, 100), (300, 7)])
def test_restated_runmean_equals_k10_restatement(n, k):
    X = np.random.default_rng(n * 1000 + k).normal(0.0, 0.4, size=(n, 5))
    same(swr.runmean_chr(X, k), rtr.runmean(X, k))
    same(sw.apply_windows_host(X, sw.runmeans_windows([0, n], k)), rtr.runmean(X, k))


def test_runmeans_table_per_chromosome():
    cs = [0, 1, 3, 6, 106, 107, 364]
    X = np.random.default_rng(3).normal(size=(364, 3))
    for k in (1, 2, 7, 100, 101, 1000):
        tab = sw.runmeans_windows(cs, k)
        assert tab.w is None and tab.G == 364
        for a, b in zip(cs[:-1], cs[1:]):                      # a window never leaves its chromosome
            assert (tab.lo[a:b] >= a).all() and (tab.lo[a:b] + tab.len[a:b] <= b).all()
        same(sw.apply_windows_host(X, tab), swr.runmeans(X, cs, k))
    same(sw.apply_windows_host(X, sw.runmeans_windows(cs, 1)), X)


EXPECTED_CORNERS = {101: "all_fallback", 5e4: "noncontiguous", 3e5: "noncontiguous", 1e7: "contiguous"}


@pytest.mark.parametrize("w", [101, 5e4, 3e5, 1e7])
def test_coordinate_tables_equal_the_restatement_and_reach_the_corners(w, caplog):
    start, stop = swr.layout60()
    X = np.random.default_rng(61).normal(0.0, 0.4, size=(60, 4))
    info = {}
    want = swr.coordinates(X, [0, 60], start, stop, w, info)
    with caplog.at_level(logging.WARNING, logger="infercnv_amd"):
        tab = sw.coordinate_windows([0, 60], start, stop, w)
    same(sw.apply_windows_host(X, tab), want)
    fallback, nonc = info.get("fallback", 0), info.get("noncontiguous", 0)
    print(f"w = {w:g}: {fallback} fallbacks, {nonc} non-contiguous index sets")
    warned = [r for r in caplog.records if "non-contiguous" in r.getMessage()]
    if EXPECTED_CORNERS[w] == "all_fallback":
        assert fallback == 60
    elif EXPECTED_CORNERS[w] == "noncontiguous":
        assert nonc >= 1
        assert len(warned) == 1 and warned[0].args[0] == nonc          # one warning per call, with the count
    else:
        assert nonc == 0 and fallback == 0 and not warned
        assert (tab.lo == 0).all() and (tab.len == 60).all()


def test_hspike_layout_widest_row_is_201():
    pos = np.arange(1, 401, dtype=np.float64)
    tab = sw.coordinate_windows([0, 400], pos, pos, 51)
    assert tab.widest == 201
    assert tab.len[200] == 201 and tab.lo[200] == 100          # 101 genes inside +- 51, 50 more on either side
    X = np.random.default_rng(5).normal(size=(400, 2))
    same(sw.apply_windows_host(X, tab), swr.coordinates(X, [0, 400], pos, pos, 51))


def test_identity_cases():
    start, stop = swr.layout60()
    X = np.random.default_rng(8).normal(size=(63, 3))
    cs = [0, 60, 61, 63]
    s3 = np.concatenate([start, [5.0], [10.0, 900.0]])
    e3 = np.concatenate([stop, [50.0], [700.0, 1500.0]])
    same(sw.apply_windows_host(X, sw.coordinate_windows(cs, s3, e3, 1)), X)           # window_length < 2
    tab = sw.coordinate_windows(cs, s3, e3, 3e5)
    assert tab.lo[60] == 60 and tab.len[60] == 1 and tab.denom[60] == 1.0             # a one-gene chromosome stays
    same(sw.apply_windows_host(X, tab), swr.coordinates(X, cs, s3, e3, 3e5))


def _exact(X, tab, g, c):
    num = sum((Fraction(float(X[int(tab.lo[g]) + t, c])) * (Fraction(float(tab.w[int(tab.w_off[g]) + t])) if tab.w is not None else 1)
               for t in range(int(tab.len[g]))), Fraction(0))
    mag = sum(abs(float(X[int(tab.lo[g]) + t, c]) * (float(tab.w[int(tab.w_off[g]) + t]) if tab.w is not None else 1.0))
              for t in range(int(tab.len[g])))
    return num / Fraction(float(tab.denom[g])), mag / float(tab.denom[g])


def test_restatement_within_the_forward_error_bound_of_exact_arithmetic():
    """|computed - exact| <= (L + 2) 2^-52 sum |w_t x_t| / denom: L - 1 adds and L products of a sequential dot product with
    positive weights, each within 2^-53 relative, and one division (Higham, Accuracy and Stability, section 3.1: gamma_L+1
    <= (L + 2) 2^-53 to first order; the factor 2 of 2^-52 covers the higher-order terms)."""
    start, stop = swr.layout60()
    X = np.random.default_rng(62).normal(0.0, 0.4, size=(60, 3))
    for tab, got in ((sw.coordinate_windows([0, 60], start, stop, 3e5), swr.coordinates(X, [0, 60], start, stop, 3e5)),
                     (sw.coordinate_windows([0, 60], start, stop, 1e7), swr.coordinates(X, [0, 60], start, stop, 1e7)),
                     (sw.runmeans_windows([0, 60], 7), swr.runmeans(X, [0, 60], 7))):
        for g in range(60):
            for c in range(3):
                exact, mag = _exact(X, tab, g, c)
                bound = (int(tab.len[g]) + 2) * 2.0 ** -52 * mag
                assert abs(Fraction(float(got[g, c])) - exact) <= Fraction(bound), (g, c, float(got[g, c]), float(exact), bound)


@pytest.mark.parametrize("sizes,window", [([102, 300, 1500], 101), ([8, 40], 7)])
def test_generic_pyramid_table_close_to_the_oracle(sizes, window):
    cs = np.concatenate([[0], np.cumsum(sizes)])
    X = np.random.default_rng(int(cs[-1])).normal(0.0, 0.1, size=(int(cs[-1]), 3))
    got = sw.apply_windows_host(X, swr.pyramid_windows(cs, window))
    want = np.concatenate([onp.smooth_window(X[a:b], window) for a, b in zip(cs[:-1], cs[1:])])
    err = np.abs(got - want).max()
    print(f"pyramid table vs oracle_np.smooth_window, window {window}: max abs difference {err:.3e}")
    assert err <= 4e-16


def test_builder_argument_validation():
    start, stop = swr.layout60()
    with pytest.raises(ValueError, match="sorted"):
        sw.runmeans_windows([0, 40, 30, 60], 101)
    with pytest.raises(ValueError, match="sorted"):
        sw.coordinate_windows([0, 40, 30, 60], start, stop, 1e5)
    with pytest.raises(ValueError, match="one entry per gene"):
        sw.coordinate_windows([0, 60], start, stop[:59], 1e5)
    with pytest.raises(ValueError, match="one entry per gene"):
        sw.coordinate_windows([0, 61], start, stop, 1e5)


def test_ops_rejects_an_unknown_smooth_method():
    from infercnv_amd import GeneOrder, InfercnvObject, ops
    obj = InfercnvObject(expr_data=np.zeros((4, 3)), gene_order=GeneOrder(chr=np.array(["a"] * 4)),
                         reference_grouped_cell_indices={"n": np.array([0])},
                         observation_grouped_cell_indices={"t": np.array([1, 2])})
    with pytest.raises(ValueError, match="smooth_method"):
        ops.hip_smooth_chain(obj, smooth_method="pyramid")
