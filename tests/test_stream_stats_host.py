"""tests/stream_stats_restate.py against what the project already trusts (oracle_np, oracle_c), and its builders against
what tests/test_gpu_stream_stats.py assumes of them.  CPU only: runs on a machine without a GPU.

Tolerances: equality wherever the arithmetic is integer, dyadic or the same IEEE operations in the same order; otherwise the
bound derived in stream_stats_restate (sum_bound, sd_bound, 1 ulp for a rational rounded twice) or the project's 1e-12.
"""
import math

import numpy as np
import pytest

import oracle_c as oc
import oracle_np as onp
import stream_stats_restate as ss


def small_counts():
    x, info = ss.count_matrix(40, 9, seed=1)
    x = np.minimum(x, 5000)                        # (the oracle sums doubles: keep the tie to it about the arithmetic, not the width)
    return x, info


def test_normalize_and_log2_match_the_oracle_bit_for_bit():
    x, info = small_counts()
    kept = x[info["keep"]]
    cs = ss.col_sums_int(x, info["keep"])
    f = ss.r_median(cs)
    got = ss.apply_counts(kept, cs, f, True, False)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = onp.normalize_counts_by_seq_depth(kept)
        want_log = onp.log2xplus1(want)
    assert np.isnan(got[:, info["c_zero"]]).all()                               # 0 / 0 * f
    assert np.array_equal(got, want, equal_nan=True)                            # equality: the same IEEE operations in the same order
    assert np.array_equal(ss.apply_counts(kept, cs, f, True, True), want_log, equal_nan=True)   # equality, likewise
    assert np.array_equal(ss.apply_counts(kept, cs, f, False, False), kept.astype(np.float64))  # equality: a conversion


def test_median_both_parities():
    assert ss.r_median([3.0, 1.0, 2.0]) == 2.0 and ss.r_median([4.0, 1.0, 3.0, 2.0]) == 2.5 and math.isnan(ss.r_median([]))
    rng = np.random.default_rng(5)
    for n in (1, 2, 9, 10):
        v = rng.integers(0, 1000, n).astype(np.float64)
        assert ss.r_median(v) == float(onp.r_median(v, axis=0))                 # equality: a selection and one exact halving


def test_gene_filters_match_the_oracle():
    x, _ = small_counts()
    sums, pos = ss.gene_stats_int(x)
    C = x.shape[1]
    xf = x.astype(np.float64)
    for cutoff in (0.3, 1.0, 2.5):
        assert ss.mean_gap(sums, C, cutoff) > 1e-9                              # no gene sits on the cutoff
        removed = onp.below_min_mean_expr_cutoff(xf, cutoff)
        kept = ss.select_genes(sums, pos, C, cutoff, 0)
        assert sorted(set(range(x.shape[0])) - set(kept.tolist())) == removed.tolist() and 0 < kept.size < x.shape[0]
    for n in (1, 2, 4):
        assert ss.select_genes(sums, pos, C, None, n).tolist() == onp.genes_passing_min_cells(xf, n).tolist()
    both = ss.select_genes(sums, pos, C, 0.3, 2)
    assert set(both.tolist()) == set(ss.select_genes(sums, pos, C, 0.3, 0).tolist()) & set(ss.select_genes(sums, pos, C, None, 2).tolist())


def test_positive_counts_edge_values():
    x = np.array([[np.nan, -0.0, -1.0, np.inf, 5e-324, 0.0, 1.0]])
    assert ss.positive_counts(x) == [3]                                         # +Inf, the denormal and 1.0
    assert onp.genes_passing_min_cells(x, 3).tolist() == [0] and onp.genes_passing_min_cells(x, 4).tolist() == []


@pytest.mark.parametrize("shape", ss.SCALE_SHAPES)
def test_scale_rows_matches_the_oracle_and_exempts_only_the_planted_genes(shape):
    G, C = shape
    const = ss.SCALE_CONSTANT[shape]
    x = ss.scale_input(G, C, seed=G, constant=const)
    got = ss.scale_rows(x)
    want = onp.scale_rows(x)
    nan_rows = np.isnan(got).all(axis=1)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).any(axis=1).tolist() == nan_rows.tolist()
    assert np.nonzero(nan_rows)[0].tolist() == sorted(const)                    # nothing but the planted constants is exempt
    ok = ~nan_rows
    if ok.any():
        assert x[ok].std(axis=1, ddof=1).min() > 1e-3                           # ... and no gene's scale is near 0
        assert np.abs(got[ok] - want[ok]).max() < 1e-12                         # the project's existing 1e-12


def test_scale_rows_single_cell_and_exact_triple():
    assert np.isnan(ss.scale_rows(ss.scale_input(7, 1))).all()                  # C = 1: 0 / sqrt(0 / 1)
    assert np.isnan(onp.scale_rows(ss.scale_input(7, 1))).all()
    m, d = np.arange(3, 13, dtype=np.float64), np.arange(1, 11, dtype=np.float64)
    x = np.stack([m - d, m, m + d], axis=1)
    assert np.array_equal(ss.scale_rows(x), np.tile([-1.0, 0.0, 1.0], (10, 1)))  # equality: mean m, sum of squares 2 d^2, scale d -- all exact
    assert np.array_equal(onp.scale_rows(x), ss.scale_rows(x))


def test_average_bounds_exact_on_dyadic_values_and_na_rm():
    for G, C in ((1, 1), (5, 8), (257, 16), (3, 1024)):
        x = ss.dyadic(G, C, seed=G)
        assert ss.average_bounds(x) == tuple(onp.get_average_bounds(x)) == tuple(oc.get_average_bounds(x))   # equality: exact means
    x = ss.dyadic(6, 4)
    y = x.copy()
    y[0, 1] = y[3, 1] = y[5, 2] = np.nan
    want = (np.mean([np.nanmin(y[:, c]) for c in range(4)]), np.mean([np.nanmax(y[:, c]) for c in range(4)]))
    assert ss.average_bounds(y) == want                                         # na.rm = TRUE: NaN entries are skipped
    y[:, 3] = np.nan
    assert all(math.isnan(v) for v in ss.average_bounds(y))                     # a cell of nothing but NaN: NA for both bounds


def test_remove_outliers_and_proxy_tables():
    x = np.array([[-3.0, -0.0, 0.0, np.nan, 2.0, 0.5]])
    got = ss.remove_outliers(x, 0.0, 1.0)
    assert np.array_equal(ss.bits(got), ss.bits(np.array([[0.0, -0.0, 0.0, np.nan, 1.0, 0.5]])))
    assert np.array_equal(got, onp.remove_outliers_norm(x, lower_bound=0.0, upper_bound=1.0), equal_nan=True)
    st = np.arange(256, dtype=np.uint8)
    p6, p3 = ss.states_to_proxy(st, 6), ss.states_to_proxy(st, 3)
    assert p6[1:7].tolist() == [0.0, 0.5, 1.0, 1.5, 2.0, 3.0] and np.isnan(p6[[0, 7, 255]]).all() and np.isnan(p6).sum() == 250
    assert p3[1:4].tolist() == [0.5, 1.0, 1.5] and np.isnan(p3[[0, 4, 5, 6, 7, 255]]).all() and np.isnan(p3).sum() == 253


def test_exact_mean_sd_matches_the_oracles_within_the_derived_bounds():
    x = ss.grid_values((300, 9), seed=3)
    genes, cells = ss.gene_list(257, seed=1) % 300, np.array(ss.LIST_CELLS)
    vals = x[np.ix_(genes, cells)].ravel(order="F")
    mean, sd = ss.exact_mean_sd(vals.tolist(), 24)
    omean, osd = onp.gene_expr_mean_sd(x, genes, cells)
    assert ss.ulp_distance(mean, omean) <= 1                                    # derived: an exact sum, one long-double division rounded twice
    assert abs(osd - sd) <= ss.sd_bound(vals.size) * sd                         # derived: sd_bound
    cells = np.array(ss.MOMENTS_CELLS)
    mean, sd = ss.exact_mean_sd(x[:, cells].ravel(order="F").tolist(), 24)
    cmean, csd = oc.mean_sd_of_cells(x, cells)
    assert ss.ulp_distance(mean, cmean) <= 1 and abs(csd - sd) <= ss.sd_bound(300 * cells.size) * sd
    assert math.isnan(ss.exact_mean_sd([1.5], 1)[1])                            # sd() of one value is NA
    xi = ss.moments_matrix(257)
    m = 11
    assert ss.int_moments(xi, cells) == int(xi[:, cells].sum())                 # equality: integers below 2^53
    assert ss.int_moments(xi, cells, m) == int(((xi[:, cells] - m) ** 2).sum())


def test_helpers():
    assert ss.ulp_distance(1.0, np.nextafter(1.0, 2.0)) == 1 and ss.ulp_distance(-0.0, 0.0) == 0
    assert ss.ulp_distance(-5e-324, 5e-324) == 2 and ss.ulp_distance(math.nan, math.nan) == 0 and ss.ulp_distance(1.0, math.nan) > 2 ** 60
    a = np.array([1.0, -1.0, 0.0]); b = np.nextafter(a, 9.0)
    assert ss.ulp_distance_array(a, b).tolist() == [1, 1, 1]
    x = np.random.default_rng(0).lognormal(size=1000)
    assert abs(float(np.sum(x)) - math.fsum(x)) <= ss.sum_bound(x.size, math.fsum(np.abs(x)))
    assert abs(float(np.cumsum(x)[-1]) - math.fsum(x)) <= ss.sum_bound(x.size, math.fsum(np.abs(x)))
    assert not np.array_equal(ss.bits(np.array([0.0])), ss.bits(np.array([-0.0])))


# ------------------------------------------------------------------ the builders
@pytest.mark.parametrize("shape", ss.INGEST_SHAPES + (ss.INGEST_CSC_WRAP,))
def test_count_matrix_has_what_the_issue_plants(shape):
    G, C = shape
    x, info = ss.count_matrix(G, C, seed=G)
    keep, kept = info["keep"], np.nonzero(info["keep"])[0]
    assert x.dtype == np.int32 and x.min() >= 0 and ss.partial_sums_below_2_53(x)
    if G * C > 2000:
        assert 0.85 < (x == 0).mean() < 0.95
    if G >= 8:
        assert not keep[0] and not keep[-1] and not keep[G // 2] and keep[1] and keep[G - 2] and keep.sum() < G - 2
    sums, pos = ss.gene_stats_int(x)
    assert keep[info["g_big"]] and (x[info["g_big"]] == ss.INT32_MAX).sum() >= min(5, C - (C >= 4))
    if C >= 3:
        assert sums[info["g_big"]] > 2 ** 32                                     # a 32-bit gene accumulator wraps
    n_big = int((x[kept, info["c_big"]] == ss.INT32_MAX).sum())
    assert n_big >= min(3, kept.size)
    cs = ss.col_sums_int(x, keep)
    if kept.size >= 3:
        assert cs[info["c_big"]] > 2 ** 32                                       # ... and so does a 32-bit column accumulator
    if info["c_zero"] is not None:
        assert cs[info["c_zero"]] == 0 and (G < 2 or x[~keep, info["c_zero"]].sum() > 0)
    assert all(isinstance(s, int) for s in sums) and sums == x.astype(np.int64).sum(axis=1).tolist()
    assert pos == (x > 0).sum(axis=1).tolist()


@pytest.mark.parametrize("shape", ((257, 5), (300, 1030)))
def test_dense_to_csc_round_trips_shuffled_with_explicit_zeros(shape):
    x, _ = ss.count_matrix(*shape, seed=shape[0])
    colptr, rowidx, vals = ss.dense_to_csc(x, seed=shape[0])
    assert colptr.dtype == np.int64 and rowidx.dtype == np.int32 and vals.dtype == np.int32
    assert colptr[0] == 0 and colptr[-1] == rowidx.size == vals.size and (np.diff(colptr) >= 0).all()
    assert np.array_equal(ss.csc_to_dense(colptr, rowidx, vals, x.shape[0]), x)
    assert (vals == 0).sum() > 0
    unsorted = 0
    for c in range(x.shape[1]):
        r = rowidx[colptr[c]:colptr[c + 1]]
        assert np.unique(r).size == r.size                                       # each (gene, cell) at most once
        unsorted += r.size >= 2 and not (np.diff(r) > 0).all()
    assert unsorted > 0


def test_csc_layouts_have_every_column_length_unsorted_with_zeros():
    seen = set()
    for C, kinds in ss.CSC_CASES.items():
        colptr, rowidx, vals, keep = ss.csc_layout(C)
        assert len(colptr) == C + 1 == len(kinds) + 1 and colptr[-1] == rowidx.size == vals.size
        assert vals.min() >= 0 and rowidx.min() >= 0 and rowidx.max() < ss.CSC_G
        for c, kind in enumerate(kinds):
            r, v = rowidx[colptr[c]:colptr[c + 1]], vals[colptr[c]:colptr[c + 1]]
            assert np.unique(r).size == r.size                                   # each (gene, cell) at most once
            if r.size >= 2:
                assert not (np.diff(r) > 0).all()                                # unsorted
            if kind == "dropped":
                assert r.size > 0 and not keep[r].any() and (v > 0).all()        # stored entries, none in a kept gene
            else:
                assert r.size == kind
                seen.add(kind)
                if kind >= 2:
                    assert (v == 0).any() and (v > 0).any()                      # explicit zeros among real counts
        x = ss.csc_to_dense(colptr, rowidx, vals, ss.CSC_G)
        assert ss.partial_sums_below_2_53(x) and int(x.sum()) == int(vals.sum())
    assert seen == set(ss.CSC_LENGTHS)
    assert sorted(C % 4 for C in ss.CSC_CASES) == [1, 1, 2, 3, 3] and sum(C < 4 for C in ss.CSC_CASES) == 3


def test_float_builders():
    x = ss.position_coded(257, 1030)
    assert np.unique(x).size == x.size and x.max() < 2 ** 53 / 2 ** 20 and x.sum() < 2 ** 53
    d = ss.dyadic(3, 16384)
    assert np.array_equal(d * 2 ** 20, np.round(d * 2 ** 20)) and np.abs(d).max() < 2 ** 10
    g = ss.grid_values((10001, 9))
    assert np.array_equal(g * 2 ** 24, np.round(g * 2 ** 24)) and not np.array_equal(g, np.round(g)) and g.min() > 0
    for G in ss.MOMENTS_G:
        m = ss.moments_matrix(G, seed=G)
        assert np.abs(m).max() <= 2 ** 15 and np.array_equal(m, np.round(m))
        assert len(ss.MOMENTS_CELLS) * G * (2 ** 15 + 2 ** 15) ** 2 < 2 ** 53      # sums of squared deviations from |mean| <= 2^15 stay exact
    assert len(ss.MOMENTS_CELLS) == 7 and len(set(ss.MOMENTS_CELLS)) == 6 and list(ss.MOMENTS_CELLS) != sorted(ss.MOMENTS_CELLS)
    assert {c % 2 for c in ss.MOMENTS_CELLS} == {0, 1} and max(ss.MOMENTS_CELLS) < 9
    for n in ss.LIST_N_GENES:
        idx = ss.gene_list(n, seed=n)
        assert idx.size == n and idx.min() >= 0 and idx.max() < ss.LIST_G
        if n >= 2:
            assert np.unique(idx).size < n                                       # a repeat
        if n >= 3:
            assert not (np.diff(idx) >= 0).all()                                 # unsorted
