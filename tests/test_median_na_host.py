"""The NA restatement of the median filter (tests/median_na_restate.py) held to the reference's own loop (CPU, K19).

R/noise_reduction.R:92-113 is a double loop that assigns median(data[posxa:posxb, posya:posyb]); np.median propagates NaN
as R's median() propagates NA, so the literal loop below IS the reference's NA behaviour on a block.  The restatement's
prefix-sum NA set must equal the NaN set of that loop, and its ifelse windows must equal the plain clamp the header states.
"""
import numpy as np
import pytest

import median_na_restate as mr


def literal_median_filter(data, window_size):
    """.median_filter (:92-113), line by line, on one block."""
    half_window = (window_size - 1) // 2
    xdim, ydim = data.shape
    results = data.copy()
    for posx in range(1, xdim + 1):
        posxa = 1 if posx <= (half_window + 1) else posx - (half_window + 1)
        posxb = xdim if posx >= (xdim - (half_window + 1)) else posx + (half_window + 1)
        for posy in range(1, ydim + 1):
            posya = 1 if posy <= (half_window + 1) else posy - (half_window + 1)
            posyb = ydim if posy >= (ydim - (half_window + 1)) else posy + (half_window + 1)
            results[posx - 1, posy - 1] = np.median(data[posxa - 1:posxb, posya - 1:posyb])
    return results


@pytest.mark.parametrize("window_size", [3, 7, 15])
def test_ifelse_windows_equal_the_plain_clamp(window_size):
    for n in range(1, 41):
        a, b = mr.ifelse_windows(n, window_size)
        ca, cb = mr.clamp_windows(n, window_size)
        assert np.array_equal(a, ca) and np.array_equal(b, cb), (n, window_size)
        assert (a >= 1).all() and (b <= n).all() and (a <= np.arange(1, n + 1)).all() and (b >= np.arange(1, n + 1)).all()


@pytest.mark.parametrize("shape", [(1, 5), (12, 9), (23, 20)])
def test_restated_na_set_equals_the_literal_loop(shape):
    rng = np.random.default_rng(sum(shape))
    data = rng.normal(size=shape)
    with np.errstate(invalid="ignore"):
        for window_size in (3, 7, 15):
            for trial in range(3):
                x = data.copy()
                n_nan = (0, 1, 4)[trial]
                flat = rng.choice(x.size, size=min(n_nan, x.size), replace=False)
                x.ravel()[flat] = np.nan
                want = literal_median_filter(x, window_size)
                got_na = mr.block_na(np.isnan(x), window_size)
                assert np.array_equal(got_na, np.isnan(want)), (shape, window_size, trial)
                # ... and where the window is clean the value does not depend on what the NA positions hold
                clean = literal_median_filter(np.where(np.isnan(x), 0.0, x), window_size)
                assert np.array_equal(want[~got_na], clean[~got_na])


def test_na_outputs_walks_blocks_and_leaves_untiled_cells():
    """na_outputs on a layout with two chromosomes and two tiles equals the literal loop block by block; an NA in a cell of no
    tile poisons nothing."""
    rng = np.random.default_rng(7)
    G, C = 14, 13
    chr_start = np.array([0, 5, 14], dtype=np.int32)
    perm = rng.permutation(C)
    tiles = [perm[:6], perm[6:11]]            # perm[11:] in no tile
    x = rng.normal(size=(G, C))
    x[4, perm[2]] = np.nan                    # last gene of chromosome 0
    x[9, perm[8]] = np.nan
    x[7, perm[12]] = np.nan                   # untiled
    want = np.zeros((G, C), dtype=bool)
    with np.errstate(invalid="ignore"):
        for t in tiles:
            for k in range(2):
                g0, g1 = chr_start[k], chr_start[k + 1]
                want[g0:g1, t] = np.isnan(literal_median_filter(x[g0:g1][:, t], 7))
    got = mr.na_outputs(mr.is_na_bits(x), chr_start, tiles, 7)
    assert np.array_equal(got, want)
    assert not got[:, perm[11:]].any()
    assert not got[5:, perm[:6]].any() and got[:5, perm[:6]].all()      # the NA of chromosome 0 stays in its block (5 genes: one window)


def test_is_na_bits_takes_every_nan_and_no_infinity():
    bits = np.array([0x7FF00000000007A2, 0xFFF8000000000000, 0x7FF0000000000001, 0x7FF8000000000000,
                     0x7FF0000000000000, 0xFFF0000000000000, 0x7FEFFFFFFFFFFFFF, 0, 0x8000000000000000], dtype=np.uint64)
    assert mr.is_na_bits(bits.view(np.float64)).tolist() == [True, True, True, True, False, False, False, False, False]
