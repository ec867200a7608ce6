"""R's NA result of apply_median_filtering, restated from R/noise_reduction.R:43-113 alone (K19).

.median_filter computes every output of a (chromosome genes x tile cells) block as median(data[posxa:posxb, posya:posyb])
with the window bounds of the four ifelse() lines (:102-106), and median() returns NA as soon as its argument holds one NA
or NaN.  So the NA set of the filter is: the outputs of tiled cells whose window holds an NA.  Cells in no tile are never
assigned (:57-86 walks the tiles only).

Nothing here looks at the library.  The finite values are not restated: where this module says a window is clean, the
filter's existing checker (oracle_c.median_filter on a matrix with finite values at the NA positions) is the expectation.
"""
import numpy as np

NA_REAL_BITS = np.uint64(0x7FF00000000007A2)      # R's NA_real_: a NaN whose low word is 1954


def is_na_bits(x):
    """NA / NaN by the bits of the doubles (any payload, either sign)."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return (b & np.uint64(0x7FFFFFFFFFFFFFFF)) > np.uint64(0x7FF0000000000000)


def ifelse_windows(n, window_size):
    """The 1-based inclusive window [a[p-1], b[p-1]] of every position p = 1 .. n of one direction, by R's own rules:
        half_window = (window_size - 1) / 2                                                   (:52)
        posa <- ifelse(pos <= (half_window + 1), 1, (pos - (half_window + 1)))                (:102, :105)
        posb <- ifelse(pos >= (n - (half_window + 1)), n, (pos + (half_window + 1)))          (:103, :106)"""
    half_window = (window_size - 1) // 2
    pos = np.arange(1, n + 1)
    a = np.where(pos <= (half_window + 1), 1, pos - (half_window + 1))
    b = np.where(pos >= (n - (half_window + 1)), n, pos + (half_window + 1))
    return a, b


def clamp_windows(n, window_size):
    """[max(1, p - h), min(n, p + h)] with h = (window_size - 1) / 2 + 1: the form the header states."""
    h = (window_size - 1) // 2 + 1
    pos = np.arange(1, n + 1)
    return np.maximum(1, pos - h), np.minimum(n, pos + h)


def block_na(isna_block, window_size):
    """Outputs of one block whose window holds an NA: window counts from a 2-D prefix sum of the block's NA flags."""
    xdim, ydim = isna_block.shape
    xa, xb = ifelse_windows(xdim, window_size)
    ya, yb = ifelse_windows(ydim, window_size)
    S = np.zeros((xdim + 1, ydim + 1), dtype=np.int64)
    S[1:, 1:] = np.cumsum(np.cumsum(isna_block.astype(np.int64), axis=0), axis=1)
    cnt = S[xb][:, yb] - S[xa - 1][:, yb] - S[xb][:, ya - 1] + S[xa - 1][:, ya - 1]
    return cnt > 0


def tiled_cells(tiles, C):
    t = np.zeros(C, dtype=bool)
    for idx in tiles:
        t[np.asarray(idx, dtype=np.int64)] = True
    return t


def na_outputs(isna, chr_start, tiles, window_size):
    """(G, C) bool: True where apply_median_filtering assigns NA.  Cells in no tile are False everywhere: they are never
    assigned and keep whatever they held.  (Tiles must not share a cell.)"""
    G, C = isna.shape
    out = np.zeros((G, C), dtype=bool)
    for idx in tiles:
        idx = np.asarray(idx, dtype=np.int64)
        if idx.size == 0:
            continue
        for k in range(len(chr_start) - 1):
            g0, g1 = int(chr_start[k]), int(chr_start[k + 1])
            if g1 > g0:
                out[g0:g1, idx] = block_na(isna[g0:g1][:, idx], window_size)
    return out


def check_output(got, x, chr_start, tiles, window_size, finite_ref):
    """The whole contract on one result: `got` and `x` are (G, C) float64, `finite_ref` the plain filter's checker on a
    matrix that equals x outside its NA positions.  Returns the restated NA set."""
    G, C = x.shape
    isna = is_na_bits(x)
    want_na = na_outputs(isna, chr_start, tiles, window_size)
    tiled = tiled_cells(tiles, C)
    gb = np.ascontiguousarray(got).view(np.uint64)
    got_na = is_na_bits(got)
    assert np.array_equal(got_na[:, tiled], want_na[:, tiled]), "NA set of the tiled cells"
    assert (gb[want_na] == NA_REAL_BITS).all(), "an NA output must be NA_real_"
    clean = ~want_na & tiled[None, :]
    rb = np.ascontiguousarray(finite_ref).view(np.uint64)
    assert np.array_equal(gb[clean], rb[clean]), "outputs of clean windows, bit for bit"
    xb = np.ascontiguousarray(x).view(np.uint64)
    assert np.array_equal(gb[:, ~tiled], xb[:, ~tiled]), "cells in no tile are copied through bit for bit"
    return want_na
