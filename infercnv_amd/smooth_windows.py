"""Host-side window tables of step 10's "runmeans" and "coordinates" smoothers (R/inferCNV_ops.R:2534-2704) for the banded
window operator of include/icnv.h (icnv_smooth_windows_dev, DESIGN K16):

    out[g, c] = (sum over t = 0 .. len[g] - 1, in this order, of x[lo[g] + t, c] * w[w_off[g] + t]) / denom[g]

Both builders work per chromosome on the `InfercnvObject.chr_layout()` order (chromosomes contiguous, `chr_start` their
offsets); a window never leaves its chromosome.  The windows and weights do not depend on the cell, so a table is built
once and applied to every cell on the device.
"""
from __future__ import annotations

import logging
from dataclasses import dataclass
from typing import Optional

import numpy as np

log = logging.getLogger("infercnv_amd")


@dataclass
class WindowTable:
    """Window g covers the rows lo[g] .. lo[g] + len[g] - 1 (0-based, in the layout order); its weights are
    w[w_off[g] .. w_off[g] + len[g]) (w None: all ones, w_off None); its sum is divided by denom[g]."""
    lo: np.ndarray                      # int32 [G]
    len: np.ndarray                     # int32 [G]
    denom: np.ndarray                   # float64 [G]
    w_off: Optional[np.ndarray] = None  # int64 [G + 1]
    w: Optional[np.ndarray] = None      # float64 [w_off[G]]

    @property
    def G(self):
        return int(self.lo.size)

    @property
    def widest(self):
        return int(self.len.max()) if self.len.size else 0


def _check_chr_start(chr_start):
    cs = np.asarray(chr_start, dtype=np.int64).ravel()
    if cs.size < 1 or cs[0] != 0 or np.any(np.diff(cs) < 0):
        raise ValueError("chr_start must start at 0 and be sorted")
    return cs


def identity_windows(G):
    """Every gene its own window: the table of window_length < 2."""
    G = int(G)
    return WindowTable(np.arange(G, dtype=np.int32), np.ones(G, dtype=np.int32), np.ones(G, dtype=np.float64))


def runmeans_windows(chr_start, window_length):
    """caTools::runmean(k = window_length, endrule = "mean") per chromosome (smooth_by_chromosome_runmeans,
    R/inferCNV_ops.R:2679-2704) with K10's alignment: for a chromosome of n genes k = min(int(window_length), n),
    k2 = k // 2, output o sums [max(0, o - (k - 1 - k2)), min(n - 1, o + k2)] and divides by the window's length; no
    weights.  k <= 1 or n == 1 (nrow(chr_data) > 1, :2690) leaves the genes unchanged."""
    cs = _check_chr_start(chr_start)
    G = int(cs[-1])
    tab = identity_windows(G)
    for a, b in zip(cs[:-1], cs[1:]):
        n = int(b - a)
        k = min(int(window_length), n)
        if n <= 1 or k <= 1:
            continue
        k2 = k // 2
        o = np.arange(n)
        lo = np.maximum(0, o - (k - 1 - k2))
        hi = np.minimum(n - 1, o + k2)
        tab.lo[a:b] = a + lo
        tab.len[a:b] = hi - lo + 1
        tab.denom[a:b] = (hi - lo + 1).astype(np.float64)
    return tab


def coordinate_windows(chr_start, start, stop, window_length):
    """.smooth_helper_by_coordinates (R/inferCNV_ops.R:2594-2622) per gene i of every chromosome, the reference's quirks kept:
    pos = (start[i] + stop[i]) / 2; A = {j: start[j] > pos - w and stop[j] < pos + w}, or {i} when that is empty; weights
    1 - |(stop[j] + start[j]) / 2 - pos| / w over A in index order; `length(around_indices < 10)` is the length of a logical
    vector, so the range always grows by to_add = len(A) // 2 positions on either side (clipped to the chromosome), each with
    weight 0.1.  When A is not contiguous the weight vector (M values) is shorter than the index range (L rows): R recycles
    it over the range (with a warning) and divides by the sum of the M values.  The row stores the recycled weights, denom
    is the sequential double sum of the M values (R's sum() accumulates in long double: the last bits may differ).  One
    warning per call counts such genes.  window_length < 2 (:2569-2572) and one-gene chromosomes (:2545) are unchanged."""
    cs = _check_chr_start(chr_start)
    G = int(cs[-1])
    start = np.asarray(start, dtype=np.float64).ravel()
    stop = np.asarray(stop, dtype=np.float64).ravel()
    if start.size != stop.size or start.size != G:
        raise ValueError(f"start and stop must both have one entry per gene ({G}), got {start.size} and {stop.size}")
    if window_length < 2:
        return identity_windows(G)
    w = float(window_length)
    lo = np.arange(G, dtype=np.int32)
    ln = np.ones(G, dtype=np.int32)
    denom = np.ones(G, dtype=np.float64)
    rows = [None] * G
    recycled = 0
    for a, b in zip(cs[:-1], cs[1:]):
        a, b = int(a), int(b)
        n = b - a
        if n <= 1:
            continue
        s, e = start[a:b], stop[a:b]
        mid = (e + s) / 2
        for i in range(n):
            pos = (s[i] + e[i]) / 2
            A = np.nonzero((s > pos - w) & (e < pos + w))[0]
            if A.size == 0:
                A = np.array([i])
            wts = 1 - np.abs(mid[A] - pos) / w
            to_add = A.size // 2
            first, last = int(A[0]), int(A[-1])
            new_low = max(0, first - to_add)
            new_high = min(n - 1, last + to_add)
            vec = np.concatenate([np.full(first - new_low, 0.1), wts, np.full(new_high - last, 0.1)])
            L = new_high - new_low + 1
            if vec.size != L:
                recycled += 1
            lo[a + i] = a + new_low
            ln[a + i] = L
            denom[a + i] = np.cumsum(vec)[-1]          # sequential, one rounding per add
            rows[a + i] = vec[np.arange(L) % vec.size]
    for g in range(G):
        if rows[g] is None:
            rows[g] = np.ones(1, dtype=np.float64)
    w_off = np.zeros(G + 1, dtype=np.int64)
    w_off[1:] = np.cumsum(ln, dtype=np.int64)
    if recycled:
        log.warning("coordinate_windows: %d genes have a non-contiguous window: the weights are recycled over the index range "
                    "as R does (R/inferCNV_ops.R:2618)", recycled)
    return WindowTable(lo, ln, denom, w_off, np.concatenate(rows) if G else np.zeros(0))


def table_for(infercnv_obj, smooth_method, window_length):
    """The table of `smooth_method` ("runmeans" / "coordinates") for an object, in its chr_layout() order."""
    perm, chr_start = infercnv_obj.chr_layout()
    if smooth_method == "runmeans":
        return runmeans_windows(chr_start, window_length)
    if smooth_method == "coordinates":
        go = infercnv_obj.gene_order
        if go.start is None or go.stop is None:
            raise ValueError('smooth_method "coordinates" needs gene_order.start and gene_order.stop')
        start, stop = np.asarray(go.start), np.asarray(go.stop)
        if perm is not None:
            start, stop = start[perm], stop[perm]
        return coordinate_windows(chr_start, start, stop, window_length)
    raise ValueError(f'smooth_method must be "pyramidinal", "runmeans" or "coordinates", got {smooth_method!r}')


def apply_windows_host(x, table):
    """The contract as a plain loop on a host (G x C) matrix: the yardstick of the tests, never the product path."""
    x = np.asarray(x, dtype=np.float64)
    out = np.empty_like(x)
    for g in range(table.G):
        s = np.zeros(x.shape[1])
        for t in range(int(table.len[g])):
            row = x[int(table.lo[g]) + t]
            s = s + (row if table.w is None else row * table.w[int(table.w_off[g]) + t])
        out[g] = s / table.denom[g]
    return out
