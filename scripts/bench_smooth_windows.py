#!/usr/bin/env python3
"""Benchmark of the window smoothers of step 10 (icnv_smooth_windows_dev, DESIGN K16).  Prints ONE JSON line (and writes it
with --out, default profiles/bench_smooth_windows.json).  Everything is measured in one run on one device:

  runmeans     window 101 on 10 000 genes x 50 000 cells, per-chromosome gene counts from tests/golden/gencode_genes_per_chr.txt
               scaled to 10 000 genes.
  coordinates  w = 1e7 on synthetic coordinates (one gene per ~1e5 bases, lengths 1e3 .. 1e5, a few genes of 2e6).
  hspike       the hspike-shaped coordinates case: start = stop = 1 .. n per chromosome, w = 51 (201 rows per window).
  copy         a plain 1-read : 1-write copy of the same matrix (torch's copy_): the stream ceiling of this box; every time
               above is also given as that copy's time over it ("fraction_of_copy_stream").
  k10_pair     on a single-chromosome 10 000 x 2 000 matrix, K10's smoothing launch (random_trees_matrix, stages = RT_SMOOTH,
               the "rt_smooth" kernel timer) next to the new operator ("smooth_windows" timer) on the same data, alternating.
               The operator must be no slower per gene x cell than K10's launch (3 % allowed for the box-to-box spread): the
               script exits with status 1 otherwise.

Kernel times are the library's hipEvent timers around the launches (icnv_timing_get); "call_ms" is the wall clock around the
whole call (table upload, launch, synchronise).  Medians over --reps after a warm-up call."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from infercnv_amd import _lib, device  # noqa: E402
from infercnv_amd import smooth_windows as sw  # noqa: E402


def chr_starts(G):
    path = os.path.join(ROOT, "tests", "golden", "gencode_genes_per_chr.txt")
    n = np.array([int(line.split()[1]) for line in open(path) if line.strip()], dtype=np.float64)
    sizes = np.maximum(1, np.floor(n * G / n.sum())).astype(np.int64)
    sizes[0] += G - sizes.sum()
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def synthetic_coordinates(cs, rng):
    start, stop = [], []
    for a, b in zip(cs[:-1], cs[1:]):
        n = int(b - a)
        s = np.sort(rng.integers(1, n * 100_000 + 1, size=n)).astype(np.float64)
        ln = rng.integers(1_000, 100_001, size=n).astype(np.float64)
        ln[rng.random(n) < 0.005] = 2_000_000.0
        start.append(s)
        stop.append(s + ln)
    return np.concatenate(start), np.concatenate(stop)


def kernel_ms(fn, name, reps):
    """Per call: (kernel ms from the library's timer `name`, wall ms of the call)."""
    fn()
    k, wall = [], []
    for _ in range(reps):
        device.timing_reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        k.append(device.timing_get(name)[0])
    return k, wall


def copy_ms(x, y, reps):
    y.copy_(x)
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y.copy_(x)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=10000)
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--pair-cells", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_smooth_windows.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_smooth_windows.py needs a GPU")
    torch.cuda.set_device(0)
    device.init(0)
    device.timing_enable(True)
    G, C = a.genes, a.cells
    rng = np.random.default_rng(16)
    cs = chr_starts(G)
    x = torch.randn((C, G), dtype=torch.float64, device="cuda") * 0.3
    out = torch.empty_like(x)
    nbytes = 8.0 * G * C
    res = {"bench": "smooth_windows", "genes": G, "cells": C, "chromosomes": int(cs.size - 1), "reps": a.reps}

    cp = copy_ms(x, out, a.reps)
    copy = float(np.median(cp))
    res["copy"] = {"ms": copy, "ms_all": [round(t, 3) for t in cp], "TBps_read_plus_write": 2 * nbytes / (copy * 1e-3) / 1e12}

    start, stop = synthetic_coordinates(cs, rng)
    pos = np.concatenate([np.arange(1, b - a + 1) for a, b in zip(cs[:-1], cs[1:])]).astype(np.float64)
    t0 = time.perf_counter()
    tables = {"runmeans": sw.runmeans_windows(cs, 101)}
    t1 = time.perf_counter()
    tables["coordinates"] = sw.coordinate_windows(cs, start, stop, 1e7)
    t2 = time.perf_counter()
    tables["hspike"] = sw.coordinate_windows(cs, pos, pos, 51)
    t3 = time.perf_counter()
    build = {"runmeans": (t1 - t0) * 1e3, "coordinates": (t2 - t1) * 1e3, "hspike": (t3 - t2) * 1e3}
    for name, tab in tables.items():
        rows = int(tab.len.astype(np.int64).sum())
        device.smooth_windows_stats(reset=True)
        k, wall = kernel_ms(lambda: device.smooth_windows(x, tab, out=out), "smooth_windows", a.reps)
        st = device.smooth_windows_stats()
        km = float(np.median(k))
        res[name] = {"kernel_ms": km, "kernel_ms_all": [round(t, 3) for t in k], "call_ms": float(np.median(wall)),
                     "host_table_build_ms": build[name], "widest_window": tab.widest, "window_rows": rows,
                     "adds": rows * C, "adds_per_s": rows * C / (km * 1e-3),
                     "tiles_lds_per_call": st["tiles_lds"] // st["calls"], "tiles_spilled_per_call": st["tiles_spilled"] // st["calls"],
                     "fraction_of_copy_stream": copy / km}

    # K10's smoothing launch next to the operator: one chromosome, the same data, alternating
    Cp = a.pair_cells
    xp = x[:Cp].contiguous()
    outp = torch.empty_like(xp)
    cells = np.arange(Cp)
    tab = sw.runmeans_windows([0, G], 101)
    k10 = lambda: device.random_trees_matrix(xp, cells, window_size=101, stages=_lib.RT_SMOOTH)   # noqa: E731
    new = lambda: device.smooth_windows(xp, tab, out=outp)                                          # noqa: E731
    same = bool(torch.equal(k10(), new()))
    t_k10, t_new = [], []
    for _ in range(a.reps):
        t_k10.append(kernel_ms(k10, "rt_smooth", 1)[0][0])
        t_new.append(kernel_ms(new, "smooth_windows", 1)[0][0])
    m_k10, m_new = float(np.median(t_k10)), float(np.median(t_new))
    ok = m_new <= 1.03 * m_k10
    res["k10_pair"] = {"genes": G, "cells": Cp, "window": 101, "bit_equal": same,
                       "rt_smooth_kernel_ms": m_k10, "rt_smooth_kernel_ms_all": [round(t, 4) for t in t_k10],
                       "smooth_windows_kernel_ms": m_new, "smooth_windows_kernel_ms_all": [round(t, 4) for t in t_new],
                       "ns_per_gene_cell": {"rt_smooth": m_k10 * 1e6 / (G * Cp), "smooth_windows": m_new * 1e6 / (G * Cp)},
                       "speedup_over_rt_smooth": m_k10 / m_new, "no_slower_than_k10_within_3_percent": ok}
    device.timing_enable(False)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not (ok and same):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
