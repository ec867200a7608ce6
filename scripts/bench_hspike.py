#!/usr/bin/env python3
"""Benchmark of the hidden spike-in's two device passes (icnv_group_gene_tables_dev / icnv_hspike_simulate_dev, DESIGN K15).
Prints ONE JSON line (and writes it with --out).

  tables    the group gene tables of synth.make_matrix_torch(10 000, 50 000) over synth.groups(C): 2 reference and 4
            observation groups that cover every cell once.  Wall ms of the whole call (index upload, four launches, the
            synchronise) and its rate on the floor of two reads of the matrix; beside it, in the same run, the read-only
            streaming rate of the same matrix: the faster of the library's col_sums and a torch.sum, each one read.  The
            reported fraction is the call's rate over that streaming rate.  No target is fixed in advance.
  simulate  4 matrices of 10 000 genes x 100 cells in one launch (two normal types: normal and spiked each), from a
            variance spline and a dropout spline fitted on the host to a synthetic trend; the host fit is timed beside it.

Times are wall clock around whole calls (each synchronises) after a warm-up call; the median is reported."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from infercnv_amd import device, synth  # noqa: E402
from infercnv_amd.smooth_spline import smooth_spline  # noqa: E402


def timed(fn, reps):
    out, ms = None, []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=10000)
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hspike.py needs a GPU")
    torch.cuda.set_device(0)
    device.init(0)
    G, C = a.genes, a.cells
    x, _ = synth.make_matrix_torch(G, C, "cuda")
    refs, obs = synth.groups(C)
    groups = list(obs) + list(refs)
    nbytes = 8.0 * G * C
    res = {"bench": "hspike", "genes": G, "cells": C, "groups": [int(len(g)) for g in groups], "reps": a.reps}

    device.col_sums(x)
    _, ms_cs = timed(lambda: device.col_sums(x), a.reps)
    torch.sum(x)
    _, ms_ts = timed(lambda: torch.sum(x), a.reps)
    stream_ms = min(float(np.median(ms_cs)), float(np.median(ms_ts)))
    stream = nbytes / (stream_ms * 1e-3)
    device.group_gene_tables(x, groups)
    (m, v, nz), ms_t = timed(lambda: device.group_gene_tables(x, groups), a.reps)
    t_ms = float(np.median(ms_t))
    device.group_means(x, groups)
    _, ms_gm = timed(lambda: device.group_means(x, groups), a.reps)
    res["tables"] = {
        "ms": t_ms, "ms_all": [round(t, 3) for t in ms_t],
        "floor_bytes": 2 * nbytes, "rate_TBps": 2 * nbytes / (t_ms * 1e-3) / 1e12,
        "stream_read_ms": {"col_sums": float(np.median(ms_cs)), "torch_sum": float(np.median(ms_ts))},
        "stream_read_TBps": stream / 1e12,
        "fraction_of_stream_rate": (2 * nbytes / (t_ms * 1e-3)) / stream,
        "group_means_ms": float(np.median(ms_gm)),
    }

    rng = np.random.default_rng(3)
    sx = np.sort(rng.uniform(0.0, 8.0, 20000))
    t0 = time.perf_counter()
    fv = smooth_spline(sx, 1.1 * sx - 0.3 + 0.2 * np.sin(sx) + 0.3 * rng.standard_normal(sx.size))
    px = np.sort(rng.uniform(-6.0, 7.0, 20000))
    fp = smooth_spline(px, 1.0 / (1.0 + np.exp(1.5 * (px - 1.0))) + 0.02 * rng.standard_normal(px.size))
    fit_ms = (time.perf_counter() - t0) * 1e3
    means = np.exp(rng.normal(1.0, 1.5, size=(4, 10000)))
    tokens = [11, 12, 13, 14]
    device.hspike_simulate(means, 100, fv, fp, 0, tokens)
    sim, ms_s = timed(lambda: device.hspike_simulate(means, 100, fv, fp, 0, tokens), a.reps)
    res["simulate"] = {"matrices": 4, "genes": 10000, "cells": 100, "ms": float(np.median(ms_s)), "ms_all": [round(t, 3) for t in ms_s],
                       "values_per_s": 4 * 10000 * 100 / (float(np.median(ms_s)) * 1e-3), "zero_fraction": float((sim == 0).double().mean().item()),
                       "host_fit_two_splines_20000_points_ms": fit_ms}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
