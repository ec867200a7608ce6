#!/usr/bin/env python3
"""Benchmark of the exact matrix sum (icnv_matrix_sum_dev, DESIGN K23) and of plot_per_group.  Prints ONE JSON line (and
writes it with --out, default profiles/bench_sampling.json).

The matrix is synth.make_matrix_torch(10 000, 50 000) with synth.groups' six groups (two reference, four observation).  One
warm-up call, then the median of three:
  matrix_sum     device.matrix_sum beside a read-only stream of the same matrix in the same run (the faster of the library's
                 col_sums and torch.sum, one read each), as a ratio of wall times
  fsum           math.fsum on a 10 000 x 200 slice, given as a rate and EXTRAPOLATED linearly to the full size
  plot_per_group end to end with write_expr_matrix = False, split into centre + range, gathers and plot_cnv calls (timers
                 around device.matrix_mean / quantiles_excluding / gather_matrix and heatmap._plot_cnv; the rest is the upload).
                 --plot-cells N draws from the first N cells of every group instead of all of them (stated in the result)."""
import argparse
import json
import math
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from infercnv_amd import GeneOrder, InfercnvObject, device, heatmap, sampling, synth  # noqa: E402


def timed(fn, reps=3):
    fn()                                        # warm-up
    out, ms = None, []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, statistics.median(ms), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=10000)
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--plot-cells", type=int, default=0, help="cells per group that plot_per_group draws (0: all)")
    ap.add_argument("--no-plot", action="store_true", help="skip the end-to-end plot_per_group")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_sampling.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sampling.py needs a GPU")
    torch.cuda.set_device(0)
    device.init(0)
    G, C = a.genes, a.cells
    x, chr_start = synth.make_matrix_torch(G, C, "cuda")
    refs, obs = synth.groups(C)
    nbytes = 8.0 * G * C
    res = {"bench": "sampling", "device": torch.cuda.get_device_name(0), "genes": G, "cells": C, "groups": len(refs) + len(obs)}

    total, ms_sum, all_sum = timed(lambda: device.matrix_sum(x))
    _, ms_torch, _ = timed(lambda: x.sum().item())
    _, ms_col, _ = timed(lambda: device.col_sums(x))
    stream_ms = min(ms_torch, ms_col)
    res["matrix_sum"] = {"sum": total, "ms": ms_sum, "ms_all": all_sum, "GBps": nbytes / ms_sum / 1e6, "stream_ms": stream_ms,
                         "stream": "torch.sum" if ms_torch <= ms_col else "col_sums", "stream_GBps": nbytes / stream_ms / 1e6,
                         "ratio_to_stream": ms_sum / stream_ms}

    part = x[:200].cpu().numpy().ravel().tolist()
    t0 = time.perf_counter()
    math.fsum(part)
    dt = time.perf_counter() - t0
    res["fsum"] = {"slice": [G, 200], "values_per_s": len(part) / dt, "extrapolated_s_full": dt * C / 200}

    if not a.no_plot:
        if a.plot_cells:
            refs, obs = [r[:a.plot_cells] for r in refs], [o[:a.plot_cells] for o in obs]
            keep = np.concatenate(refs + obs)
            where = {int(c): i for i, c in enumerate(keep)}
            expr = np.ascontiguousarray(x[torch.from_numpy(keep.astype(np.int64)).cuda()].cpu().numpy().T)
            refs, obs = [np.array([where[int(c)] for c in r]) for r in refs], [np.array([where[int(c)] for c in o]) for o in obs]
        else:
            expr = np.ascontiguousarray(x.cpu().numpy().T)
        del x
        chrs = np.repeat(np.array([f"chr{i + 1}" for i in range(len(chr_start) - 1)]), np.diff(chr_start))
        obj = InfercnvObject(expr_data=expr, gene_order=GeneOrder(chr=chrs),
                             reference_grouped_cell_indices={f"normal_{i + 1}": r for i, r in enumerate(refs)},
                             observation_grouped_cell_indices={f"tumor_{i + 1}": o for i, o in enumerate(obs)})
        spent = {"centre_range": 0.0, "gathers": 0.0, "plot_cnv": 0.0}
        depth = [0]                               # inside plot_cnv: its own quantile call is part of "plot_cnv"

        def wrap(module, name, key, enters=False):
            inner = getattr(module, name)

            def outer(*args, **kw):
                if depth[0]:
                    return inner(*args, **kw)
                torch.cuda.synchronize()
                t = time.perf_counter()
                depth[0] += enters
                try:
                    return inner(*args, **kw)
                finally:
                    depth[0] -= enters
                    torch.cuda.synchronize()
                    spent[key] += time.perf_counter() - t
            setattr(module, name, outer)
            return module, name, inner

        saved = [wrap(heatmap, "_plot_cnv", "plot_cnv", True), wrap(device, "matrix_mean", "centre_range"),
                 wrap(device, "quantiles_excluding", "centre_range"), wrap(device, "gather_matrix", "gathers")]
        runs = []
        for i in range(4):                        # one warm-up, then three: a run writes one page per group
            for k in spent:
                spent[k] = 0.0
            with tempfile.TemporaryDirectory() as tmp:
                t0 = time.perf_counter()
                sampling.plot_per_group(obj, out_dir=tmp, write_expr_matrix=False)
                wall = time.perf_counter() - t0
            runs.append(dict(spent, wall_s=wall, upload_and_rest_s=wall - sum(spent.values())))
        for module, n, inner in saved:
            setattr(module, n, inner)
        median_run = sorted(runs[1:], key=lambda r: r["wall_s"])[1]
        res["plot_per_group"] = {"cells_drawn": int(expr.shape[1]), "cells_per_group": a.plot_cells or "all", "write_expr_matrix": False,
                                 "warm_up": runs[0], "median_of_three": median_run}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
