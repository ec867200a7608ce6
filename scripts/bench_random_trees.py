#!/usr/bin/env python3
"""Benchmark of the random-trees subclustering (icnv_random_trees_dev, DESIGN K10): the permutation statistic of
R/inferCNV_tumor_subclusters.random_smoothed_trees.R:217-298, ward.D2, 10 000 genes, 100 iterations, window 101.
Writes profiles/bench_random_trees.json and prints it.

  single2000   one clade of 2 000 cells (1 observed + 100 permuted trees), one call
  level8       one recursion level of 8 clades x 1 000 cells (808 trees), one call
  define10k    define_signif_tumor_subclusters_via_random_smooothed_trees on 10 000 cells in 5 groups of 2 000 (wall time,
               one device call per recursion level)
  single20000  one clade of 20 000 cells, built in waves (ICNV_RT_SCRATCH_MB = 131072)
  cpu1000      the NumPy restatement's permutation + runmean + centring and SciPy's pdist + linkage at 1 000 cells: a few
               trees timed, scaled to 101, against the device call on the same clade

Times are wall clock around whole calls after a warm-up call (the entry point synchronises); the split comes from the
library's per-kernel timers, enabled in a second timed call.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from infercnv_amd import device  # noqa: E402

KERNELS = ("rt_check", "rt_permute", "rt_smooth", "chain_large_center", "exact_dist", "hclust_prep",
           "hclust_lds", "hclust_hbm", "rt_max_height")
G, ITERS, WINDOW = 10000, 100, 101


def make_data(G, C, seed, clusters=5):
    """log-ratio-like data on the device (cells x genes): per-gene offsets, a few cell clusters, cell noise"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((C, G), generator=g, device="cuda", dtype=torch.float64) * 0.3
    cl = torch.randint(0, clusters, (C,), generator=g, device="cuda")
    x += (torch.randn((clusters, G), generator=g, device="cuda", dtype=torch.float64) * 0.2)[cl]
    return x.contiguous()


def call(x, clades, split=False):
    if split:
        device.timing_reset()
        device.timing_enable(True)
    device.random_trees_stats(reset=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    trees, rand = device.random_trees(x, clades, [1000 + i for i in range(len(clades))], WINDOW, ITERS, 0, "ward.D2")
    torch.cuda.synchronize()
    out = {"ms": round((time.perf_counter() - t0) * 1e3, 2), "stats": device.random_trees_stats(reset=True)}
    if split:
        sp = {k: round(device.timing_get(k)[0], 3) for k in KERNELS}
        out["split_ms"] = sp
        out["stage_ms"] = {"permute": sp["rt_check"] + sp["rt_permute"], "smooth": sp["rt_smooth"],
                           "center": sp["chain_large_center"], "dist": sp["exact_dist"],
                           "chain": sp["hclust_prep"] + sp["hclust_lds"] + sp["hclust_hbm"] + sp["rt_max_height"]}
        out["stage_ms"] = {k: round(v, 2) for k, v in out["stage_ms"].items()}
        pre = out["stage_ms"]["permute"] + out["stage_ms"]["smooth"] + out["stage_ms"]["center"]
        out["pre_share_of_kernels"] = round(pre / max(sum(out["stage_ms"].values()), 1e-9), 3)
        device.timing_enable(False)
        device.timing_reset()
    return out, (trees, rand)


def timed_case(name, x, clades):
    call(x, clades)                         # warm-up: the workspace pool grows once
    r, _ = call(x, clades)
    rs, _ = call(x, clades, split=True)
    r.update(case=name, clades=len(clades), cells=[int(len(c)) for c in clades][:8], split_ms=rs["split_ms"],
             stage_ms=rs["stage_ms"], pre_share_of_kernels=rs["pre_share_of_kernels"], timed_split_call_ms=rs["ms"])
    print(json.dumps(r), flush=True)
    return r


def cpu_restatement(x_host, n, trees=2):
    """ms per tree of the NumPy restatement (permutation, runmean, centring) + SciPy pdist / linkage"""
    sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
    import random_trees_restate as rr
    from scipy.cluster.hierarchy import linkage
    from scipy.spatial.distance import pdist
    cells = np.arange(n)
    t0 = time.perf_counter()
    for r in range(trees):
        Z = rr.clade_matrix(x_host, cells, WINDOW, 0, 1000, r)
        linkage(pdist(Z.T), "ward")
    return (time.perf_counter() - t0) * 1e3 / trees


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="single2000,level8,define10k,single20000,cpu1000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_random_trees.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    device.init(0)
    cases = args.cases.split(",")
    out = {"bench": "random_trees", "device": torch.cuda.get_device_name(0), "method": "ward.D2", "genes": G,
           "iterations": ITERS, "window": WINDOW, "cases": []}

    if "single2000" in cases:
        x = make_data(G, 2000, 1)
        out["cases"].append(timed_case("single_2000", x, [np.arange(2000)]))
        del x
    if "level8" in cases:
        x = make_data(G, 8000, 2)
        out["cases"].append(timed_case("level_8x1000", x, [np.arange(i * 1000, (i + 1) * 1000) for i in range(8)]))
        del x
    if "define10k" in cases:
        from infercnv_amd import tumor_subclusters as ts
        from infercnv_amd.infercnv_object import GeneOrder, InfercnvObject
        rng = np.random.default_rng(3)
        C = 10000
        xh = 1.0 + rng.normal(0.0, 0.3, size=(G, C))
        for grp in range(5):   # two clones per group: a gain and a loss on different chromosomes
            cells = np.arange(grp * 2000, (grp + 1) * 2000)
            half = rng.permutation(cells)[:1000]
            xh[grp * 1000:grp * 1000 + 800, half] += 0.5
        obj = InfercnvObject(xh, GeneOrder(np.repeat([f"chr{i}" for i in range(10)], G // 10)),
                             observation_grouped_cell_indices={f"g{i}": np.arange(i * 2000, (i + 1) * 2000) for i in range(5)})
        levels = []
        orig = device.random_trees

        def timed(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = orig(*a, **k)
            levels.append({"clades": len(a[1]), "cells": int(sum(len(c) for c in a[1])), "ms": round((time.perf_counter() - t0) * 1e3, 1)})
            return res

        device.random_trees = timed
        try:
            ts.define_signif_tumor_subclusters_via_random_smooothed_trees(obj, 0.05, "ward.D2", True)   # warm-up
            levels.clear()
            t0 = time.perf_counter()
            res = ts.define_signif_tumor_subclusters_via_random_smooothed_trees(obj, 0.05, "ward.D2", True)
            wall = (time.perf_counter() - t0) * 1e3
        finally:
            device.random_trees = orig
        r = {"case": "define_signif_10000_5x2000", "wall_ms": round(wall, 1), "levels": levels,
             "subclusters": {g: len(v) for g, v in res.tumor_subclusters["subclusters"].items()}}
        out["cases"].append(r)
        print(json.dumps(r), flush=True)
    if "single20000" in cases:
        os.environ["ICNV_RT_SCRATCH_MB"] = "131072"
        x = make_data(G, 20000, 4)
        call(x, [np.arange(300)])   # warm-up (small)
        r, (trees, rand) = call(x, [np.arange(20000)], split=True)
        h = trees[0][1].cpu().numpy()
        r.update(case="single_20000_waves", scratch_mb=131072, heights_sorted=bool(np.all(np.diff(h) >= 0)),
                 rand_finite=bool(torch.isfinite(rand).all().item()))
        del os.environ["ICNV_RT_SCRATCH_MB"]
        out["cases"].append(r)
        print(json.dumps(r), flush=True)
        del x
    if "cpu1000" in cases:
        x = make_data(G, 1000, 5)
        gpu, _ = call(x, [np.arange(1000)])
        gpu, _ = call(x, [np.arange(1000)])
        per_tree = cpu_restatement(x.cpu().numpy().T, 1000)
        r = {"case": "cpu_restatement_1000", "cpu_ms_per_tree": round(per_tree, 1), "cpu_ms_101_trees_scaled": round(per_tree * 101, 1),
             "gpu_call_ms": gpu["ms"], "speedup": round(per_tree * 101 / gpu["ms"], 1), "cpu_threads": torch.get_num_threads()}
        out["cases"].append(r)
        print(json.dumps(r), flush=True)

    line = json.dumps(out)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
