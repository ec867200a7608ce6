#!/usr/bin/env python3
"""Benchmark of the PCA route of the Leiden subclustering (DESIGN K18; .leiden_seurat_preprocess_routine,
R/inferCNV_tumor_subclusters.R:699-723), per stage, with the "simple" route (K8 + K11) on the same inputs in the same run.
Prints ONE JSON line (and writes it with --out).

  a        one group of 50 000 cells x 10 000 genes, k = 20, CPM, auto resolution
  b        23 chromosomes x 4 groups x 12 500 cells (92 problems, 10 000 genes), k = 20, modularity, gamma = 1

Times are wall clock around whole stages (each synchronises) after a warm-up run of the route; the host stages (the trend
fit, numpy.linalg.eigh) are part of them and reported by name.  No time is fixed in advance."""
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
from infercnv_amd import tumor_subclusters as ts  # noqa: E402


def make_data(G, C, seed, n_clones=5):
    """step-15-like data on the device (cells x genes): positive per-gene levels, clones with their own profiles, cell noise"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((C, G), generator=g, device="cuda", dtype=torch.float64) * 0.05
    x += 0.5 + 2.5 * torch.rand((1, G), generator=g, device="cuda", dtype=torch.float64)
    cl = torch.randint(0, n_clones, (C,), generator=g, device="cuda")
    x += (torch.randn((n_clones, G), generator=g, device="cuda", dtype=torch.float64) * 0.05)[cl]
    return x.contiguous()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def case(name, x, problems, k, objective, gammas, reps):
    genes = [g for g, _ in problems]
    cells = [c for _, c in problems]
    sizes = [c.size for c in cells]
    best = None
    for rep in range(reps + 1):                      # the first run warms the pool up
        t = {}
        st = ts.pca_stages(x, genes, cells, k, timings=t)
        scaled = [ts._graph_resolution(objective, g) for g in gammas]
        (memb, ncl), t["leiden_graph"] = wall(lambda: device.leiden_graph(st["row_off"], st["col"], st["weight"], st["loop"], st["n_cells"],
                                                                          objective, [scaled[p] for p in st["active"]]))
        t["total"] = sum(t.values())
        if rep and (best is None or t["total"] < best["total"]):
            best = t
    (idx, _), knn_ms = wall(lambda: device.knn(x, problems, k))
    device.leiden(idx, sizes, objective, gammas)     # warm-up
    (_, ncl_s), leiden_ms = wall(lambda: device.leiden(idx, sizes, objective, gammas))
    return {"case": name, "problems": len(problems), "cells": int(sum(sizes)), "k": k, "objective": objective,
            "pca_route_ms": {k2: round(v, 2) for k2, v in best.items()}, "fallbacks": len(st["fallback"]),
            "snn_entries": int(st["col"].numel()), "clusters": [int(v) for v in ncl[:8]],
            "simple_route_ms": {"knn": round(knn_ms, 2), "leiden": round(leiden_ms, 2), "total": round(knn_ms + leiden_ms, 2)},
            "simple_clusters": [int(v) for v in ncl_s[:8]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--cases", default="a,b")
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--genes", type=int, default=10000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    device.init(0)
    G, C = args.genes, args.cells
    res = {"bench": "leiden_pca", "device": torch.cuda.get_device_name(0), "genes": G, "cells": C, "cases": []}
    cases = args.cases.split(",")
    if "a" in cases:
        x = make_data(G, C, 1)
        res["cases"].append(case(f"a_single_{C}", x, [(np.arange(G, dtype=np.int32), np.arange(C, dtype=np.int32))], 20, "CPM",
                                 [ts.auto_leiden_resolution(C)], args.reps))
        del x
    if "b" in cases:
        x = make_data(G, C, 2)
        bounds = np.linspace(0, G, 24).astype(np.int32)
        q = C // 4
        problems = [(np.arange(bounds[c], bounds[c + 1], dtype=np.int32), np.arange(grp * q, (grp + 1) * q, dtype=np.int32))
                    for c in range(23) for grp in range(4)]
        res["cases"].append(case(f"b_per_chr_92x{q}", x, problems, 20, "modularity", [1.0] * len(problems), args.reps))
        del x
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
