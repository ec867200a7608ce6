#!/usr/bin/env python3
"""Benchmark of the Leiden community detection (icnv_leiden_dev, DESIGN K11): cluster_leiden of .leiden_simple_snn
(R/inferCNV_tumor_subclusters.R:726-741) on the kNN blocks of K8.  Prints ONE JSON line (and writes it with --out).

  a        one group of 50 000 cells x 10 000 genes, k = 20, CPM, auto resolution
  b        23 chromosomes x 4 groups x 12 500 cells (92 problems, 10 000 genes), k = 20, modularity, gamma = 1
  c        define_signif_tumor_subclusters on 10 000 genes x 50 000 cells in 5 groups (leiden_method = "simple"):
           kNN, Leiden and trees split (the library's stats counters)

Times are wall clock around whole calls (each synchronises) after a warm-up call.  The target is Leiden <= 0.5 x the K8
call on the same problems.  --restate also times tests/leiden_restate.py on one 2 000-cell problem (context only: igraph
is not a dependency of the project, so R's cluster_leiden is not timed)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from infercnv_amd import device  # noqa: E402


def make_data(G, C, seed, n_clones=5):
    """smoothed-like data on the device (cells x genes): per-gene offsets, clones with their own profiles, cell noise"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((C, G), generator=g, device="cuda", dtype=torch.float64) * 0.3
    x += torch.randn((1, G), generator=g, device="cuda", dtype=torch.float64)
    cl = torch.randint(0, n_clones, (C,), generator=g, device="cuda")
    x += (torch.randn((n_clones, G), generator=g, device="cuda", dtype=torch.float64) * 0.5)[cl]
    return x.contiguous()


def timed(fn, reps):
    out, ms = None, []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, ms


def case_knn_leiden(name, x, problems, k, objective, gammas, reps):
    idx, _ = device.knn(x, problems, k)
    _, knn_ms = timed(lambda: device.knn(x, problems, k), reps)
    sizes = [c.size for _, c in problems]
    device.leiden(idx, sizes, objective, gammas)           # warm-up
    device.leiden_stats(reset=True)
    (memb, ncl), ms = timed(lambda: device.leiden(idx, sizes, objective, gammas), reps)
    st = device.leiden_stats(reset=True)
    per_call = {k2: v / reps for k2, v in st.items()}
    best = min(ms)
    return {"case": name, "problems": len(problems), "cells": int(sum(sizes)), "k": k, "objective": objective,
            "leiden_ms": round(best, 2), "leiden_ms_all": [round(v, 2) for v in ms], "knn_ms": round(min(knn_ms), 2),
            "leiden_vs_knn": round(best / min(knn_ms), 3), "clusters": [int(v) for v in ncl[:8]],
            "stats_per_call": per_call}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--restate", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    device.init(0)
    G = 10000
    res = {"bench": "leiden", "device": torch.cuda.get_device_name(0),
           "targets": {"a leiden_ms": "<= 535", "b leiden_ms": "<= 240", "leiden_vs_knn": "<= 0.5"}, "cases": []}
    cases = args.cases.split(",")
    genes = np.arange(G, dtype=np.int32)
    if "a" in cases:
        x = make_data(G, 50000, 1)
        n = 50000
        res["cases"].append(case_knn_leiden("a_single_50000", x, [(genes, np.arange(n, dtype=np.int32))], 20, "CPM",
                                            [(11.98 / n) ** (1 / 1.165)], args.reps))
        del x
    if "b" in cases:
        x = make_data(G, 50000, 2)
        bounds = np.linspace(0, G, 24).astype(np.int32)
        problems = [(np.arange(bounds[c], bounds[c + 1], dtype=np.int32), np.arange(grp * 12500, (grp + 1) * 12500, dtype=np.int32))
                    for c in range(23) for grp in range(4)]
        res["cases"].append(case_knn_leiden("b_per_chr_92x12500", x, problems, 20, "modularity", [1.0] * len(problems), args.reps))
        del x
    if "c" in cases:
        from infercnv_amd import tumor_subclusters as ts
        from infercnv_amd.infercnv_object import GeneOrder, InfercnvObject
        x = make_data(G, 50000, 3)
        obj = InfercnvObject(expr_data=x.t().cpu().numpy(), gene_order=GeneOrder(chr=np.repeat([f"chr{i}" for i in range(1, 11)], G // 10)),
                             observation_grouped_cell_indices={f"g{i}": np.arange(i * 10000, (i + 1) * 10000) for i in range(5)})
        del x
        for st in (device.knn_stats, device.leiden_stats, device.hclust_stats):
            st(reset=True)
        t0 = time.perf_counter()
        out, _ = ts.define_signif_tumor_subclusters(obj, leiden_method="simple", z_score_filter=0)
        torch.cuda.synchronize()
        total = (time.perf_counter() - t0) * 1e3
        kn = device.knn_stats(reset=True)
        ld = device.leiden_stats(reset=True)
        hc = device.hclust_stats(reset=True)
        subs = out.tumor_subclusters["subclusters"]
        res["cases"].append({"case": "c_define_signif_5x10000", "total_ms": round(total, 1),
                             "leiden_ms": round(ld["us"] / 1e3, 1), "trees_ms": round(hc["us"] / 1e3, 1),
                             "knn_calls": kn["calls"], "leiden_calls": ld["calls"], "hclust_calls": hc["calls"],
                             "knn_and_host_ms": round(total - ld["us"] / 1e3 - hc["us"] / 1e3, 1),
                             "subclusters": {g: len(v) for g, v in subs.items()}})
    if args.restate:
        import leiden_restate as lr
        from scipy.spatial import cKDTree
        rng = np.random.default_rng(0)
        X = rng.normal(size=(2000, 10))
        X[np.arange(2000), rng.integers(0, 5, 2000)] += 6.0
        nn = cKDTree(X).query(X, k=20)[1].astype(np.int32)
        t0 = time.perf_counter()
        lr.leiden(nn, lr.CPM, (11.98 / 2000) ** (1 / 1.165))
        res["restatement_ms_per_2000_cell_problem"] = round((time.perf_counter() - t0) * 1e3, 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
