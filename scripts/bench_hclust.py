#!/usr/bin/env python3
"""Benchmark of the hierarchical clustering (icnv_hclust_cells_dev, DESIGN K9): hclust(parallelDist(t(x)), "ward.D2") of
the subclustering (R/inferCNV_tumor_subclusters.R:191, 582, 609).  Writes profiles/bench_hclust.json and prints it.

  single   one group of 50 000 cells x 10 000 genes, split into the distance stage (R's sequential dist) and the clustering stage
           (finiteness check + chain); one call
  leiden   250 partitions of 20 - 1 000 cells (random subsets of 40 000 cells) over 10 000 genes, one batched call
  host     the route the reference takes once the distances are on the device: a D2H copy of K7's matrix
           (icnv_cell_distances_dev) plus SciPy's `linkage(..., "ward")` on it, at n = 10 000 and 20 000, against one
           icnv_hclust_cells_dev call on the same cells

Times are wall clock around whole calls after a warm-up call (the entry points synchronise); the split comes from the
library's per-kernel timers, enabled in the same call.
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

KERNELS = ("exact_dist", "hclust_prep", "hclust_lds", "hclust_hbm")


def make_data(G, C, seed):
    """continuous, smoothed-like data on the device: per-gene offsets, five cell clusters, cell noise"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((C, G), generator=g, device="cuda", dtype=torch.float64) * 0.3
    x += torch.randn((1, G), generator=g, device="cuda", dtype=torch.float64)
    cl = torch.randint(0, 5, (C,), generator=g, device="cuda")
    x += (torch.randn((5, G), generator=g, device="cuda", dtype=torch.float64) * 0.5)[cl]
    return x.contiguous()


def call(x, problems, split=False):
    if split:
        device.timing_reset()
        device.timing_enable(True)
    device.hclust_stats(reset=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = device.hclust_cells(x, problems, "ward.D2")
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    out = {"ms": round(ms, 2), "stats": device.hclust_stats(reset=True)}
    if split:
        out["split_ms"] = {k: round(device.timing_get(k)[0], 3) for k in KERNELS}
        device.timing_enable(False)
        device.timing_reset()
    return out, res


def host_baseline(x, n):
    from scipy.cluster.hierarchy import linkage
    from scipy.spatial.distance import squareform
    cells = np.arange(n, dtype=np.int32)
    d = device.cell_distances(x, cells)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    D = d.cpu().numpy()
    t1 = time.perf_counter()
    Z = linkage(squareform(D, checks=False), "ward")
    t2 = time.perf_counter()
    del d
    gpu, res = call(x, [(np.arange(x.shape[1]), cells)])
    m = res[0][0].cpu().numpy()
    ab = np.sort(Z[:, :2].astype(np.int64), axis=1)
    same = bool(np.array_equal(m, np.where(ab < n, -(ab + 1), ab - n + 1)))
    host_ms = (t2 - t0) * 1e3
    return {"case": f"host_baseline_n{n}", "d2h_ms": round((t1 - t0) * 1e3, 1), "scipy_linkage_ms": round((t2 - t1) * 1e3, 1),
            "host_ms": round(host_ms, 1), "gpu_call_ms": gpu["ms"], "speedup": round(host_ms / gpu["ms"], 2),
            "same_topology": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="single,leiden,host")
    ap.add_argument("--single-cells", type=int, default=50000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_hclust.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    device.init(0)
    G = 10000
    cases = args.cases.split(",")
    out = {"bench": "hclust", "device": torch.cuda.get_device_name(0), "method": "ward.D2", "genes": G, "cases": []}

    if "leiden" in cases:
        x = make_data(G, 40000, 2)
        rng = np.random.default_rng(7)
        sizes = rng.integers(20, 1001, size=250)
        problems = [(np.arange(G), np.sort(rng.choice(40000, size=int(s), replace=False)).astype(np.int32)) for s in sizes]
        call(x, problems)   # warm-up: the workspace pool grows to the batch's size once
        r, _ = call(x, problems, split=True)
        r.update(case="leiden_250", problems=250, cells=int(sizes.sum()), min_cells=int(sizes.min()), max_cells=int(sizes.max()))
        out["cases"].append(r)
        print(json.dumps(r), flush=True)
        del x

    if "host" in cases:
        x = make_data(G, 20000, 3)
        call(x, [(np.arange(G), np.arange(300, dtype=np.int32))])   # warm-up
        for n in (10000, 20000):
            r = host_baseline(x, n)
            out["cases"].append(r)
            print(json.dumps(r), flush=True)
        del x

    if "single" in cases:
        n = args.single_cells
        x = make_data(G, n, 1)
        call(x, [(np.arange(G), np.arange(300, dtype=np.int32))])   # warm-up
        r, res = call(x, [(np.arange(G), np.arange(n, dtype=np.int32))], split=True)
        sp = r["split_ms"]
        r.update(case=f"single_{n}x{G}", distance_ms=round(sp["exact_dist"], 1),
                 clustering_ms=round(sp["hclust_prep"] + sp["hclust_lds"] + sp["hclust_hbm"], 1),
                 steps_per_cell=round(r["stats"]["chain_steps"] / n, 3))
        h = res[0][1].cpu().numpy()
        r["heights_sorted"] = bool(np.all(np.diff(h) >= 0))
        out["cases"].append(r)
        print(json.dumps(r), flush=True)

    line = json.dumps(out)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
