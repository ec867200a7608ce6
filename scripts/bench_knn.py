#!/usr/bin/env python3
"""Benchmark of the exact kNN (icnv_knn_dev, DESIGN K8): RANN::nn2 of the Leiden subclustering
(R/inferCNV_tumor_subclusters.R:726).  Prints ONE JSON line.

  single   one tumour group: 50 000 cells x 10 000 genes, k = 20
  per_chr  the per-chromosome batch of :646-697: 23 chromosomes x 4 groups of 12 500 cells (10 000 genes), k = 20, one call

Times are device events around whole calls after a warm-up call.  A second call with the library's per-kernel timers on
gives the split (gather / screen / select / refine / exhaustive).  The screen's rate is 2 sum_p n_p^2 G_p over the screen
kernel's time, set against K7's measured 42 TFLOP/s and the fp64 matrix-core peak (78.6 TFLOP/s).  32 query rows per case
are checked against an oracle that sums (x_i - x_j)^2 over the genes in order, one rounded operation at a time.
--k7 also times K7 (icnv_cell_distances_dev, 10 000 x 10 000 cells, 10 000 genes), the kernel the screen shares its tiles with.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ctypes as ct  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

from infercnv_amd import _lib, device  # noqa: E402

K7_TFLOPS = 42.0          # DESIGN K7, measured
PEAK_TFLOPS = 78.6        # fp64 MFMA peak of the MI355X


def make_data(G, C, seed):
    """continuous, smoothed-like data on the device: per-gene offsets, five cell clusters, cell noise"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((C, G), generator=g, device="cuda", dtype=torch.float64) * 0.3
    x += torch.randn((1, G), generator=g, device="cuda", dtype=torch.float64)
    cl = torch.randint(0, 5, (C,), generator=g, device="cuda")
    x += (torch.randn((5, G), generator=g, device="cuda", dtype=torch.float64) * 0.5)[cl]
    return x.contiguous()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def kernel_split():
    L = _lib.load()
    out = {}
    for name in ("knn_gather", "knn_screen", "knn_select", "knn_refine", "knn_exhaustive"):
        ms, n = ct.c_double(0.0), ct.c_int64(0)
        L.icnv_timing_get(name.encode(), ct.byref(ms), ct.byref(n))
        out[name] = round(ms.value, 3)
    return out


def oracle_check(x, problems, k, got_i, got_d, n_rows, seed):
    """n_rows query rows spread over the problems: exact sequential sums on the device, one rounded operation per
    kernel (torch.sub / mul / add: nothing can contract into an FMA), ranked by (d2, j)"""
    rng = np.random.default_rng(seed)
    offs = np.cumsum([0] + [len(c) for _, c in problems])
    picks = rng.choice(offs[-1], n_rows, replace=False)
    bad = 0
    for r in picks:
        p = int(np.searchsorted(offs, r, side="right") - 1)
        genes, cells = problems[p]
        i = int(r - offs[p])
        cells_t = torch.from_numpy(np.asarray(cells, dtype=np.int64)).cuda()
        X = x[cells_t]                                    # n_p x G
        s = torch.zeros(len(cells), dtype=torch.float64, device="cuda")
        for g in np.asarray(genes):
            col = X[:, int(g)]
            t = torch.sub(col[i], col)
            s = torch.add(s, torch.mul(t, t))
        d2 = s.cpu().numpy()
        order = np.lexsort((np.arange(d2.size), d2))[:k]
        if not (np.array_equal(got_i[r], order) and np.array_equal(got_d[r].view(np.uint64), np.sqrt(d2[order]).view(np.uint64))):
            bad += 1
    return {"rows": int(n_rows), "mismatches": int(bad)}


def run_case(name, x, problems, k, reps, check_rows):
    L = _lib.load()
    gram_flop = float(sum(2.0 * len(c) ** 2 * len(g) for g, c in problems))
    device.knn(x, problems, k)                          # warm-up (pool allocations, code objects)
    torch.cuda.synchronize()
    device.knn_stats(reset=True)
    times = []
    for _ in range(reps):
        ms, (idx, dist) = timed(lambda: device.knn(x, problems, k))
        times.append(ms)
    stats = device.knn_stats(reset=True)
    L.icnv_timing_reset()
    L.icnv_timing_enable(1)
    device.knn(x, problems, k)
    torch.cuda.synchronize()
    split = kernel_split()
    L.icnv_timing_enable(0)
    L.icnv_timing_reset()
    ms = float(np.median(times))
    screen_tflops = gram_flop / (split["knn_screen"] * 1e-3) / 1e12 if split["knn_screen"] > 0 else None
    res = {"case": name, "problems": len(problems), "k": k, "ms": round(ms, 2), "ms_all": [round(t, 2) for t in times],
           "split_ms": split, "gram_flop": gram_flop, "screen_tflops": round(screen_tflops, 2) if screen_tflops else None,
           "screen_vs_k7": round(screen_tflops / K7_TFLOPS, 3) if screen_tflops else None,
           "screen_vs_peak": round(screen_tflops / PEAK_TFLOPS, 3) if screen_tflops else None,
           "call_vs_screen": round(ms / split["knn_screen"], 3) if split["knn_screen"] > 0 else None,
           "call_vs_gram_at_k7_rate": round(ms / (gram_flop / (K7_TFLOPS * 1e12) * 1e3), 3),
           "stats_per_call": {kk: v // reps for kk, v in stats.items()}}
    if check_rows:
        res["oracle"] = oracle_check(x, problems, k, idx.cpu().numpy(), dist.cpu().numpy(), check_rows, seed=len(problems))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--check-rows", type=int, default=32)
    ap.add_argument("--cases", default="single,per_chr")
    ap.add_argument("--k7", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    device.init(0)
    k, G = 20, 10000
    out = {"bench": "knn", "device": torch.cuda.get_device_name(0), "targets": {
        "screen_vs_k7": ">= 0.8", "single call_vs_screen": "<= 1.3", "per_chr call_vs_gram_at_k7_rate": "<= 1.5"}, "cases": []}
    t0 = time.time()
    cases = args.cases.split(",")
    if "single" in cases:
        x = make_data(G, 50000, 1)
        out["cases"].append(run_case("single_50000x10000", x, [(np.arange(G), np.arange(50000))], k, args.reps, args.check_rows))
        del x
    if "per_chr" in cases:
        x = make_data(G, 50000, 2)
        bounds = np.linspace(0, G, 24).astype(np.int64)
        problems = [(np.arange(bounds[c], bounds[c + 1]), np.arange(q * 12500, (q + 1) * 12500))
                    for c in range(23) for q in range(4)]
        out["cases"].append(run_case("per_chr_23x4x12500", x, problems, k, args.reps, args.check_rows))
        del x
    if args.k7:
        x = make_data(G, 10000, 3)
        cells = np.arange(10000, dtype=np.int32)
        device.cell_distances(x, cells)
        torch.cuda.synchronize()
        ts = [timed(lambda: device.cell_distances(x, cells))[0] for _ in range(3)]
        out["k7_cell_distances_10000x10000_ms"] = round(float(np.median(ts)), 2)
    torch.cuda.empty_cache()
    out["wall_s"] = round(time.time() - t0, 1)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
