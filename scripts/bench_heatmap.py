#!/usr/bin/env python3
"""Benchmark of plot_cnv's data layer (icnv_quantiles_excluding_dev / icnv_heatmap_bins_dev / icnv_heatmap_raster_dev, DESIGN
K17).  Prints ONE JSON line (and writes it with --out, default profiles/bench_heatmap.json).

Three matrices of synth.make_matrix_torch(10 000, 50 000) run through the smoothing chain:
  smoothed     the chain's output before step 22
  denoised     the same after step 22: most entries are ONE value (the dominant-value case)
  centre_90    the smoothed matrix with 90 % of its entries set to x.center (the excluded value)
For each: wall ms per entry point (median after a warm-up call; every call synchronises), the radix passes and compacted
candidates of the quantile call, and bytes read / time as a fraction of the read-only streaming rate measured in the same run
(the faster of the library's col_sums and torch.sum, one read each) -- the quantile call reads the matrix once per pass, the
bins call once; the raster reads H x W samples and is reported in ms only.  End to end: heatmap.plot_cnv(write_expr_matrix =
False) on the smoothed matrix as an InfercnvObject (host matrix in, files out: the upload and the trees of K9 are inside).
CPU yardstick: np.partition for the same two quantiles on a 10 000 x 5 000 slice, EXTRAPOLATED linearly to the full size."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from infercnv_amd import GeneOrder, InfercnvObject, device, heatmap, synth  # noqa: E402


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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-plot", action="store_true", help="skip the end-to-end plot_cnv")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_heatmap.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_heatmap.py needs a GPU")
    torch.cuda.set_device(0)
    device.init(0)
    G, C = a.genes, a.cells
    x, chr_start = synth.make_matrix_torch(G, C, "cuda")
    refs, obs = synth.groups(C)
    denoised, smoothed = device.smooth_chain(x, chr_start, refs, want_pre_denoise=True)
    del x
    nbytes = 8.0 * G * C
    res = {"bench": "heatmap", "device": torch.cuda.get_device_name(0), "genes": G, "cells": C, "reps": a.reps}

    device.col_sums(smoothed)
    _, ms_cs = timed(lambda: device.col_sums(smoothed), a.reps)
    torch.sum(smoothed)
    _, ms_ts = timed(lambda: torch.sum(smoothed), a.reps)
    stream_ms = min(float(np.median(ms_cs)), float(np.median(ms_ts)))
    stream = nbytes / (stream_ms * 1e-3)
    res["stream_read"] = {"col_sums_ms": float(np.median(ms_cs)), "torch_sum_ms": float(np.median(ms_ts)), "TBps": stream / 1e12}

    order = np.random.default_rng(1).permutation(C).astype(np.int32)
    H, W = 1350, 2388                                  # the observation panel of R's page at 300 dpi
    res["cases"] = []
    for name in ("smoothed", "denoised", "centre_90"):
        if name == "smoothed":
            m = smoothed
        elif name == "denoised":
            m = denoised
        else:
            m = smoothed.clone()
        center = float(m.mean().item())
        if name == "centre_90":
            m[torch.rand(m.shape, device=m.device) < 0.9] = center
        device.quantiles_excluding(m, center, (0.01, 0.99))
        device.heatmap_stats(reset=True)
        q, ms_q = timed(lambda: device.quantiles_excluding(m, center, (0.01, 0.99)), a.reps)
        st = device.heatmap_stats(reset=True)
        passes = st["radix_passes"] / a.reps
        reads = passes + (1 if st["candidates"] else 0)
        d = max(abs(center - q["quantiles"][0]), abs(q["quantiles"][1] - center))
        breaks = np.linspace(center - d, center + d, 16)
        device.heatmap_bins(m, breaks)
        counts, ms_b = timed(lambda: device.heatmap_bins(m, breaks), a.reps)
        device.heatmap_raster(m, breaks, order, H, W)
        _, ms_r = timed(lambda: device.heatmap_raster(m, breaks, order, H, W), a.reps)
        q_ms, b_ms = float(np.median(ms_q)), float(np.median(ms_b))
        res["cases"].append({
            "case": name, "x_center": center, "n_kept": q["n_kept"], "n_excluded": q["n_excluded"],
            "quantiles": [float(v) for v in q["quantiles"]], "dominant_bin_share": float(counts.max() / counts.sum()),
            "quantiles_ms": q_ms, "quantiles_ms_all": [round(t, 3) for t in ms_q], "radix_passes": passes,
            "candidates": st["candidates"] / a.reps, "matrix_reads": reads,
            "quantiles_fraction_of_stream_rate": (reads * nbytes / (q_ms * 1e-3)) / stream,
            "bins_ms": b_ms, "bins_ms_all": [round(t, 3) for t in ms_b], "bins_fraction_of_stream_rate": (nbytes / (b_ms * 1e-3)) / stream,
            "raster_ms": float(np.median(ms_r)), "raster_shape": [H, W]})
        if name == "centre_90":
            del m

    sl = smoothed[:min(5000, C)].cpu().numpy().ravel()
    c = float(sl.mean())
    t0 = time.perf_counter()
    kept = sl[sl != c]
    k = [int(np.floor((kept.size - 1) * p)) for p in (0.01, 0.99)]
    np.partition(kept, sorted({k[0], k[0] + 1, k[1], min(k[1] + 1, kept.size - 1)}))
    part_ms = (time.perf_counter() - t0) * 1e3
    res["cpu_np_partition"] = {"slice": [G, min(5000, C)], "ms": part_ms, "ms_extrapolated_linearly_to_full_size": part_ms * C / min(5000, C),
                               "extrapolated": True}

    if not a.no_plot:
        host = np.ascontiguousarray(smoothed.cpu().numpy().T)
        del denoised
        chrs = np.repeat(np.arange(len(chr_start) - 1), np.diff(chr_start)).astype(str)
        obj = InfercnvObject(expr_data=host, gene_order=GeneOrder(chr=chrs),
                             reference_grouped_cell_indices={f"ref{i}": g for i, g in enumerate(refs)},
                             observation_grouped_cell_indices={f"obs{i}": g for i, g in enumerate(obs)})
        with tempfile.TemporaryDirectory() as tmp:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            heatmap.plot_cnv(obj, tmp, x_center=float(smoothed.mean().item()), write_expr_matrix=False)
            torch.cuda.synchronize()
            res["plot_cnv_end_to_end_s"] = time.perf_counter() - t0
            res["plot_cnv_files"] = sorted(os.listdir(tmp))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
