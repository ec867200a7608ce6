#!/usr/bin/env python3
"""Benchmark of the CNV region reports (cnv_regions.generate_cnv_region_reports, icnv_cnv_report_*, DESIGN K24).  Prints ONE
JSON line (and writes it with --out, default profiles/bench_cnv_reports.json).

Synthetic i6 states, genes x cells, neutral state 3, with --share of the genes of every cell in non-neutral runs of 20-60 genes;
by = "cell", ignore_neutral_state = 3, as run() calls it with analysis_mode = "cells".  One warm-up, then medians of three:
  reports      total seconds of generate_cnv_region_reports, bytes written, and its parts: the uint8 conversion and upload,
               consensus / runs, the two .dat files (of which the kernels by their event timers, the device-to-host copy wait
               and f.write of the writer thread), the small files.
  floor        in the same run: writing as many bytes as the two .dat files hold from a pinned buffer to the same directory.
  host_writer  the parent's writer (_generate_cnv_region_reports_host) on a slice of --slice cells: lines per second,
               EXTRAPOLATED as a rate to the full size.  The slice's files must equal the device writer's byte for byte.
  subcluster   the same states with by = "subcluster" and --groups groups."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from infercnv_amd import cnv_regions, device  # noqa: E402
from infercnv_amd.infercnv_object import GeneOrder, InfercnvObject  # noqa: E402

KERNELS = ("cnv_report_prefix", "cnv_report_lengths", "cnv_report_scan", "cnv_report_emit")
SUFFIXES = (".cell_groupings", ".pred_cnv_regions.dat", ".pred_cnv_genes.dat", ".genes_used.dat")


def make_object(G, C, share, n_groups, seed=24):
    rng = np.random.default_rng(seed)
    n_chr = 22
    sizes = np.full(n_chr, G // n_chr)
    sizes[: G - sizes.sum()] += 1
    chrs = np.concatenate([np.full(n, f"chr{k + 1}") for k, n in enumerate(sizes)])
    pos = np.concatenate([np.arange(n) * 50000 + 1 for n in sizes])
    states = np.full((G, C), 3.0)
    runs = max(int(round(share * G / 40)), 0)                 # runs of 20-60 genes, 40 on average
    for c in range(C):
        for a, n, s in zip(rng.integers(0, G - 60, runs), rng.integers(20, 61, runs), rng.choice([1, 2, 4, 5, 6], runs)):
            states[a:a + n, c] = s
    n_ref = max(C // 10, 1)
    obs, ref = np.arange(C - n_ref, dtype=np.int32), np.arange(C - n_ref, C, dtype=np.int32)
    subs = {"tumor": {f"tumor_s{q + 1}": p for q, p in enumerate(np.array_split(obs, max(n_groups - 1, 1)))}, "normal": {"normal_s1": ref}}
    return InfercnvObject(expr_data=states, gene_order=GeneOrder(chr=chrs, start=pos, stop=pos + 30000),
                          reference_grouped_cell_indices={"normal": ref}, observation_grouped_cell_indices={"tumor": obs},
                          tumor_subclusters={"subclusters": subs}, gene_names=np.array([f"GENE{i}" for i in range(G)]),
                          cell_names=np.array([f"cell_{i:06d}" for i in range(C)]))


def slice_object(obj, n):
    """The first n // 2 observation and the first n - n // 2 reference cells as an object of their own."""
    obs = obj.observation_grouped_cell_indices["tumor"][: n // 2]
    ref = obj.reference_grouped_cell_indices["normal"][: n - n // 2]
    keep = np.concatenate([obs, ref])
    o, r = np.arange(obs.size, dtype=np.int32), np.arange(obs.size, keep.size, dtype=np.int32)
    return InfercnvObject(expr_data=np.ascontiguousarray(obj.expr_data[:, keep]), gene_order=obj.gene_order,
                          reference_grouped_cell_indices={"normal": r}, observation_grouped_cell_indices={"tumor": o},
                          tumor_subclusters={"subclusters": {"tumor": {"tumor_s1": o}, "normal": {"normal_s1": r}}},
                          gene_names=obj.gene_names, cell_names=obj.cell_names[keep])


def timed_reports(obj, tmp, by, repeats):
    """Medians over `repeats` runs after one warm-up: the parts of LAST_REPORT_STATS, the kernels' event timers, the sizes."""
    runs = []
    for i in range(repeats + 1):
        device.timing_enable(True)
        device.timing_reset()
        device.cnv_report_stats(reset=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cnv_regions.generate_cnv_region_reports(obj, "bench", tmp, ignore_neutral_state=3, by=by)
        total = time.perf_counter() - t0
        kern = {}
        for k in KERNELS:
            try:
                kern[k] = device.timing_get(k)[0]
            except Exception:                      # a kernel that never ran has no timer
                kern[k] = 0.0
        device.timing_enable(False)
        st, lib = dict(cnv_regions.LAST_REPORT_STATS), device.cnv_report_stats()
        streams = [st.get(k, {}) for k in ("regions", "genes")]
        row = {"total_s": total, "convert_upload_s": st["convert_upload_s"], "consensus_runs_s": st["runs_s"],
               "regions_file_s": st["regions_s"], "genes_file_s": st["genes_s"], "genes_used_file_s": st["genes_used_s"],
               "kernels_s": sum(kern.values()) / 1e3, "library_format_wall_s": lib["us"] / 1e6,
               "format_s": sum(s.get("format_s", 0.0) for s in streams), "stall_s": sum(s.get("stall_s", 0.0) for s in streams),
               "d2h_copy_wait_s": sum(s.get("copy_wait_s", 0.0) for s in streams), "f_write_s": sum(s.get("write_s", 0.0) for s in streams)}
        row.update({"kernel_ms_" + k: v for k, v in kern.items()})
        if i:                                      # the first run is the warm-up
            runs.append(row)
    med = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
    sizes = {s: os.path.getsize(os.path.join(tmp, "bench" + s)) for s in SUFFIXES}
    med.update(bytes_written=sum(sizes.values()), dat_bytes=sizes[".pred_cnv_regions.dat"] + sizes[".pred_cnv_genes.dat"], file_bytes=sizes,
               records=lib["records"] // 2, lines=lib["lines"], format_calls=lib["calls"], repeats=repeats)
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=10000)
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--share", type=float, default=0.1, help="share of a cell's genes in non-neutral runs")
    ap.add_argument("--slice", type=int, default=200, help="cells of the host writer's slice")
    ap.add_argument("--groups", type=int, default=300, help="groups of the by = subcluster run")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dir", default=None, help="directory on local disk for the files (default: the system's temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_cnv_reports.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cnv_reports.py needs a GPU")
    torch.cuda.set_device(0)
    device.init(0)
    G, C = a.genes, a.cells
    obj = make_object(G, C, a.share, a.groups)
    res = {"bench": "cnv_reports", "device": torch.cuda.get_device_name(0), "genes": G, "cells": C, "non_neutral_share": a.share,
           "chunk_bytes": int(os.environ.get("ICNV_CNV_REPORT_CHUNK", cnv_regions.REPORT_CHUNK))}

    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        # the parent's writer on a slice, and the byte check
        sl = slice_object(obj, min(a.slice, C))
        cnv_regions.generate_cnv_region_reports(sl, "slice_dev", tmp, ignore_neutral_state=3, by="cell")
        t0 = time.perf_counter()
        cnv_regions._generate_cnv_region_reports_host(sl, "slice_host", tmp, ignore_neutral_state=3, by="cell")
        host_s = time.perf_counter() - t0
        same = all(open(os.path.join(tmp, "slice_dev" + s), "rb").read() == open(os.path.join(tmp, "slice_host" + s), "rb").read() for s in SUFFIXES)
        sl_lines = sum(open(os.path.join(tmp, "slice_host" + s), "rb").read().count(b"\n") for s in SUFFIXES)

        cell = timed_reports(obj, tmp, "cell", a.repeats)
        res["reports"] = cell
        all_lines = cell["lines"] + C + G + 4
        res["host_writer"] = {"slice_cells": sl.expr_data.shape[1], "seconds": host_s, "lines": sl_lines, "lines_per_s": sl_lines / host_s,
                              "seconds_extrapolated_as_a_rate_to_full_size": all_lines / (sl_lines / host_s), "extrapolated": True,
                              "slice_files_equal_device_writer": bool(same)}
        res["ratio_to_host_writer_rate"] = res["host_writer"]["seconds_extrapolated_as_a_rate_to_full_size"] / cell["total_s"]

        # the floor: as many bytes as the two .dat files, from a pinned buffer, to the same directory
        nbytes = cell["dat_bytes"]
        piece = max(min(nbytes, 256 << 20), 1)
        view = memoryview(torch.zeros(piece, dtype=torch.uint8).pin_memory().numpy())
        floor = []
        for _ in range(a.repeats + 1):
            t0 = time.perf_counter()
            with open(os.path.join(tmp, "floor.bin"), "wb") as f:
                left = nbytes
                while left > 0:
                    n = min(piece, left)
                    f.write(view[:n])
                    left -= n
            floor.append(time.perf_counter() - t0)
        floor_s = statistics.median(floor[1:])
        os.remove(os.path.join(tmp, "floor.bin"))
        dat_s = cell["regions_file_s"] + cell["genes_file_s"]
        parts = {k: cell[k] for k in ("convert_upload_s", "consensus_runs_s", "kernels_s", "d2h_copy_wait_s", "f_write_s", "genes_used_file_s")}
        res["floor"] = {"file_write_s": floor_s, "file_write_GBps": nbytes / floor_s / 1e9, "dat_files_s": dat_s,
                        "dat_files_over_floor": dat_s / floor_s, "total_over_floor": cell["total_s"] / floor_s,
                        "largest_part": max(parts, key=parts.get)}

        res["subcluster"] = timed_reports(obj, tmp, "subcluster", a.repeats)
        res["subcluster"]["groups"] = a.groups
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
