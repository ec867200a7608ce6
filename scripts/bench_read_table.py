#!/usr/bin/env python3
"""Benchmark of the table reader (icnv_parse_table_dev / device.read_table, DESIGN K21).  Prints ONE JSON line (and writes it
with --out, default profiles/bench_read_table.json).

One run after a warm-up, all in this process; the files are written by K20's formatter (heatmap.write_matrix) into --dir:
  counts      a genes x cells TSV of integer counts: seconds of device.read_table from the page cache (timers off; three
              readings, the median reported, every reading listed), GB/s of text, the reader's split (read_s in the reading
              thread; parse_s and stall_s in the calling thread), the share of fields parsed on the host, whether the reading
              equals the matrix the file was printed from; then a reading with the event timers on for the kernel
              milliseconds per pass.
  floor       in the same run, after each reading: the same bytes from the same file into one pinned buffer, 64 MiB at a
              time (the median).  Acceptance: counts.total_over_floor <= 1.5.
  decimals    the same for a file of 6-digit decimals with cells / 5 columns.
  gz          the counts slice below, gzip level 1: seconds and MB/s of text (bounded by the host's zlib; not tuned).
  cpu         on a genes x --slice slice of the counts: the restatement's per-token parse (tests/create_object_restate.py,
              str.split and float()) and numpy.loadtxt, numbers per second, EXTRAPOLATED as a rate to the full size.  The
              slice read by the library must equal the restatement bit for bit."""
import argparse
import gzip
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from infercnv_amd import device, heatmap  # noqa: E402

KERNELS = ("table_parse_structure", "table_parse_index", "table_parse_fields", "table_parse_collect", "table_parse_transpose")


def timed_read(path, timers):
    device.timing_enable(bool(timers))
    device.timing_reset()
    torch.cuda.synchronize()
    rows, cols, x, st = device.read_table(path)
    torch.cuda.synchronize()
    out = dict(st, file_bytes=os.path.getsize(path), shape=list(x.shape))
    out["GBps_of_text"] = out["file_bytes"] / st["wall_s"] / 1e9
    out["host_parsed_share"] = st["host_parsed"] / max(st["fields"], 1)
    if timers:
        kern = {}
        for k in KERNELS:
            try:
                kern[k] = device.timing_get(k)
            except Exception:                      # a kernel that never ran has no timer
                kern[k] = (0.0, 0)
        out["kernel_ms"] = {k: v[0] for k, v in kern.items()}
        out["kernel_launches"] = {k: v[1] for k, v in kern.items()}
    device.timing_enable(False)
    return out, x


def floor_read(path):
    buf = torch.empty(64 << 20, dtype=torch.uint8, pin_memory=True)
    view = memoryview(buf.numpy())
    t0 = time.perf_counter()
    with open(path, "rb", buffering=0) as f:
        while f.readinto(view):
            pass
    return time.perf_counter() - t0


def measure(path, written=None, repeats=3):
    """Warm-up, then `repeats` readings with the timers off, each followed by a floor reading of the same file; the ratio is
    taken on the medians.  written: the (n_cols, n_rows) tensor the file was printed from, when its text is exact."""
    timed_read(path, False)                        # warm-up: code objects, pinned and device buffers, the page cache
    floor_read(path)
    reads, floors, equal, differing = [], [], None, 0
    for _ in range(repeats):
        st, x = timed_read(path, False)
        if written is not None:
            equal = bool(torch.equal(x, written)) and equal is not False
            differing = max(differing, int((x != written).sum().item()))
        del x
        reads.append(st)
        floors.append(floor_read(path))
    traced, x = timed_read(path, True)
    del x
    walls = sorted(r["wall_s"] for r in reads)
    plain = next(r for r in reads if r["wall_s"] == walls[len(walls) // 2])
    floor_s = sorted(floors)[len(floors) // 2]
    out = {"read_table": plain, "wall_s_of_every_reading": [r["wall_s"] for r in reads], "floor_s_of_every_reading": floors,
           "with_timers": {k: traced[k] for k in ("wall_s", "parse_s", "kernel_ms", "kernel_launches")},
           "floor": {"seconds": floor_s, "GBps": plain["file_bytes"] / floor_s / 1e9}, "total_over_floor": plain["wall_s"] / floor_s}
    if written is not None:
        out["equals_the_written_matrix"] = equal
        out["values_that_differ_from_the_written_matrix"] = differing
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=10000)
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--slice", type=int, default=200, help="cells of the CPU baselines' slice")
    ap.add_argument("--dir", default=None, help="directory on local disk for the files (default: the system's temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_read_table.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_read_table.py needs a GPU")
    import create_object_restate as cor
    torch.cuda.set_device(0)
    device.init(0)
    G, C, S = a.genes, a.cells, min(a.slice, a.cells)
    gen = torch.Generator(device="cuda").manual_seed(21)
    genes, cells = [f"GENE{i}" for i in range(G)], [f"cell_{i:06d}" for i in range(C)]
    res = {"bench": "read_table", "device": torch.cuda.get_device_name(0), "genes": G, "cells": C,
           "chunk_bytes": int(os.environ.get("ICNV_READ_TABLE_CHUNK", device.READ_TABLE_CHUNK))}

    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        counts = torch.floor(torch.empty((C, G), dtype=torch.float64, device="cuda").exponential_(0.4, generator=gen))
        path = os.path.join(tmp, "counts.tsv")
        heatmap.write_matrix(path, counts, np.arange(C, dtype=np.int32), "gene_rows", genes, cells, quote=False, sep="\t")
        sl_path = os.path.join(tmp, "slice.tsv")
        heatmap.write_matrix(sl_path, counts, np.arange(S, dtype=np.int32), "gene_rows", genes, cells[:S], quote=False, sep="\t")
        res["counts"] = measure(path, written=counts)      # integer counts print exactly: the reading must give the matrix back
        del counts
        torch.cuda.empty_cache()
        os.remove(path)

        Cd = max(C // 5, 1)
        # a tensor divisor: torch multiplies by the reciprocal of a Python scalar, which is not the correctly rounded quotient
        dec = torch.randint(0, 1000000, (Cd, G), generator=gen, device="cuda").to(torch.float64) / torch.full((1,), 1000.0, dtype=torch.float64,
                                                                                                              device="cuda")
        path = os.path.join(tmp, "decimals.tsv")
        heatmap.write_matrix(path, dec, np.arange(Cd, dtype=np.int32), "gene_rows", genes, cells[:Cd], quote=False, sep="\t")
        res["decimals"] = dict(measure(path, written=dec), cells=Cd)    # k / 1000 with k < 10^6: at most 6 digits, printed exactly
        del dec
        torch.cuda.empty_cache()
        os.remove(path)

        # the CPU baselines and the bit check, on the slice
        rows, cols, x, _ = device.read_table(sl_path)
        t0 = time.perf_counter()
        r_rows, r_cols, r_bits = cor.read_table(sl_path)
        restate_s = time.perf_counter() - t0
        same = rows == r_rows and cols == r_cols and bool(np.array_equal(x.cpu().numpy().view(np.int64), r_bits.T))
        t0 = time.perf_counter()
        lt = np.loadtxt(sl_path, delimiter="\t", skiprows=1, usecols=range(1, S + 1), ndmin=2)
        loadtxt_s = time.perf_counter() - t0
        same_lt = bool(np.array_equal(lt.view(np.int64), r_bits))
        res["cpu"] = {"slice": [G, S], "extrapolated": True, "library_equals_restatement": same, "loadtxt_equals_restatement": same_lt,
                      "restatement": {"seconds": restate_s, "numbers_per_s": G * S / restate_s,
                                      "seconds_extrapolated_as_a_rate_to_full_size": restate_s * C / S},
                      "numpy_loadtxt": {"seconds": loadtxt_s, "numbers_per_s": G * S / loadtxt_s,
                                        "seconds_extrapolated_as_a_rate_to_full_size": loadtxt_s * C / S}}
        gz_path = sl_path + ".gz"
        with open(sl_path, "rb") as src, gzip.open(gz_path, "wb", compresslevel=1) as dst:
            dst.write(src.read())
        device.read_table(gz_path)
        t0 = time.perf_counter()
        _, _, xg, _ = device.read_table(gz_path)
        torch.cuda.synchronize()
        gz_s = time.perf_counter() - t0
        res["gz"] = {"slice": [G, S], "text_bytes": os.path.getsize(sl_path), "seconds": gz_s,
                     "MBps_of_text": os.path.getsize(sl_path) / gz_s / 1e6, "equals_plain": bool(torch.equal(xg, x))}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
