#!/usr/bin/env python3
"""Benchmark of the matrix-file writer (icnv_format_table_dev / heatmap.write_matrix, DESIGN K20).  Prints ONE JSON line (and
writes it with --out, default profiles/bench_table_text.json).

One run after a warm-up, all in this process:
  writer       `<name>.observations.txt` of a clamped N(1, 0.1) matrix, genes x cells in a permuted cell order, quoted names, into a
               file in --dir: seconds, GB/s of text, and the split -- seconds inside the library (format_s, of which the digits,
               lengths and emit kernels by their event timers), the writer thread waiting for a device-to-host copy
               (copy_wait_s) and inside f.write (write_s), the formatting thread waiting for a free buffer (stall_s).  Formatting
               runs on one thread, copies and writes on another: wall_s is about max(format_s + stall_s, copy_wait_s + write_s).
  floors       in the same run: a read-only stream of the matrix (torch.sum), a device-to-host copy of as many bytes as the file
               has (256 MiB pieces into one pinned buffer), writing that many bytes from the pinned buffer to the same directory.
  write_table  the host writer (heatmap.write_table, r_num per number) on a genes x 200 slice of the same matrix: numbers per
               second, EXTRAPOLATED as a rate to the full size.  The slice's file must equal write_matrix's byte for byte.
  fallback     elements of the full file that the host formatted."""
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

from infercnv_amd import device, heatmap  # noqa: E402

KERNELS = ("table_text_digits", "table_text_lengths", "table_text_emit", "table_text_collect")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=10000)
    ap.add_argument("--cells", type=int, default=45000)
    ap.add_argument("--slice", type=int, default=200, help="cells of the write_table slice")
    ap.add_argument("--dir", default=None, help="directory on local disk for the files (default: the system's temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_table_text.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_table_text.py needs a GPU")
    torch.cuda.set_device(0)
    device.init(0)
    G, C, S = a.genes, a.cells, min(a.slice, a.cells)
    gen = torch.Generator(device="cuda").manual_seed(20)
    x = torch.normal(1.0, 0.1, (C, G), generator=gen, device="cuda", dtype=torch.float64).clamp_(0.75, 1.25)
    order = np.random.default_rng(20).permutation(C).astype(np.int32)
    genes, cells = [f"GENE{i}" for i in range(G)], [f"cell_{i:06d}" for i in range(C)]
    res = {"bench": "table_text", "device": torch.cuda.get_device_name(0), "genes": G, "cells": C,
           "chunk_bytes": int(os.environ.get("ICNV_TABLE_TEXT_CHUNK", heatmap.TABLE_TEXT_CHUNK))}

    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        path = os.path.join(tmp, "infercnv.observations.txt")
        # warm-up and the byte check against the host writer, on a slice
        sl = order[:S]
        heatmap.write_matrix(os.path.join(tmp, "slice_gpu.txt"), x, sl, "gene_rows", genes, [cells[c] for c in sl])
        host = x[torch.from_numpy(sl.astype(np.int64)).cuda()].cpu().numpy()          # (S, G)
        rows = host.T.tolist()
        t0 = time.perf_counter()
        heatmap.write_table(os.path.join(tmp, "slice_host.txt"), rows, genes, [cells[c] for c in sl])
        wt_s = time.perf_counter() - t0
        same = open(os.path.join(tmp, "slice_gpu.txt"), "rb").read() == open(os.path.join(tmp, "slice_host.txt"), "rb").read()
        res["write_table"] = {"slice": [G, S], "seconds": wt_s, "numbers_per_s": G * S / wt_s,
                              "seconds_extrapolated_as_a_rate_to_full_size": wt_s * C / S, "extrapolated": True,
                              "list_of_lists_not_timed": True, "slice_file_equals_write_matrix": bool(same)}
        del rows, host

        device.timing_enable(True)
        device.timing_reset()
        device.table_text_stats(reset=True)
        torch.cuda.synchronize()
        st = heatmap.write_matrix(path, x, order, "gene_rows", genes, [cells[c] for c in order])
        torch.cuda.synchronize()
        kern = {}
        for k in KERNELS:
            try:
                kern[k] = device.timing_get(k)
            except Exception:                      # a kernel that never ran has no timer
                kern[k] = (0.0, 0)
        device.timing_enable(False)
        tt = device.table_text_stats()
        nbytes = os.path.getsize(path)
        res["writer"] = dict(st, file_bytes=nbytes, GBps_of_text=nbytes / st["wall_s"] / 1e9, numbers_per_s=G * C / st["wall_s"],
                             kernel_ms={k: v[0] for k, v in kern.items()}, kernel_launches={k: v[1] for k, v in kern.items()},
                             library_wall_s=tt["us"] / 1e6, calls=tt["calls"])
        res["fallback"] = {"host_formatted": tt["host_formatted"], "elements": tt["elements"], "collect_rounds": tt["collect_rounds"]}
        os.remove(path)

        # the floors
        torch.sum(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        torch.sum(x)
        torch.cuda.synchronize()
        read_s = time.perf_counter() - t0
        piece = min(nbytes, 256 << 20)
        d_buf = torch.zeros(piece, dtype=torch.uint8, device="cuda")
        h_buf = torch.empty(piece, dtype=torch.uint8, pin_memory=True)
        h_buf.copy_(d_buf)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        left = nbytes
        while left > 0:
            n = min(piece, left)
            h_buf[:n].copy_(d_buf[:n], non_blocking=True)
            left -= n
        torch.cuda.synchronize()
        d2h_s = time.perf_counter() - t0
        view = memoryview(h_buf.numpy())
        t0 = time.perf_counter()
        with open(os.path.join(tmp, "floor.bin"), "wb") as f:
            left = nbytes
            while left > 0:
                n = min(piece, left)
                f.write(view[:n])
                left -= n
        disk_s = time.perf_counter() - t0
        floors = {"matrix_read_s": read_s, "d2h_copy_s": d2h_s, "file_write_s": disk_s}
        slowest = max(floors, key=floors.get)
        res["floors"] = dict(floors, matrix_read_TBps=8.0 * G * C / read_s / 1e12, d2h_GBps=nbytes / d2h_s / 1e9,
                             file_write_GBps=nbytes / disk_s / 1e9, slowest=slowest, writer_over_slowest=st["wall_s"] / floors[slowest])
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
