#!/usr/bin/env python3
"""Benchmark of the MatrixMarket reader and the sparse route (device.read_mtx, CreateInfercnvObject(sparse), DESIGN K22).  Prints
ONE JSON line (and writes it with --out, default profiles/bench_read_mtx.json).

One run after a warm-up, all in this process; a seeded genes x cells integer matrix at --density is written into --dir once as
matrix.mtx in column-major order (what 10x writes), once shuffled, and once as a dense TSV by K20's formatter:
  sorted      seconds of device.read_mtx from the page cache (timers off; three readings, the median reported, every reading
              listed), GB/s of text, the reader's split, whether the reading equals the matrix written; then a reading with
              the event timers on for the kernel milliseconds per pass.
  floor       in the same run, after each reading: the same bytes from the same file into one pinned buffer, 64 MiB at a time
              (the median) -- the floor K21 used.  Target: sorted.total_over_floor <= 1.25.
  shuffled    the same entries in a seeded random order: the route through torch.sort.
  scipy       scipy.io.mmread of the sorted file, once.
  object      CreateInfercnvObject + device.ingest_counts from the .mtx and from the dense TSV of the same matrix (once each,
              after one warm-up each): seconds, the bytes that cross PCIe on each route computed from the shapes, whether the
              two log-scale matrices are equal bit for bit, and the device memory the sparse route holds at its end on top of
              what was held before it (the library's pool and torch's cache only grow during it, so this is its peak)."""
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

import infercnv_amd  # noqa: E402
from infercnv_amd import device, heatmap  # noqa: E402

KERNELS = ("triplets_structure", "triplets_index", "triplets_parse", "csc_build_check", "csc_build_colptr")


def digits(v, width):
    """(n, width) uint8 digits of the non-negative int64 tensor v, right-aligned, and the mask of the digits that count."""
    pos = torch.arange(width - 1, -1, -1, device=v.device)
    d = (v[:, None] // (10 ** pos)[None, :]) % 10
    n = torch.clamp(torch.floor(torch.log10(v.clamp(min=1).double())).long() + 1, min=1)
    n = n + ((10 ** n.clamp(max=18)) <= v).long() - ((10 ** (n - 1).clamp(min=0)) > v.clamp(min=1)).long()     # log10 rounds: settle it exactly
    return (d + 48).to(torch.uint8), pos[None, :] < n[:, None]


def write_triplets(path, banner, row, col, val, block=4_000_000):
    """`i j v` lines (1-based) of the int64 CUDA tensors, formatted on the device block by block."""
    with open(path, "wb") as f:
        f.write(banner)
        for a in range(0, row.numel(), block):
            parts, masks = [], []
            for v, w, end in ((row[a:a + block] + 1, 10, 32), (col[a:a + block] + 1, 10, 32), (val[a:a + block], 10, 10)):
                d, m = digits(v, w)
                parts += [d, torch.full((v.numel(), 1), end, dtype=torch.uint8, device=v.device)]
                masks += [m, torch.ones((v.numel(), 1), dtype=torch.bool, device=v.device)]
            f.write(torch.cat(parts, 1)[torch.cat(masks, 1)].cpu().numpy().tobytes())


def timed_read(path, timers):
    device.timing_enable(bool(timers))
    device.timing_reset()
    torch.cuda.synchronize()
    counts, st = device.read_mtx(path)
    torch.cuda.synchronize()
    out = dict(st, file_bytes=os.path.getsize(path))
    out["GBps_of_text"] = out["file_bytes"] / st["wall_s"] / 1e9
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
    return out, counts


def floor_read(path):
    buf = torch.empty(64 << 20, dtype=torch.uint8, pin_memory=True)
    view = memoryview(buf.numpy())
    t0 = time.perf_counter()
    with open(path, "rb", buffering=0) as f:
        while f.readinto(view):
            pass
    return time.perf_counter() - t0


def measure(path, written, repeats=3):
    """Warm-up, then `repeats` readings with the timers off, each followed by a floor reading of the same file; the ratio is
    taken on the medians.  written: the (C, G) float64 tensor the file was printed from."""
    timed_read(path, False)
    floor_read(path)
    reads, floors, equal = [], [], True
    for _ in range(repeats):
        st, counts = timed_read(path, False)
        equal = equal and bool(torch.equal(counts.to_dense(), written))
        del counts
        reads.append(st)
        floors.append(floor_read(path))
    traced, counts = timed_read(path, True)
    del counts
    walls = sorted(r["wall_s"] for r in reads)
    plain = next(r for r in reads if r["wall_s"] == walls[len(walls) // 2])
    floor_s = sorted(floors)[len(floors) // 2]
    return {"read_mtx": plain, "wall_s_of_every_reading": [r["wall_s"] for r in reads], "floor_s_of_every_reading": floors,
            "with_timers": {k: traced[k] for k in ("wall_s", "parse_s", "kernel_ms", "kernel_launches")},
            "floor": {"seconds": floor_s, "GBps": plain["file_bytes"] / floor_s / 1e9}, "total_over_floor": plain["wall_s"] / floor_s,
            "equals_the_written_matrix": equal}


def note(text):
    print(f"[bench_read_mtx] {text}", file=sys.stderr, flush=True)


def used_bytes():
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    return total - free


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=10000)
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--density", type=float, default=0.10)
    ap.add_argument("--dir", default=None, help="directory on local disk for the files (default: the system's temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_read_mtx.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_read_mtx.py needs a GPU")
    torch.cuda.set_device(0)
    device.init(0)
    G, C = a.genes, a.cells
    gen = torch.Generator(device="cuda").manual_seed(22)
    res = {"bench": "read_mtx", "device": torch.cuda.get_device_name(0), "genes": G, "cells": C, "density": a.density,
           "chunk_bytes": int(os.environ.get("ICNV_READ_MTX_CHUNK", device.READ_MTX_CHUNK))}
    genes, cells = [f"GENE{i}" for i in range(G)], [f"cell_{i:06d}" for i in range(C)]
    order = [(g, f"chr{1 + i * 22 // G}", 1000 * i + 1, 1000 * i + 900) for i, g in enumerate(genes)]
    annot = [(c, "normal" if j % 4 == 0 else "tumor") for j, c in enumerate(cells)]

    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        dense = torch.floor(torch.empty((C, G), dtype=torch.float64, device="cuda").exponential_(0.05, generator=gen)) + 1
        dense *= torch.rand((C, G), generator=gen, device="cuda") < a.density
        col, row = torch.nonzero(dense, as_tuple=True)                 # row-major over (C, G): column-major order of the G x C matrix
        val = dense[col, row].long()
        nnz = int(val.numel())
        res["entries"] = nnz
        banner = b"%%%%MatrixMarket matrix coordinate integer general\n%d %d %d\n" % (G, C, nnz)
        path, shuffled = os.path.join(tmp, "matrix.mtx"), os.path.join(tmp, "shuffled.mtx")
        write_triplets(path, banner, row, col, val)
        perm = torch.randperm(nnz, generator=gen, device="cuda")
        write_triplets(shuffled, banner, row[perm], col[perm], val[perm])
        del row, col, val, perm
        note(f"files written: {nnz} entries")
        res["sorted"] = measure(path, dense)
        note("sorted file read")
        res["shuffled"] = measure(shuffled, dense)
        note("shuffled file read")
        os.remove(shuffled)

        import scipy.io
        t0 = time.perf_counter()
        m = scipy.io.mmread(path)
        res["scipy_mmread"] = {"seconds": time.perf_counter() - t0, "entries": int(m.nnz)}
        del m
        note("scipy.io.mmread done")

        tsv = os.path.join(tmp, "counts.tsv")
        heatmap.write_matrix(tsv, dense, np.arange(C, dtype=np.int32), "gene_rows", genes, cells, quote=False, sep="\t")
        del dense
        torch.cuda.empty_cache()

        def sparse_route():
            obj, counts = infercnv_amd.CreateInfercnvObject(path, order, annot, ["normal"], gene_names=genes, cell_names=cells, return_device=True)
            x, keep, factor = device.ingest_counts(counts)
            torch.cuda.synchronize()
            return obj, x, counts.nnz

        def dense_route():
            obj, x = infercnv_amd.CreateInfercnvObject(tsv, order, annot, ["normal"], return_device=True)
            counts = device.DeviceCounts(x.shape[1], x.shape[0], dense=x.to(torch.int32).contiguous())
            x, keep, factor = device.ingest_counts(counts)
            torch.cuda.synchronize()
            return obj, x, None

        out = {}
        for name, route in (("mtx", sparse_route), ("tsv", dense_route)):
            route()                                                    # warm-up
            device.release_pool()
            torch.cuda.empty_cache()
            before = used_bytes()
            t0 = time.perf_counter()
            obj, x, kept = route()
            out[name] = {"seconds": time.perf_counter() - t0, "device_bytes_held_at_the_end_over_before": used_bytes() - before,
                         "file_bytes": os.path.getsize(path if name == "mtx" else tsv)}
            note(f"route {name} done")
            g, c = obj.expr_data.shape
            out[name]["pcie_bytes_from_shapes"] = ({"h2d_text": out[name]["file_bytes"], "d2h_csc": 8 * kept + 8 * (c + 1), "d2h_col_sums": 8 * C}
                                                   if name == "mtx" else
                                                   {"h2d_text": out[name]["file_bytes"], "d2h_matrix": 8 * g * c, "d2h_col_sums": 8 * C})
            out[name + "_x"] = x
            del obj
        out["log_matrices_equal_bit_for_bit"] = bool(torch.equal(out.pop("mtx_x").view(torch.int64), out.pop("tsv_x").view(torch.int64)))
        res["object"] = out
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
