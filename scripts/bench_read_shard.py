#!/usr/bin/env python3
"""Benchmark of the column-selected readers (device.read_table / device.read_mtx with cells=, DESIGN K26): one rank's share of
a file against the route the parent commit has for the same cells.  Prints ONE JSON line (and writes it with --out, default
profiles/bench_read_shard.json).

One run after a warm-up, all in this process, on the two files K21's and K22's benchmarks generate (the same seeds and
writers): the genes x cells TSV of integer counts and the matrix.mtx at --density.  The cells are those of rank --rank of a
cyclic deal over --world.  For each file, from the same run:
  selected    device.read_*(path, cells=mine)
  parent      device.read_*(path) followed by device.gather_matrix(x, cells=mine) / device.csc_select(counts, all genes, mine)
  (a) wall    seconds of both, timers off: three readings each, interleaved, every reading listed, the medians compared; before
              every reading the same bytes are read into one pinned buffer, 64 MiB at a time (the floor K21 and K22 took; six
              readings, the median reported).
              Condition: the selected median is not above the parent median by more than the spread (max - min) of the
              parent's three readings.
  (b) kernels milliseconds of the parse kernels by the library's event timers, one reading of each route with the timers on
  (c) memory  device bytes in use at the end of each route, result held, over what was in use before it, read from
              hipMemGetInfo (torch.cuda.mem_get_info): the counter covers the library's pool and torch's cache alike; both
              are emptied before the route and only grow during it, so the difference is the route's peak.
  equal       whether the two routes give the same bits."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from infercnv_amd import device, heatmap, sharded  # noqa: E402
from bench_read_mtx import floor_read, used_bytes, write_triplets  # noqa: E402

TABLE_KERNELS = ("col_map_check", "table_parse_structure", "table_parse_index", "table_parse_fields", "table_parse_collect",
                 "table_parse_transpose", "table_cols_index", "table_cols_rows", "table_cols_fields", "table_cols_collect", "gather_matrix")
MTX_KERNELS = ("col_map_check", "triplets_structure", "triplets_index", "triplets_parse", "triplets_keep_count", "triplets_keep_fill",
               "csc_build_check", "csc_build_colptr", "csc_select_count", "csc_select_fill")


def note(text):
    print(f"[bench_read_shard] {text}", file=sys.stderr, flush=True)


def timed(route, kernels=None):
    device.timing_enable(kernels is not None)
    device.timing_reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    result = route()
    torch.cuda.synchronize()
    out = {"wall_s": time.perf_counter() - t0}
    if kernels is not None:
        ms = {}
        for k in kernels:
            try:
                ms[k] = device.timing_get(k)[0]
            except Exception:                      # a kernel that never ran has no timer
                ms[k] = 0.0
        out["kernel_ms"] = {k: v for k, v in ms.items() if v}
        out["kernel_ms_total"] = sum(ms.values())
    device.timing_enable(False)
    return out, result


def peak_bytes(route):
    device.release_pool()
    torch.cuda.empty_cache()
    before = used_bytes()
    result = route()
    held = used_bytes() - before
    del result
    return held


def compare(path, selected, parent, same, kernels, repeats=3):
    _, a = timed(selected)                         # warm-up: code objects, pinned and device buffers, the page cache
    _, b = timed(parent)
    equal = bool(same(a, b))
    del a, b
    floor_read(path)
    sel_s, par_s, floors = [], [], []
    for _ in range(repeats):                       # floor, selected, floor, parent: both routes follow the same thing
        for route, into in ((selected, sel_s), (parent, par_s)):
            floors.append(floor_read(path))
            st, result = timed(route)
            del result
            into.append(st["wall_s"])
    med = lambda v: sorted(v)[len(v) // 2]
    spread = max(par_s) - min(par_s)
    out = {"file_bytes": os.path.getsize(path), "equal_bit_for_bit": equal,
           "selected_wall_s_of_every_reading": sel_s, "parent_wall_s_of_every_reading": par_s, "floor_s_of_every_reading": floors,
           "selected_wall_s": med(sel_s), "parent_wall_s": med(par_s), "floor_s": med(floors), "parent_spread_s": spread,
           "selected_over_parent": med(sel_s) / med(par_s), "selected_over_floor": med(sel_s) / med(floors),
           "selected_not_slower_than_parent_by_more_than_its_spread": bool(med(sel_s) <= med(par_s) + spread)}
    for name, route in (("selected", selected), ("parent", parent)):
        st, result = timed(route, kernels)
        del result
        out[name + "_kernel_ms"], out[name + "_kernel_ms_total"] = st["kernel_ms"], st["kernel_ms_total"]
    out["selected_peak_device_bytes"] = peak_bytes(selected)
    out["parent_peak_device_bytes"] = peak_bytes(parent)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=10000)
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--density", type=float, default=0.10)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--rank", type=int, default=3)
    ap.add_argument("--dir", default=None, help="directory on local disk for the files (default: the system's temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_read_shard.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_read_shard.py needs a GPU")
    torch.cuda.set_device(0)
    device.init(0)
    G, C = a.genes, a.cells
    mine = sharded.cyclic_cells(C, a.world, a.rank)
    genes, cells = [f"GENE{i}" for i in range(G)], [f"cell_{i:06d}" for i in range(C)]
    res = {"bench": "read_shard", "device": torch.cuda.get_device_name(0), "genes": G, "cells": C, "density": a.density, "deal": "cyclic",
           "world": a.world, "rank": a.rank, "cells_of_the_rank": int(mine.size), "memory_counter": "hipMemGetInfo (torch.cuda.mem_get_info)"}

    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        gen = torch.Generator(device="cuda").manual_seed(21)                  # K21's file
        counts = torch.floor(torch.empty((C, G), dtype=torch.float64, device="cuda").exponential_(0.4, generator=gen))
        tsv = os.path.join(tmp, "counts.tsv")
        heatmap.write_matrix(tsv, counts, np.arange(C, dtype=np.int32), "gene_rows", genes, cells, quote=False, sep="\t")
        del counts
        torch.cuda.empty_cache()
        note("TSV written")
        res["table"] = compare(tsv, lambda: device.read_table(tsv, cells=mine)[2],
                               lambda: device.gather_matrix(device.read_table(tsv)[2], cells=mine),
                               lambda x, y: torch.equal(x.view(torch.int64), y.view(torch.int64)), TABLE_KERNELS)
        os.remove(tsv)
        note("TSV measured")

        gen = torch.Generator(device="cuda").manual_seed(22)                  # K22's file
        dense = torch.floor(torch.empty((C, G), dtype=torch.float64, device="cuda").exponential_(0.05, generator=gen)) + 1
        dense *= torch.rand((C, G), generator=gen, device="cuda") < a.density
        col, row = torch.nonzero(dense, as_tuple=True)
        val = dense[col, row].long()
        del dense
        nnz = int(val.numel())
        mtx = os.path.join(tmp, "matrix.mtx")
        write_triplets(mtx, b"%%%%MatrixMarket matrix coordinate integer general\n%d %d %d\n" % (G, C, nnz), row, col, val)
        del row, col, val
        torch.cuda.empty_cache()
        note(f".mtx written: {nnz} entries")
        all_genes = np.arange(G)
        same = lambda x, y: all(torch.equal(s, t) for s, t in zip(x.t[1:], y.t[1:]))
        res["mtx"] = dict(compare(mtx, lambda: device.read_mtx(mtx, cells=mine)[0],
                                  lambda: device.csc_select(device.read_mtx(mtx)[0], all_genes, mine), same, MTX_KERNELS), entries=nnz)
        note(".mtx measured")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
