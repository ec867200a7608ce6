#!/usr/bin/env python3
"""Benchmark of writing and reading an infercnv object as .rds (infercnv_amd.rds, icnv_xdr_encode_dev / icnv_xdr_decode_dev,
DESIGN K27).  Prints ONE JSON line (and writes it with --out, default profiles/bench_rds.json).

A genes x cells object (default 10 000 x 50 000: 4 GB of expr.data) with gene and cell names and nothing else of size.  All
timings in one run, one warm-up, then medians of --repeats:
  from_host      save_infercnv_obj from the host array: wall seconds, split into the upload, the kernels (event timers), the
                 writer thread's wait for the device-to-host copies and its f.write.
  from_x_dev     the same with x_dev=, the (cells, genes) matrix where the chain leaves it: nothing uploaded or transposed.
  floor          writing as many bytes as the file holds from a pinned buffer to the same directory -- the floor the matrix
                 files (K20) and the CNV reports (K24) were held to.  The bar is from_x_dev within 1.25 x of it.
  host_baseline  np.asfortranarray(x).astype(">f8") followed by tofile on a slice of --slice cells, EXTRAPOLATED as a rate to
                 the full size.
  load           load_infercnv_obj(return_device=True) of the file just written (from the page cache), and the check that
                 the loaded device matrix holds the bits that were saved."""
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

from infercnv_amd import device, load_infercnv_obj, rds, save_infercnv_obj  # noqa: E402
from infercnv_amd.infercnv_object import GeneOrder, InfercnvObject  # noqa: E402


def timed_save(obj, path, x_dev, repeats):
    rows = []
    for i in range(repeats + 1):
        device.timing_enable(True)
        device.timing_reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stats = save_infercnv_obj(obj, path, x_dev=x_dev)
        wall = time.perf_counter() - t0
        kernels_ms = device.timing_get("xdr_encode")[0]
        device.timing_enable(False)
        big = max(stats, key=lambda s: s["bytes"])
        if i:
            rows.append({"wall_s": wall, "upload_s": big["upload_s"], "kernels_s": kernels_ms / 1e3, "stream_wall_s": big["wall_s"],
                         "encode_calls_s": big["format_s"], "stall_s": big["stall_s"], "d2h_copy_wait_s": big["copy_wait_s"],
                         "f_write_s": big["write_s"], "chunks": big["chunks"]})
    med = {k: statistics.median(r[k] for r in rows) for k in rows[0]}
    med["file_bytes"] = os.path.getsize(path)
    med["GBps"] = med["file_bytes"] / med["wall_s"] / 1e9
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=10000)
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--slice", type=int, default=2000, help="cells of the host baseline's slice")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dir", default=None, help="directory on local disk for the files (default: the system's temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_rds.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rds.py needs a GPU")
    torch.cuda.set_device(0)
    device.init(0)
    G, C = a.genes, a.cells
    gen = torch.Generator(device="cuda").manual_seed(27)
    x_dev = torch.randn((C, G), dtype=torch.float64, device="cuda", generator=gen)
    x = np.ascontiguousarray(x_dev.cpu().numpy().T)                      # the object's host array: row-major genes x cells
    n_ref = max(C // 10, 1)
    obj = InfercnvObject(expr_data=x, gene_order=GeneOrder(np.repeat([f"chr{k + 1}" for k in range(22)], -(-G // 22))[:G],
                                                           np.arange(G) * 50000 + 1, np.arange(G) * 50000 + 30001),
                         reference_grouped_cell_indices={"normal": np.arange(C - n_ref, C)},
                         observation_grouped_cell_indices={"tumor": np.arange(C - n_ref)},
                         gene_names=np.array([f"GENE{i}" for i in range(G)]), cell_names=np.array([f"cell_{i:06d}" for i in range(C)]))
    res = {"bench": "rds", "device": torch.cuda.get_device_name(0), "genes": G, "cells": C, "payload_bytes": G * C * 8,
           "chunk_bytes": rds.CHUNK_BYTES, "repeats": a.repeats}

    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        path = os.path.join(tmp, "bench.infercnv_obj")
        blind = obj.copy()
        blind.expr_data = None
        res["from_x_dev"] = timed_save(blind, path, x_dev, a.repeats)

        loads = []
        for i in range(a.repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            back, back_dev = load_infercnv_obj(path, return_device=True)
            torch.cuda.synchronize()
            loads.append(time.perf_counter() - t0)
            same = bool(torch.equal(back_dev.view(torch.int64), x_dev.view(torch.int64)))
            del back_dev
        res["load"] = {"return_device_s": statistics.median(loads[1:]), "from_page_cache": True, "device_matrix_equals_saved_bits": same,
                       "GBps": os.path.getsize(path) / statistics.median(loads[1:]) / 1e9}
        x_dev_file_head = open(path, "rb").read(1 << 24)

        res["from_host"] = timed_save(obj, path, None, a.repeats)
        res["from_host"]["file_equals_x_dev_file"] = bool(res["from_host"]["file_bytes"] == res["from_x_dev"]["file_bytes"]
                                                          and open(path, "rb").read(1 << 24) == x_dev_file_head)
        nbytes = res["from_x_dev"]["file_bytes"]
        os.remove(path)

        # the floor: as many bytes from a pinned buffer to the same directory
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
        os.remove(os.path.join(tmp, "floor.bin"))
        floor_s = statistics.median(floor[1:])
        res["floor"] = {"file_write_s": floor_s, "file_write_GBps": nbytes / floor_s / 1e9,
                        "from_x_dev_over_floor": res["from_x_dev"]["wall_s"] / floor_s, "from_host_over_floor": res["from_host"]["wall_s"] / floor_s,
                        "bar": 1.25, "from_x_dev_within_bar": bool(res["from_x_dev"]["wall_s"] <= 1.25 * floor_s)}

        # the host baseline on a slice of the cells, as a rate
        n = min(a.slice, C)
        sl = x[:, :n]
        base = []
        for _ in range(a.repeats + 1):
            t0 = time.perf_counter()
            be = np.asfortranarray(sl).astype(">f8")
            with open(os.path.join(tmp, "host.bin"), "wb") as f:
                be.T.tofile(f)                                             # the Fortran array's memory order: column after column
            base.append(time.perf_counter() - t0)
        os.remove(os.path.join(tmp, "host.bin"))
        base_s = statistics.median(base[1:])
        full = base_s * (C / n)
        res["host_baseline"] = {"slice_cells": n, "seconds": base_s, "GBps": G * n * 8 / base_s / 1e9,
                                "seconds_extrapolated_as_a_rate_to_full_size": full, "extrapolated": True}
        res["ratio_to_host_baseline_rate"] = {"from_x_dev": full / res["from_x_dev"]["wall_s"], "from_host": full / res["from_host"]["wall_s"]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
