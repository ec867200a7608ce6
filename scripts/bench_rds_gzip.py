#!/usr/bin/env python3
"""Benchmark of writing a gzip-compressed .rds from the device (infercnv_amd.rds.GzipAssembler, icnv_deflate_pieces_dev /
icnv_deflate_pack_dev, DESIGN K28).  Prints ONE JSON line (and writes it with --out, default profiles/bench_rds_gzip.json).

A genes x cells object (default 10 000 x 50 000) with a denoised-like expr.data on the device (N(1, 0.05) with the 1.5 sd band
set to 1.0) and a count-like count.data on the host (Poisson 0.15 as doubles), 4 GB each.  All timings in one process, one
warm-up, then medians of --repeats, the two saves alternating:
  compressed     save_infercnv_obj(compress=True, x_dev=): wall seconds, the file's size, pieces and stored pieces, the seconds
                 inside the deflate calls.
  uncompressed   the same object with compress=False -- the route this change leaves as it was.  THE TARGET: compressed wall <=
                 uncompressed wall in the same run (a margin of 1.0 x).
  floor          writing as many bytes as the compressed file holds from a pinned buffer to the same directory.
  smoothed       the same pair of saves for an object whose only matrix is N(1, 0.05): compression buys little there.
  kernels        per kind of data (denoised, counts, smoothed, HMM states), on a --slice-mb slice of its XDR stream: the time of
                 icnv_deflate_pieces_dev and of icnv_deflate_pack_dev between device events (median of --repeats after a
                 warm-up), input GB/s, the packed size, and zlib level 1 and level 6 on the same slice (host, one thread).
  gzipfile_host  the host route (compress=True, device=False: Python's GzipFile) on --gz-cells cells of both matrices,
                 EXTRAPOLATED as a rate to the full size and labelled so."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from infercnv_amd import device, rds, save_infercnv_obj  # noqa: E402
from infercnv_amd.infercnv_object import GeneOrder, InfercnvObject  # noqa: E402


def median_of(rows):
    return {k: statistics.median(r[k] for r in rows) for k in rows[0]}


def timed_pair(obj, x_dev, tmp, repeats):
    """Medians of the compressed and the uncompressed save of one object, alternating, after one warm-up of each."""
    comp, plain = [], []
    paths = os.path.join(tmp, "c.infercnv_obj"), os.path.join(tmp, "p.infercnv_obj")
    for i in range(repeats + 1):
        for compress, rows, path in ((True, comp, paths[0]), (False, plain, paths[1])):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stats = save_infercnv_obj(obj, path, x_dev=x_dev, compress=compress)
            wall = time.perf_counter() - t0
            if i:
                row = {"wall_s": wall, "file_bytes": os.path.getsize(path), "f_write_s": sum(s["write_s"] for s in stats),
                       "upload_s": sum(s["upload_s"] for s in stats), "stall_s": sum(s["stall_s"] for s in stats),
                       "fill_s": sum(s["format_s"] for s in stats)}
                if compress:
                    row.update({k: sum(s[k] for s in stats) for k in ("raw_bytes", "compressed_bytes", "pieces", "stored_pieces", "deflate_s")})
                rows.append(row)
    sizes = tuple(os.path.getsize(p) for p in paths)
    for p in paths:
        os.remove(p)
    c, p = median_of(comp), median_of(plain)
    return {"compressed": c, "uncompressed": p, "size_ratio": sizes[0] / sizes[1], "shrinks_by": sizes[1] / sizes[0],
            "compressed_over_uncompressed_wall": c["wall_s"] / p["wall_s"], "target": 1.0,
            "target_met": bool(c["wall_s"] <= p["wall_s"])}


def kernel_row(stream_dev, repeats, zlib_levels):
    """Kernel times of one XDR stream slice (a CUDA uint8 vector) and its size against zlib."""
    n = int(stream_dev.numel())
    piece = device.DEFLATE_PIECE
    slots = torch.empty((-(-n // piece), device.deflate_bound(piece)), dtype=torch.uint8, device="cuda")
    out = torch.empty(slots.numel(), dtype=torch.uint8, device="cuda")
    t_pieces, t_pack = [], []
    for i in range(repeats + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        dst, lens, _ = device.deflate_pieces(stream_dev, piece, dst=slots)
        e[1].record()
        packed = device.deflate_pack(dst, lens, out=out)
        e[2].record()
        torch.cuda.synchronize()
        if i:
            t_pieces.append(e[0].elapsed_time(e[1]) / 1e3)
            t_pack.append(e[1].elapsed_time(e[2]) / 1e3)
    lens_h = lens.cpu().numpy()
    row = {"slice_bytes": n, "pieces": int(lens_h.size), "stored_pieces": int((lens_h[:-1] == piece + 5).sum()),
           "packed_bytes": int(packed.numel()), "packed_over_input": packed.numel() / n,
           "deflate_pieces_s": statistics.median(t_pieces), "deflate_pack_s": statistics.median(t_pack)}
    row["deflate_pieces_input_GBps"] = n / row["deflate_pieces_s"] / 1e9
    row["both_kernels_input_GBps"] = n / (row["deflate_pieces_s"] + row["deflate_pack_s"]) / 1e9
    host = stream_dev.cpu().numpy().tobytes()
    inflated = zlib.decompressobj(-15).decompress(packed.cpu().numpy().tobytes() + b"\x03\x00")
    row["inflates_to_input"] = bool(inflated == host)
    for level in zlib_levels:
        t0 = time.perf_counter()
        size = len(zlib.compress(host, level))
        dt = time.perf_counter() - t0
        row[f"zlib{level}_bytes"], row[f"zlib{level}_host_MBps"] = size, n / dt / 1e6
        row[f"packed_over_zlib{level}"] = packed.numel() / size
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=10000)
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--slice-mb", type=int, default=256, help="MB of each kind's XDR stream the kernel and zlib figures use")
    ap.add_argument("--gz-cells", type=int, default=400, help="cells of the GzipFile host route's slice")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dir", default=None, help="directory on local disk for the files (default: the system's temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_rds_gzip.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rds_gzip.py needs a GPU")
    torch.cuda.set_device(0)
    device.init(0)
    G, C = a.genes, a.cells
    gen = torch.Generator(device="cuda").manual_seed(28)
    smoothed = torch.randn((C, G), dtype=torch.float64, device="cuda", generator=gen) * 0.05 + 1.0
    x_dev = torch.where((smoothed - 1.0).abs() < 0.075, torch.ones_like(smoothed), smoothed)          # denoised-like
    counts_dev = torch.poisson(torch.full((G, C), 0.15, dtype=torch.float32, device="cuda"), generator=gen).double()
    counts = counts_dev.cpu().numpy()                                                                    # the object's host count.data
    n_ref = max(C // 10, 1)
    obj = InfercnvObject(expr_data=None, count_data=counts,
                         gene_order=GeneOrder(np.repeat([f"chr{k + 1}" for k in range(22)], -(-G // 22))[:G],
                                              np.arange(G) * 50000 + 1, np.arange(G) * 50000 + 30001),
                         reference_grouped_cell_indices={"normal": np.arange(C - n_ref, C)},
                         observation_grouped_cell_indices={"tumor": np.arange(C - n_ref)},
                         gene_names=np.array([f"GENE{i}" for i in range(G)]), cell_names=np.array([f"cell_{i:06d}" for i in range(C)]))
    res = {"bench": "rds_gzip", "device": torch.cuda.get_device_name(0), "genes": G, "cells": C, "payload_bytes": 2 * G * C * 8,
           "chunk_bytes": rds.CHUNK_BYTES, "piece_bytes": device.DEFLATE_PIECE, "repeats": a.repeats}

    # ---- the kernels and the sizes, per kind of data, on a slice of the XDR stream
    n_slice = min(a.slice_mb << 20, G * C * 8) // 8
    states = torch.randint(1, 7, (n_slice // 128 + 1,), device="cuda", generator=gen).double().repeat_interleave(128)[:n_slice]
    kinds = {"denoised": x_dev.reshape(-1)[:n_slice], "counts": counts_dev.t().reshape(-1)[:n_slice],
             "smoothed": smoothed.reshape(-1)[:n_slice], "states": states}
    res["kernels"] = {k: kernel_row(device.xdr_encode(v.contiguous()), a.repeats, (1, 6)) for k, v in kinds.items()}
    del states, kinds, counts_dev

    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        res["object"] = timed_pair(obj, x_dev, tmp, a.repeats)
        lone = obj.copy()
        lone.count_data = None
        res["smoothed"] = timed_pair(lone, smoothed, tmp, a.repeats)

        # the floor: as many bytes as the compressed file holds, from a pinned buffer to the same directory
        nbytes = int(res["object"]["compressed"]["file_bytes"])
        chunk = max(min(nbytes, 256 << 20), 1)
        view = memoryview(torch.zeros(chunk, dtype=torch.uint8).pin_memory().numpy())
        floor = []
        for _ in range(a.repeats + 1):
            t0 = time.perf_counter()
            with open(os.path.join(tmp, "floor.bin"), "wb") as f:
                left = nbytes
                while left > 0:
                    k = min(chunk, left)
                    f.write(view[:k])
                    left -= k
            floor.append(time.perf_counter() - t0)
        os.remove(os.path.join(tmp, "floor.bin"))
        floor_s = statistics.median(floor[1:])
        res["floor"] = {"bytes": nbytes, "file_write_s": floor_s, "compressed_over_floor": res["object"]["compressed"]["wall_s"] / floor_s}

        # the host route on a slice of the cells, as a rate
        n = min(a.gz_cells, C)
        part = InfercnvObject(expr_data=np.ascontiguousarray(x_dev[:n].cpu().numpy().T), count_data=np.ascontiguousarray(counts[:, :n]),
                              gene_order=obj.gene_order, reference_grouped_cell_indices={"normal": np.arange(n // 2)},
                              observation_grouped_cell_indices={"tumor": np.arange(n // 2, n)}, gene_names=obj.gene_names,
                              cell_names=obj.cell_names[:n])
        t0 = time.perf_counter()
        save_infercnv_obj(part, os.path.join(tmp, "host.rds.gz"), compress=True, device=False)
        dt = time.perf_counter() - t0
        res["gzipfile_host"] = {"slice_cells": n, "seconds": dt, "input_MBps": 2 * G * n * 8 / dt / 1e6,
                                "file_over_input": os.path.getsize(os.path.join(tmp, "host.rds.gz")) / (2 * G * n * 8),
                                "seconds_extrapolated_as_a_rate_to_full_size": dt * C / n, "extrapolated": True}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
