#!/usr/bin/env python3
"""Benchmark of R count matrices read on the device (device.read_rds_counts, CreateInfercnvObject from .rds, DESIGN K34).  Prints
ONE JSON line (and writes it with --out, default profiles/bench_rds_counts.json).

K22's seeded genes x cells integer matrix at --density is written into --dir three times: as a gzip .rds of a dgCMatrix and as a
gzip .rds of the dense integer matrix (both through write_rds(compress=True): flush points, so K29 inflates them), and as
matrix.mtx.gz (gzip level 1 on the host).  Everything runs in this process, each route once for warm-up and then three times,
the median reported and every reading listed:
  rds_device     CreateInfercnvObject(path.rds), the new route: seconds, the reader's stats of the median reading (the inflate
                 route taken, bytes uploaded), and from one further reading with the event timers on the kernel milliseconds
  rds_host       the only route there was before: rds.read_rds(path) on the host, then CreateInfercnvObject of the arrays (a
                 scipy csc_matrix with sparse=True for the dgCMatrix)
  mtx_gz         CreateInfercnvObject of matrix.mtx.gz with the names (dgCMatrix case only)
  pcie_bytes     computed from the shapes and the reader's stats: host to device (the compressed file on the device-inflate
                 route, the payloads otherwise), device to host (the object's matrix, the column sums)
  device_bytes   what the device held at the end of the route on top of what it held before (the library's pool and torch's
                 cache only grow during it, so this is its peak), and torch's own peak
  equal          whether the new route's object equals the host route's in expr_data, names and groups
The ratio the README quotes is rds_host.seconds / rds_device.seconds of the dgCMatrix file."""
import argparse
import gzip
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import infercnv_amd  # noqa: E402
from infercnv_amd import device, rds  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_read_mtx import used_bytes, write_triplets  # noqa: E402

KERNELS = ("rds_columns", "rds_csc_check", "rds_csc_fill")


def note(text):
    print(f"[bench_rds_counts] {text}", file=sys.stderr, flush=True)


def median_of(route, repeats=3):
    """route() -> (object, extra dict) once for warm-up, then `repeats` times."""
    route()
    device.release_pool()
    torch.cuda.empty_cache()
    readings = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = used_bytes()
        t0 = time.perf_counter()
        obj, extra = route()
        torch.cuda.synchronize()
        readings.append(dict(extra, seconds=time.perf_counter() - t0, device_bytes_held_at_the_end_over_before=used_bytes() - before,
                             torch_peak_bytes=int(torch.cuda.max_memory_allocated())))
        del obj
    walls = sorted(r["seconds"] for r in readings)
    mid = next(r for r in readings if r["seconds"] == walls[len(walls) // 2])
    return dict(mid, seconds_of_every_reading=[r["seconds"] for r in readings])


def kernel_ms(route):
    device.timing_enable(True)
    device.timing_reset()
    route()
    torch.cuda.synchronize()
    out = {}
    for k in KERNELS:
        try:
            out[k] = device.timing_get(k)[0]
        except Exception:                          # a kernel that never ran has no timer
            out[k] = 0.0
    device.timing_enable(False)
    return out


def same(a, b):
    ea, eb = a.expr_data, b.expr_data
    if hasattr(ea, "tocsc") != hasattr(eb, "tocsc"):
        return False
    if hasattr(ea, "tocsc"):
        ok = all(np.array_equal(x, y) for x, y in ((ea.indptr, eb.indptr), (ea.indices, eb.indices), (ea.data, eb.data)))
    else:
        ok = np.array_equal(ea, eb)
    return bool(ok and list(a.gene_names) == list(b.gene_names) and list(a.cell_names) == list(b.cell_names) and
                all(np.array_equal(a.observation_grouped_cell_indices[k], b.observation_grouped_cell_indices[k]) for k in a.observation_grouped_cell_indices))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=10000)
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--density", type=float, default=0.10)
    ap.add_argument("--dir", default=None, help="directory on local disk for the files (default: the system's temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_rds_counts.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rds_counts.py needs a GPU")
    torch.cuda.set_device(0)
    device.init(0)
    G, C = a.genes, a.cells
    gen = torch.Generator(device="cuda").manual_seed(22)
    res = {"bench": "rds_counts", "measured": True, "device": torch.cuda.get_device_name(0), "genes": G, "cells": C, "density": a.density}
    genes, cells = [f"GENE{i}" for i in range(G)], [f"cell_{i:06d}" for i in range(C)]
    order = [(g, f"chr{1 + i * 22 // G}", 1000 * i + 1, 1000 * i + 900) for i, g in enumerate(genes)]
    annot = [(c, "normal" if j % 4 == 0 else "tumor") for j, c in enumerate(cells)]
    names = dict(gene_names=genes, cell_names=cells)
    create = lambda m, **kw: infercnv_amd.CreateInfercnvObject(m, order, annot, ["normal"], **kw)

    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        dense = torch.floor(torch.empty((C, G), dtype=torch.float64, device="cuda").exponential_(0.05, generator=gen)) + 1
        dense *= torch.rand((C, G), generator=gen, device="cuda") < a.density
        col, row = torch.nonzero(dense, as_tuple=True)                 # row-major over (C, G): column-major order of the G x C matrix
        val = dense[col, row]
        nnz = int(val.numel())
        res["entries"] = nnz
        mtx = os.path.join(tmp, "matrix.mtx")
        write_triplets(mtx, b"%%%%MatrixMarket matrix coordinate integer general\n%d %d %d\n" % (G, C, nnz), row, col, val.long())
        with open(mtx, "rb") as src, gzip.open(mtx + ".gz", "wb", compresslevel=1) as dst:
            shutil.copyfileobj(src, dst, 16 << 20)
        os.remove(mtx)
        p = torch.zeros(C + 1, dtype=torch.int64, device="cuda")
        p[1:] = torch.cumsum(torch.bincount(col, minlength=C), 0)
        sparse_value = rds.RS4("dgCMatrix", "Matrix", {"i": row.to(torch.int32).cpu().numpy(), "p": p.to(torch.int32).cpu().numpy(),
                                                       "Dim": np.array([G, C], dtype=np.int32), "Dimnames": [rds._names(genes), rds._names(cells)],
                                                       "x": val.cpu().numpy(), "factors": []})
        del row, col, val, p
        files = {"dgCMatrix": os.path.join(tmp, "sparse.rds"), "matrix_int": os.path.join(tmp, "dense.rds")}
        rds.write_rds(sparse_value, files["dgCMatrix"], compress=True)
        del sparse_value
        rds.write_rds(rds.RValue(rds.RDeviceMatrix(dense.to(torch.int32)), {"dimnames": [rds._names(genes), rds._names(cells)]}), files["matrix_int"],
                      compress=True)
        del dense
        torch.cuda.empty_cache()
        note(f"files written: {nnz} entries")

        for kind, path in files.items():
            out = {"file_bytes": os.path.getsize(path)}
            seen = {}

            def device_route():
                obj = create(path)
                seen["device"] = obj
                return obj, {}

            def reader_stats():
                _, _, got, st = device.read_rds_counts(path)
                del got
                return st

            def host_route():
                t0 = time.perf_counter()
                v = rds.read_rds(path)
                t1 = time.perf_counter()
                if kind == "dgCMatrix":
                    import scipy.sparse as sp
                    m = sp.csc_matrix((v.slots["x"], v.slots["i"], v.slots["p"]), shape=tuple(int(d) for d in v.slots["Dim"]))
                    obj = create(m, sparse=True, **names)
                else:
                    obj = create(v.value, **names)
                seen["host"] = obj
                return obj, {"read_rds_s": t1 - t0}

            out["rds_device"] = median_of(device_route)
            out["rds_device"]["reader"] = {k: v for k, v in reader_stats().items()}
            out["rds_device"]["kernel_ms"] = kernel_ms(device_route)
            note(f"{kind}: device route done")
            out["rds_host"] = median_of(host_route)
            note(f"{kind}: host route done")
            out["equal"] = same(seen["device"], seen["host"])
            obj = seen["device"]
            g, c = obj.expr_data.shape
            kept = int(obj.expr_data.nnz) if hasattr(obj.expr_data, "tocsc") else None
            st = out["rds_device"]["reader"]
            h2d = out["file_bytes"] if st["inflate"].startswith("device") else st["uploaded_bytes"]
            out["pcie_bytes"] = {"rds_device": {"h2d": int(h2d), "d2h_matrix": 12 * kept + 8 * (c + 1) if kept is not None else 8 * g * c, "d2h_col_sums": 8 * C},
                                 "rds_host": {"h2d": (12 * nnz + 8 * (C + 1)) if kind == "dgCMatrix" else 8 * G * C,
                                              "d2h_matrix": 12 * kept + 8 * (c + 1) if kept is not None else 8 * g * c, "d2h_col_sums": 8 * C}}
            seen.clear()
            del obj
            if kind == "dgCMatrix":
                out["mtx_gz"] = median_of(lambda: (create(mtx + ".gz", **names), {}))
                out["mtx_gz"]["file_bytes"] = os.path.getsize(mtx + ".gz")
                note("mtx.gz route done")
            out["host_over_device"] = out["rds_host"]["seconds"] / out["rds_device"]["seconds"]
            res[kind] = out
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
