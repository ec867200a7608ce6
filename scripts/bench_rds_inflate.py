#!/usr/bin/env python3
"""Benchmark of reading a gzip-compressed .rds on the device (infercnv_amd.rds.inflate_gzip, icnv_inflate_scan_dev /
_measure_dev / _units_dev, icnv_crc32_pieces_dev, DESIGN K29).  Prints ONE JSON line (and writes it with --out, default
profiles/bench_rds_inflate.json); progress goes to stderr.

The file: K28's benchmark object, genes x cells (default 10 000 x 50 000), a denoised-like expr.data and a count-like
count.data of 4 GB each, written with compress=True; and the same object uncompressed.  All timings in one process, one warm-up,
then the median and the spread (max - min) of --repeats readings, the three loads alternating:
  device         load_infercnv_obj(return_device=True) of the compressed file: wall seconds, the phases of inflate_stats()
                 (upload, scan, measure, chain, decode, crc; reader = the rest), candidates, chain units, false candidates, and
                 the peak of torch's device memory during the load.
  host           the same call with ICNV_INFLATE=0: gzip.decompress on the host and a second upload, the only route before K29.
                 THE BAR: device wall < host wall by more than the spread of either.
  uncompressed   the same call on the compress=False file (reported, not gated).
  kinds          per kind of data (denoised, counts, smoothed, HMM states), on a --slice-mb slice of its XDR stream compressed
                 by icnv_deflate_pieces_dev: scan, measure, decode and CRC seconds (median of --repeats after a warm-up, each
                 waited for), output GB/s of the decode alone and of measure + decode, and zlib's inflate of the same stream on
                 the host (one thread).  The bar per kind: measure + decode < zlib's inflate by more than the spread.
  turned_away    the seconds inflate_gzip spends on a GzipFile-written file (no flush points, what R writes) of --gz-cells
                 cells before it returns None, against gzip.decompress of that file."""
import argparse
import gzip
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

from infercnv_amd import device, load_infercnv_obj, rds, save_infercnv_obj  # noqa: E402
from infercnv_amd.infercnv_object import GeneOrder, InfercnvObject  # noqa: E402


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def med(v):
    return {"median": statistics.median(v), "spread": max(v) - min(v), "readings": list(v)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def kind_row(stream_dev, repeats):
    """One slice of an XDR stream: compressed by K28's kernels, inflated by K29's, and by zlib on the host."""
    n = int(stream_dev.numel())
    dst, lens, _ = device.deflate_pieces(stream_dev, device.DEFLATE_PIECE)
    packed = torch.cat([device.deflate_pack(dst, lens), torch.tensor([3, 0], dtype=torch.uint8, device="cuda")])   # + a final empty block
    del dst
    t = {k: [] for k in ("scan", "measure", "decode", "crc")}
    for i in range(repeats + 1):
        ts, cand = timed(lambda: device.inflate_scan(packed))
        start = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), cand[cand < packed.numel()]])
        tm, (end, out_len, status) = timed(lambda: device.inflate_measure(packed, start, rds.INFLATE_MAX_IN))
        ok = bool((status <= 1).all()) and bool((end[:-1] == start[1:]).all()) and int(out_len.sum()) == n
        off = torch.cumsum(out_len, 0) - out_len
        out = torch.empty(n, dtype=torch.uint8, device="cuda")
        td, st2 = timed(lambda: device.inflate_units(packed, start, end, off, out_len, out))
        tc, crcs = timed(lambda: device.crc32_pieces(out, rds.INFLATE_CRC_PIECE))
        ok = ok and bool((st2 == status).all()) and bool(torch.equal(out, stream_dev))
        if i:
            for k, v in zip(t, (ts, tm, td, tc)):
                t[k].append(v)
    host = packed.cpu().numpy().tobytes()
    tz = []
    for i in range(repeats):
        t0 = time.perf_counter()
        inflated = zlib.decompressobj(-15).decompress(host)
        tz.append(time.perf_counter() - t0)
    both = [a + b for a, b in zip(t["measure"], t["decode"])]
    row = {"slice_bytes": n, "packed_bytes": int(packed.numel()), "units": int(start.numel()), "equals_input": ok and len(inflated) == n,
           **{f"{k}_s": med(v) for k, v in t.items()}, "measure_plus_decode_s": med(both), "zlib_inflate_host_s": med(tz)}
    row["decode_output_GBps"] = n / row["decode_s"]["median"] / 1e9
    row["measure_plus_decode_output_GBps"] = n / row["measure_plus_decode_s"]["median"] / 1e9
    row["zlib_output_GBps"] = n / row["zlib_inflate_host_s"]["median"] / 1e9
    row["beats_zlib_by_more_than_the_spread"] = bool(max(both) + max(row["measure_plus_decode_s"]["spread"], row["zlib_inflate_host_s"]["spread"]) < min(tz))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=10000)
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--slice-mb", type=int, default=256)
    ap.add_argument("--gz-cells", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dir", default=None, help="directory on local disk for the files (default: the system's temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_rds_inflate.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rds_inflate.py needs a GPU")
    torch.cuda.set_device(0)
    device.init(0)
    G, C = a.genes, a.cells
    gen = torch.Generator(device="cuda").manual_seed(28)
    smoothed = torch.randn((C, G), dtype=torch.float64, device="cuda", generator=gen) * 0.05 + 1.0
    x_dev = torch.where((smoothed - 1.0).abs() < 0.075, torch.ones_like(smoothed), smoothed)          # denoised-like
    counts_dev = torch.poisson(torch.full((G, C), 0.15, dtype=torch.float32, device="cuda"), generator=gen).double()
    res = {"bench": "rds_inflate", "device": torch.cuda.get_device_name(0), "genes": G, "cells": C, "payload_bytes": 2 * G * C * 8,
           "max_in": rds.INFLATE_MAX_IN, "repeats": a.repeats}

    n_slice = min(a.slice_mb << 20, G * C * 8) // 8
    states = torch.randint(1, 7, (n_slice // 128 + 1,), device="cuda", generator=gen).double().repeat_interleave(128)[:n_slice]
    kinds = {"denoised": x_dev.reshape(-1)[:n_slice], "counts": counts_dev.t().reshape(-1)[:n_slice],
             "smoothed": smoothed.reshape(-1)[:n_slice], "states": states}
    res["kinds"] = {}
    for k, v in kinds.items():
        res["kinds"][k] = kind_row(device.xdr_encode(v.contiguous()), a.repeats)
        say(k, json.dumps(res["kinds"][k]))
    del states, kinds, smoothed
    counts = counts_dev.cpu().numpy()
    del counts_dev
    n_ref = max(C // 10, 1)
    obj = InfercnvObject(expr_data=None, count_data=counts,
                         gene_order=GeneOrder(np.repeat([f"chr{k + 1}" for k in range(22)], -(-G // 22))[:G],
                                              np.arange(G) * 50000 + 1, np.arange(G) * 50000 + 30001),
                         reference_grouped_cell_indices={"normal": np.arange(C - n_ref, C)},
                         observation_grouped_cell_indices={"tumor": np.arange(C - n_ref)},
                         gene_names=np.array([f"GENE{i}" for i in range(G)]), cell_names=np.array([f"cell_{i:06d}" for i in range(C)]))

    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        paths = {"device": os.path.join(tmp, "c.rds"), "host": os.path.join(tmp, "c.rds"), "uncompressed": os.path.join(tmp, "p.rds")}
        save_infercnv_obj(obj, paths["device"], x_dev=x_dev, compress=True)
        save_infercnv_obj(obj, paths["uncompressed"], x_dev=x_dev)
        res["file_bytes"] = {"compressed": os.path.getsize(paths["device"]), "uncompressed": os.path.getsize(paths["uncompressed"])}
        say("files written", res["file_bytes"])
        want = x_dev.view(torch.int64)
        rows = {k: [] for k in paths}
        phases, peak, equal = [], [], True
        for i in range(a.repeats + 1):
            for route, path in paths.items():
                os.environ["ICNV_INFLATE"] = "0" if route == "host" else "1"
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                dt, (got, got_x) = timed(lambda: load_infercnv_obj(path, return_device=True))
                st = rds.inflate_stats()
                say(route, i, f"{dt:.3f} s", st["route"], st.get("reason", ""))
                if route == "device" and st["route"] != "device":
                    raise SystemExit(f"the device route was not taken: {st}")
                equal = equal and bool(torch.equal(got_x.view(torch.int64), want)) and bool(np.array_equal(got.count_data, counts))
                if i:
                    rows[route].append(dt)
                    if route == "device":
                        phases.append(dict(st["seconds"], reader=dt - sum(st["seconds"].values())))
                        peak.append(torch.cuda.max_memory_allocated() - base)
                        res["units"] = {k: st[k] for k in ("candidates", "chain_units", "false_candidates", "compressed_bytes", "inflated_bytes")}
                del got, got_x
        os.environ.pop("ICNV_INFLATE", None)
        res["load"] = {k: med(v) for k, v in rows.items()}
        res["load"]["device_phases_s"] = {k: statistics.median(p[k] for p in phases) for k in phases[0]}
        res["load"]["device_peak_bytes_above_the_resident_matrix"] = max(peak)
        res["load"]["equal_to_what_was_saved"] = equal
        d, h, u = (res["load"][k] for k in ("device", "host", "uncompressed"))
        res["load"]["host_over_device"] = h["median"] / d["median"]
        res["load"]["device_over_uncompressed"] = d["median"] / u["median"]
        res["load"]["bar_met"] = bool(max(d["readings"]) + max(d["spread"], h["spread"]) < min(h["readings"]))

        # a file without flush points
        n = min(a.gz_cells, C)
        part = InfercnvObject(expr_data=np.ascontiguousarray(x_dev[:n].cpu().numpy().T), count_data=np.ascontiguousarray(counts[:, :n]),
                              gene_order=obj.gene_order, reference_grouped_cell_indices={"normal": np.arange(n // 2)},
                              observation_grouped_cell_indices={"tumor": np.arange(n // 2, n)}, gene_names=obj.gene_names,
                              cell_names=obj.cell_names[:n])
        r_path = os.path.join(tmp, "r.rds")
        save_infercnv_obj(part, r_path, compress=True, device=False)
        away, host = [], []
        for i in range(a.repeats + 1):
            dt, out = timed(lambda: rds.inflate_gzip(r_path))
            if out is not None:
                raise SystemExit("a file without flush points was taken")
            t0 = time.perf_counter()
            with open(r_path, "rb") as f:
                gzip.decompress(f.read())
            if i:
                away.append(dt)
                host.append(time.perf_counter() - t0)
        res["turned_away"] = {"cells": n, "file_bytes": os.path.getsize(r_path), "reason": rds.inflate_stats()["reason"],
                              "inflate_gzip_s": med(away), "gzip_decompress_s": med(host)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
