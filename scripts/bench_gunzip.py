#!/usr/bin/env python3
"""Benchmark of inflating gzip streams without flush points on the device (infercnv_amd.gunzip, icnv_gunzip_*_dev, DESIGN K30).
Prints ONE JSON line (and writes it with --out, default profiles/bench_gunzip.json); progress goes to stderr.

One process, one warm-up, then the median and the spread (max - min) of --repeats readings, the two routes alternating.  The
baseline of every row is the same call with ICNV_INFLATE=0: the parent's route, unchanged code.
  readers   (a) K22's MatrixMarket file (--genes x --text-cells, 10 % density) and (b) K21's dense table of the same matrix,
            each compressed once with zlib level 6 (what the gzip command line writes), through device.read_mtx /
            device.read_table: the device route against the same call with ICNV_INFLATE=0 (Python's gzip on a reader thread
            beside the parse).  crossover: (a) cut to prefixes of whole lines, each compressed the same way; the smallest
            file from which the device route stays ahead by more than the spread, rounded up to a power of two, is
            gunzip.GUNZIP_MIN_BYTES.
  object    an R-like infercnv object (no flush points: the plain .rds through zlib level 6, the code R's gzfile runs) of
            --genes x --cells at K28's kinds of data, through load_infercnv_obj(return_device=True), device route against
            ICNV_INFLATE=0; phases, units and the peak of torch's device memory.  THE BAR for the route's default.
  object_crossover   the same at --crossover-cells cells: where the routes cross for this consumer (reported).
  kinds     per kind of data (denoised, counts, smoothed, HMM states) a --slice-mb slice of its XDR stream through zlib
            level 6: output GB/s of gunzip.gunzip (upload included and excluded) against zlib's inflate on one core."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from infercnv_amd import device, gunzip, load_infercnv_obj, save_infercnv_obj  # noqa: E402
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


def gz_level6(data):
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    return c.compress(data) + c.flush()


def host_route(file_bytes):
    """The parent's way to the same place: inflate on one core, then the bytes to the device."""
    plain = zlib.decompress(file_bytes, 31)
    return torch.frombuffer(bytearray(plain), dtype=torch.uint8).cuda()


def both_routes(file_bytes, plain, repeats):
    """device / host seconds of one file, alternating, after a warm-up; the device route's phases, units and memory."""
    dev_s, host_s, phases, peak = [], [], [], []
    st = None
    for i in range(repeats + 1):
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        td, out = timed(lambda: gunzip.gunzip(file_bytes))
        st = gunzip.gunzip_stats()
        if out is None:
            return {"compressed_bytes": len(file_bytes), "inflated_bytes": len(plain), "route": "host", "reason": st["reason"]}
        peak_now = torch.cuda.max_memory_allocated() - base
        if i == 0 and out.cpu().numpy().tobytes() != plain:
            raise SystemExit("the device route's bytes differ from zlib's")
        del out
        th, out = timed(lambda: host_route(file_bytes))
        del out
        if i:
            dev_s.append(td)
            host_s.append(th)
            phases.append(st["seconds"])
            peak.append(peak_now)
    d, h = med(dev_s), med(host_s)
    return {"compressed_bytes": len(file_bytes), "inflated_bytes": len(plain), "route": "device", "device_s": d, "host_s": h,
            "host_over_device": h["median"] / d["median"],
            "device_ahead_by_more_than_the_spread": bool(max(dev_s) + max(d["spread"], h["spread"]) < min(host_s)),
            "phases_s": {k: statistics.median(p[k] for p in phases) for k in phases[0]},
            "tails_share_of_device": statistics.median(p["tails"] for p in phases) / d["median"],
            **{k: st[k] for k in ("candidates", "chain_units", "false_candidates", "units_short", "markers_tail")},
            "peak_device_bytes": max(peak)}


def gzip_file(src, dst):
    t0 = time.perf_counter()
    with open(src, "rb") as f, open(dst, "wb") as g:
        c = zlib.compressobj(6, zlib.DEFLATED, 31)
        for block in iter(lambda: f.read(1 << 24), b""):
            g.write(c.compress(block))
        g.write(c.flush())
    return time.perf_counter() - t0


def reader_routes(read, path, repeats, same):
    """read(path) -- device.read_mtx or device.read_table of a .gz -- on the device route and with ICNV_INFLATE=0, alternating."""
    rows, phases, peak, st, keep = {"device": [], "host": []}, [], [], None, None
    for i in range(repeats + 1):
        for route in rows:
            os.environ["ICNV_INFLATE"] = "0" if route == "host" else "1"
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            dt, out = timed(lambda: read(path))
            stats = out[-1]
            if route == "device":
                if stats["source"] != "device_gunzip":
                    os.environ.pop("ICNV_INFLATE", None)
                    return {"file_bytes": os.path.getsize(path), "route": "host", "reason": stats["source_reason"]}
                st = gunzip.gunzip_stats()
            if i == 0:
                if route == "device":
                    keep = out
                else:
                    if not same(keep, out):
                        raise SystemExit(f"the two routes differ on {path}")
                    keep = None
            elif route == "device":
                phases.append(dict(st["seconds"], parse=stats["parse_s"]))
                peak.append(torch.cuda.max_memory_allocated() - base)
            if i:
                rows[route].append(dt)
            del out
    os.environ.pop("ICNV_INFLATE", None)
    d, h = med(rows["device"]), med(rows["host"])
    return {"file_bytes": os.path.getsize(path), "inflated_bytes": st["inflated_bytes"], "route": "device", "device_s": d, "host_s": h,
            "host_over_device": h["median"] / d["median"],
            "device_ahead_by_more_than_the_spread": bool(max(rows["device"]) + max(d["spread"], h["spread"]) < min(rows["host"])),
            "phases_s": {k: statistics.median(p[k] for p in phases) for k in phases[0]},
            "tails_share_of_device": statistics.median(p["tails"] for p in phases) / d["median"],
            **{k: st[k] for k in ("candidates", "chain_units", "false_candidates", "units_short", "markers_tail")},
            "peak_device_bytes": max(peak)}


def readers_section(tmp, G, C, repeats):
    """(a) K22's MatrixMarket file and (b) K21's dense table of the same matrix, each compressed once by zlib level 6, through
    read_mtx / read_table; and (a) cut to prefixes of whole lines for the size at which the routes cross."""
    from bench_read_mtx import write_triplets
    from infercnv_amd import heatmap
    gen = torch.Generator(device="cuda").manual_seed(22)
    dense = torch.floor(torch.empty((C, G), dtype=torch.float64, device="cuda").exponential_(0.05, generator=gen)) + 1
    dense *= torch.rand((C, G), generator=gen, device="cuda") < 0.10
    col, row = torch.nonzero(dense, as_tuple=True)
    val = dense[col, row].long()
    nnz = int(val.numel())
    mtx, tsv = os.path.join(tmp, "matrix.mtx"), os.path.join(tmp, "counts.tsv")
    write_triplets(mtx, b"%%%%MatrixMarket matrix coordinate integer general\n%d %d %d\n" % (G, C, nnz), row, col, val)
    del row, col, val
    heatmap.write_matrix(tsv, dense, np.arange(C, dtype=np.int32), "gene_rows", [f"GENE{i}" for i in range(G)],
                         [f"cell_{i:06d}" for i in range(C)], quote=False, sep="\t")
    del dense
    out = {"genes": G, "cells": C, "entries": nnz}
    same_mtx = lambda x, y: all(torch.equal(p, q) for p, q in zip(x[0].t[1:], y[0].t[1:]))
    same_tsv = lambda x, y: x[0] == y[0] and x[1] == y[1] and torch.equal(x[2].view(torch.int64), y[2].view(torch.int64))
    for name, path, read, same in (("matrix_market", mtx, device.read_mtx, same_mtx), ("dense_tsv", tsv, device.read_table, same_tsv)):
        seconds = gzip_file(path, path + ".gz")
        out[name] = dict(reader_routes(read, path + ".gz", repeats, same), plain_bytes=os.path.getsize(path), written_by_zlib_in_s=seconds)
        say(name, json.dumps(out[name]))
        os.remove(path + ".gz")
    os.remove(tsv)
    with open(mtx, "rb") as f:
        text = f.read()
    body0 = text.index(b"\n", text.index(b"\n") + 1) + 1                # behind the banner and the size line
    rows, size = [], 1 << 22                                           # prefixes of 4 MiB of text and up, doubling
    while size < len(text) - body0:
        cut = text.rfind(b"\n", body0, body0 + size) + 1
        body = text[body0:cut]
        last_col = int(body[body.rfind(b"\n", 0, len(body) - 1) + 1:].split()[1])
        part = os.path.join(tmp, "part.mtx")
        with open(part, "wb") as f:
            f.write(b"%%%%MatrixMarket matrix coordinate integer general\n%d %d %d\n" % (G, last_col, body.count(b"\n")) + body)
        gzip_file(part, part + ".gz")
        rows.append(reader_routes(device.read_mtx, part + ".gz", repeats, same_mtx))
        say("prefix", json.dumps({k: rows[-1].get(k) for k in ("file_bytes", "route", "host_over_device", "device_ahead_by_more_than_the_spread")}))
        size *= 2
    rows.append(out["matrix_market"])
    ahead = [bool(r.get("device_ahead_by_more_than_the_spread")) for r in rows]
    first = next((i for i in range(len(rows)) if all(ahead[i:])), None)
    out["crossover"] = {"prefixes": rows[:-1], "smallest_file_bytes_from_which_the_device_stays_ahead": None if first is None else rows[first]["file_bytes"],
                        "rounded_up_to_a_power_of_two": None if first is None else 1 << (rows[first]["file_bytes"] - 1).bit_length()}
    return out


def object_row(tmp, G, C, x_dev, counts, repeats):
    """An R-like object of C cells: written plain, compressed by zlib level 6 on one core, loaded by both routes."""
    n_ref = max(C // 10, 1)
    obj = InfercnvObject(expr_data=None, count_data=counts,
                         gene_order=GeneOrder(np.repeat([f"chr{k + 1}" for k in range(22)], -(-G // 22))[:G],
                                              np.arange(G) * 50000 + 1, np.arange(G) * 50000 + 30001),
                         reference_grouped_cell_indices={"normal": np.arange(C - n_ref, C)},
                         observation_grouped_cell_indices={"tumor": np.arange(C - n_ref)},
                         gene_names=np.array([f"GENE{i}" for i in range(G)]), cell_names=np.array([f"cell_{i:06d}" for i in range(C)]))
    plain_path, r_path = os.path.join(tmp, "p.rds"), os.path.join(tmp, "r.rds")
    save_infercnv_obj(obj, plain_path, x_dev=x_dev)
    t0 = time.perf_counter()
    with open(plain_path, "rb") as src, open(r_path, "wb") as dst:
        c = zlib.compressobj(6, zlib.DEFLATED, 31)
        for block in iter(lambda: src.read(1 << 24), b""):
            dst.write(c.compress(block))
        dst.write(c.flush())
    row = {"cells": C, "file_bytes": os.path.getsize(r_path), "plain_bytes": os.path.getsize(plain_path),
           "written_by_zlib_in_s": time.perf_counter() - t0}
    os.remove(plain_path)
    say("object file", row)
    want = x_dev.view(torch.int64)
    rows = {"device": [], "host": []}
    phases, peak, equal, st = [], [], True, None
    for i in range(repeats + 1):
        for route in rows:
            os.environ["ICNV_INFLATE"] = "0" if route == "host" else "1"
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            dt, (got, got_x) = timed(lambda: load_infercnv_obj(r_path, return_device=True))
            if route == "device":
                st = gunzip.gunzip_stats()
                if st["route"] != "device":
                    raise SystemExit(f"the device route was not taken: {st}")
            equal = equal and bool(torch.equal(got_x.view(torch.int64), want)) and bool(np.array_equal(got.count_data, counts))
            if i:
                rows[route].append(dt)
                if route == "device":
                    phases.append(dict(st["seconds"], reader=dt - sum(st["seconds"].values())))
                    peak.append(torch.cuda.max_memory_allocated() - base)
            del got, got_x
    os.environ.pop("ICNV_INFLATE", None)
    os.remove(r_path)
    d, h = med(rows["device"]), med(rows["host"])
    row.update({"device_s": d, "host_s": h, "host_over_device": h["median"] / d["median"],
                "device_ahead_by_more_than_the_spread": bool(max(rows["device"]) + max(d["spread"], h["spread"]) < min(rows["host"])),
                "phases_s": {k: statistics.median(p[k] for p in phases) for k in phases[0]},
                "tails_share_of_device": statistics.median(p["tails"] for p in phases) / d["median"],
                "peak_device_bytes_above_the_resident_matrix": max(peak), "equal_to_what_was_saved": equal,
                **{k: st[k] for k in ("candidates", "chain_units", "false_candidates", "units_short", "markers_tail")}})
    say("object", json.dumps({k: row[k] for k in ("cells", "file_bytes", "host_over_device", "device_ahead_by_more_than_the_spread")}))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=10000)
    ap.add_argument("--cells", type=int, default=50000, help="cells of the R-like object: K28's shape (its 8 GB are compressed by one core in about a minute)")
    ap.add_argument("--crossover-cells", default="125,250,500,1000,2000,4000", help="smaller objects, for the size at which the routes cross")
    ap.add_argument("--text-cells", type=int, default=50000, help="cells of the MatrixMarket file and the dense table: K22's and K21's shape")
    ap.add_argument("--slice-mb", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_gunzip.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gunzip.py needs a GPU")
    torch.cuda.set_device(0)
    device.init(0)
    gunzip.GUNZIP_MIN_BYTES = 0                                # the routes are compared at every size; the constant is this run's result
    rng = np.random.default_rng(30)
    G, C = a.genes, a.cells
    res = {"bench": "gunzip", "device": torch.cuda.get_device_name(0), "genes": G, "object_cells": C, "text_cells": a.text_cells,
           "slice_mb": a.slice_mb, "repeats": a.repeats, "zlib_level": 6,
           }

    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        res["readers"] = readers_section(tmp, G, a.text_cells, a.repeats)

    gen = torch.Generator(device="cuda").manual_seed(28)
    smoothed = torch.randn((C, G), dtype=torch.float64, device="cuda", generator=gen) * 0.05 + 1.0
    x_dev = torch.where((smoothed - 1.0).abs() < 0.075, torch.ones_like(smoothed), smoothed)          # denoised-like
    counts_dev = torch.poisson(torch.full((G, C), 0.15, dtype=torch.float32, device="cuda"), generator=gen).double()
    n_slice = min(a.slice_mb << 20, G * C * 8) // 8
    states = torch.randint(1, 7, (n_slice // 128 + 1,), device="cuda", generator=gen).double().repeat_interleave(128)[:n_slice]
    kinds = {"denoised": x_dev.reshape(-1)[:n_slice], "counts": counts_dev.t().reshape(-1)[:n_slice], "smoothed": smoothed.reshape(-1)[:n_slice],
             "states": states}
    res["kinds"] = {}
    for k, v in kinds.items():
        plain = device.xdr_encode(v.contiguous()).cpu().numpy().tobytes()
        file_bytes = gz_level6(plain)
        row = both_routes(file_bytes, plain, a.repeats)
        tz = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            zlib.decompress(file_bytes, 31)
            tz.append(time.perf_counter() - t0)
        row["zlib_inflate_s"] = med(tz)
        row["zlib_output_GBps"] = len(plain) / row["zlib_inflate_s"]["median"] / 1e9
        if row["route"] == "device":
            row["device_output_GBps"] = len(plain) / row["device_s"]["median"] / 1e9
            row["device_output_GBps_without_upload"] = len(plain) / (row["device_s"]["median"] - row["phases_s"]["upload"]) / 1e9
        res["kinds"][k] = row
        say(k, json.dumps(row))
        del plain, file_bytes
    del states, kinds, smoothed

    counts = counts_dev.cpu().numpy()
    del counts_dev
    sizes = sorted({int(c) for c in a.crossover_cells.split(",") if c and int(c) < C} | {C})
    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        rows = [object_row(tmp, G, n, x_dev[:n], np.ascontiguousarray(counts[:, :n]), a.repeats) for n in sizes]
    res["object"] = rows[-1]
    ahead = [r["device_ahead_by_more_than_the_spread"] for r in rows]
    first = next((i for i in range(len(rows)) if all(ahead[i:])), None)
    res["object_crossover"] = {"rows": rows[:-1], "smallest_file_bytes_from_which_the_device_stays_ahead":
                               None if first is None else rows[first]["file_bytes"],
                               "rounded_up_to_a_power_of_two": None if first is None else 1 << (rows[first]["file_bytes"] - 1).bit_length()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
