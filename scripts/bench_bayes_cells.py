#!/usr/bin/env python3
"""Benchmark of steps 18-19 per cell (bayes_net route="table", DESIGN K25).  Prints ONE JSON line (and writes it with --out,
default profiles/bench_bayes_cells.json).

Synthetic i6 states as scripts/bench_cnv_reports.py makes them (neutral state 3, --share of every cell's genes in non-neutral
runs of 20-60 genes), by = "cell"; the expression matrix is Normal(1, 0.3) on the device.  Wall seconds of one pass each:
  table      RegionTable.from_states (upload, run records, cell lists, tokens) and the group numbers
  loglik     device.bayes_loglik_arrays
  sampler    device.bayes_sample, default schedule; icnv_bayes_stats of the call
  filter     filterHighPNormals on the host genes x cells matrix (decisions, one fill_regions launch, the overlay,
             CNV_State_Probabilities.dat)
  adjusted   adjust_genes_regions_report from the records (the step-17 reports are written first, untimed here)
  old_route  route="dict" and the parsing adjust on a slice of --old-slice cells, EXTRAPOLATED as a rate (regions / s)
  packed     with --baseline-lib PATH (libicnv_hip.so of the PARENT commit, built separately): icnv_bayes_sample_dev on the
             regions of a --slice cells slice, the same L and offsets, in a child process per library through the same ctypes
             harness; a warm-up, then three calls each.  Passes when the median is faster by more than the spread of the three
             readings; a ratio below 2 is recorded as a miss."""
import argparse
import ctypes as ct
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

MU = np.array([0.01, 0.5, 1.0, 1.5, 2.0, 3.0])
TAU = 1.0 / np.array([0.1, 0.2, 0.3, 0.3, 0.35, 0.4]) ** 2
SCHED = (500, 200, 1000)


def sampler_child(lib_path, npz):
    """Times icnv_bayes_sample_dev of the library at lib_path through ctypes alone, so a library of another commit loads."""
    d = np.load(npz)
    L, off, tok = d["L"], np.ascontiguousarray(d["off"], dtype=np.int64), np.ascontiguousarray(d["token"], dtype=np.uint64)
    lib = ct.CDLL(lib_path)
    torch.cuda.set_device(0)
    assert lib.icnv_init(0) == 0
    Ld = torch.from_numpy(L).cuda()
    R, K = off.size - 1, L.shape[1]
    theta = torch.empty((R, K, K), dtype=torch.float64, device="cuda")
    freq = torch.empty((L.shape[0], K), dtype=torch.int32, device="cuda")
    fn = lib.icnv_bayes_sample_dev
    fn.restype = ct.c_int
    fn.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_int32, ct.c_int32, ct.c_int32, ct.c_int32, ct.c_int32, ct.c_uint64,
                   ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p]
    ms = []
    for _ in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = fn(Ld.data_ptr(), off.ctypes.data, tok.ctypes.data, R, K, *SCHED, 7, theta.data_ptr(), None, freq.data_ptr(), None)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        assert rc == 0, rc
    print(json.dumps({"ms": ms[1:], "theta_sum": float(theta.nan_to_num().sum().item()), "freq_sum": int(freq.sum().item())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=10000)
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--share", type=float, default=0.1)
    ap.add_argument("--slice", type=int, default=2000)
    ap.add_argument("--old-slice", type=int, default=200)
    ap.add_argument("--baseline-lib")
    ap.add_argument("--sampler-child", nargs=2, metavar=("LIB", "NPZ"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_bayes_cells.json"))
    a = ap.parse_args()
    if a.sampler_child:
        return sampler_child(*a.sampler_child)

    from bench_cnv_reports import make_object, slice_object
    from infercnv_amd import _lib, bayes_net, cnv_regions, device
    torch.cuda.set_device(0)
    device.init(0)
    G, C = a.genes, a.cells
    obj = make_object(G, C, a.share, 2)
    states = obj.expr_data
    x = torch.randn((C, G), dtype=torch.float64, device="cuda") * 0.3 + 1.0
    res = {"bench": "bayes_cells", "G": G, "C": C, "share": a.share, "device": torch.cuda.get_device_name(0), "schedule": SCHED}

    def clock(fn, label=None):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(f"[bench_bayes_cells] {label or fn.__name__}: {dt:.3f} s", file=sys.stderr, flush=True)
        return out, dt

    with tempfile.TemporaryDirectory() as tmp:
        clock(lambda: cnv_regions.generate_cnv_region_reports(obj, "17_HMM_pred", tmp, ignore_neutral_state=3, by="cell"), "step-17 reports")
        m = bayes_net.MCMCInferCNV(infercnv_obj=obj)
        m.args = {"HMM_type": "i6", "postMcmcMethod": "removeCNV", "reassignCNVs": True, "out_dir": os.path.join(tmp, "bayes"),
                  "BayesMaxPNormal": 0, "seed": 7, "n_adapt": SCHED[0], "n_burn": SCHED[1], "n_keep": SCHED[2], "keep_samples": False,
                  "by": "cell"}
        m.mu, m.sig, m.x_dev = MU, TAU, x

        def build():
            t = bayes_net.RegionTable.from_states(obj, states, "cell", 3)
            bayes_net._attach_table(m, t)
            m.group_id = t.group_id(C)
            return t

        t, res["table_s"] = clock(build, "table")
        res["regions"] = len(t)
        device.bayes_stats(reset=True)
        _, res["mcmc_s"] = clock(lambda: bayes_net.run_mcmc_table(m), "mcmc")     # the two device calls and the host's share of getProbabilities
        res["bayes_stats"] = device.bayes_stats(reset=True)
        res["loglik_s"], res["sampler_s"] = res["bayes_stats"]["loglik_us"] / 1e6, res["bayes_stats"]["us"] / 1e6
        (f, new_states), res["filter_s"] = clock(lambda: bayes_net.filterHighPNormals(m, states, 0.2), "filter")
        res["regions_kept"], res["cells_changed"] = len(f.table), int((new_states != states).any(axis=0).sum())
        _, res["adjusted_s"] = clock(lambda: cnv_regions.adjust_genes_regions_report(f, "17_HMM_pred", "adjusted", tmp), "adjusted reports")
        res["adjusted_bytes"] = sum(os.path.getsize(os.path.join(tmp, "adjusted" + s)) for s in (".pred_cnv_genes.dat", ".pred_cnv_regions.dat"))
        del f, new_states

        small = slice_object(obj, a.old_slice)
        xs = x[torch.as_tensor(np.concatenate([obj.observation_grouped_cell_indices["tumor"][: a.old_slice // 2],
                                               obj.reference_grouped_cell_indices["normal"][: a.old_slice - a.old_slice // 2]]), device="cuda")]
        cnv_regions.generate_cnv_region_reports(small, "17_small", tmp, ignore_neutral_state=3, by="cell")

        def old_route():
            md = bayes_net.inferCNVBayesNet(small, small.expr_data, "i6", by="cell", seed=7, mu=MU, sig=TAU, x=xs.contiguous())
            fd, _ = bayes_net.filterHighPNormals(md, small.expr_data, 0.2)
            cnv_regions.adjust_genes_regions_report(fd, "17_small", "adjusted_small", tmp)
            return len(md.cnv_regions)

        n_old, old_s = clock(old_route, "old route on the slice")
        new_s = res["table_s"] + res["mcmc_s"] + res["filter_s"] + res["adjusted_s"]
        res["old_route"] = {"cells": a.old_slice, "regions": n_old, "s": old_s, "regions_per_s": n_old / old_s,
                            "extrapolated_s_at_full_size": len(t) / (n_old / old_s), "note": "a rate from a slice, not a measurement at size"}
        res["new_route_regions_per_s"] = len(t) / new_s

        if a.baseline_lib:
            cut = int(np.searchsorted(t.col, a.slice))           # by cell a group is a cell: the regions of the first cells
            npz = os.path.join(tmp, "slice.npz")
            off = t.cell_off[: cut + 1]
            _, L, _ = device.bayes_loglik_arrays(x, t.row_first[:cut], t.gene_count[:cut], t.cell_idx[: int(off[-1])], off, MU, TAU)
            np.savez(npz, L=L.cpu().numpy(), off=off, token=t.token[:cut])
            runs = {}
            for name, lib in (("parent", a.baseline_lib), ("this", _lib.LIB_PATH)):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--sampler-child", lib, npz], capture_output=True,
                                     text=True, timeout=900)
                if out.returncode != 0:
                    raise RuntimeError(f"sampler child ({name}) failed: {out.stderr[-2000:]}")
                runs[name] = json.loads(out.stdout.strip().splitlines()[-1])
            med = {k: float(np.median(v["ms"])) for k, v in runs.items()}
            spread = max(max(v["ms"]) - min(v["ms"]) for v in runs.values())
            ratio = med["parent"] / med["this"]
            res["packed"] = {"cells": a.slice, "regions": cut, "parent_ms": runs["parent"]["ms"], "this_ms": runs["this"]["ms"],
                             "parent_median_ms": med["parent"], "this_median_ms": med["this"], "spread_ms": spread, "ratio": ratio,
                             "same_output": runs["parent"]["theta_sum"] == runs["this"]["theta_sum"]
                             and runs["parent"]["freq_sum"] == runs["this"]["freq_sum"],
                             "faster_by_more_than_the_spread": med["parent"] - med["this"] > spread,
                             "verdict": "met" if ratio >= 2 and med["parent"] - med["this"] > spread else "missed (ratio below 2)"}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
