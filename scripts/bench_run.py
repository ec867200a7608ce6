#!/usr/bin/env python3
"""Benchmark of infercnv_amd.run (pipeline.py): wall time per step of the whole pipeline.  Prints ONE JSON line (and writes it
with --out, default profiles/bench_run.json).

Input: integer counts rint(2^x - 1) of synth.make_matrix_np(10 000, 50 000) -- two reference groups, four observation groups.
After a warm-up run on a 2 000-cell slice, three timed runs:
  denoise_stepwise   run(HMM=False, denoise=True, no_plot=True) with on_step set: the stepwise route, per-step wall time
                     from the hook's time stamps (a step's time includes everything since the previous hook call)
  hmm_stepwise       run(HMM=True, HMM_type="i6", analysis_mode="subclusters", leiden_method="simple",
                     write_expr_matrix=True) with on_step set (plots on: write_expr_matrix only acts through plot_cnv)
  denoise_fused      the first configuration without on_step: the fused route's total
Two legs (--leg host | resident | both, default both), each with the three runs (DESIGN K32):
  host       the object as CreateInfercnvObject returns it: every step goes through a host-buffer entry.  This is the code
             path of the commits before K32, unchanged: the yardstick.
  resident   obj.to_device() first (timed and counted as `to_device`): every step goes through the `_dev` entries.
Per step, next to the wall time, the bytes that crossed PCIe each way since the previous hook call: the library's own count
of its host-buffer entries (icnv_host_path_stats) plus what Python moved with Tensor.cuda / Tensor.cpu / Tensor.to.
No target and no ratio is set in advance: nobody has measured either leg."""
import argparse
import ctypes as ct
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from infercnv_amd import GeneOrder, InfercnvObject, _lib, device, run, synth  # noqa: E402


def make_object(G, C):
    x, chr_start = synth.make_matrix_np(G, C)
    counts = np.asfortranarray(np.rint(np.exp2(x) - 1.0).astype(np.int32))
    del x
    refs, obs = synth.groups(C)
    chrs = np.array([f"chr{i + 1}" for i in range(len(chr_start) - 1)])[np.repeat(np.arange(len(chr_start) - 1), np.diff(chr_start))]
    return InfercnvObject(expr_data=counts, count_data=counts, gene_order=GeneOrder(chr=chrs),
                          reference_grouped_cell_indices={f"ref{i}": g for i, g in enumerate(refs)},
                          observation_grouped_cell_indices={f"obs{i}": g for i, g in enumerate(obs)})


class Crossings:
    """Bytes across PCIe each way: the library's host-buffer entries (icnv_host_path_stats) and torch's own copies."""

    def __init__(self):
        self.up = self.down = 0
        self.L = _lib.load()
        cuda, cpu, to = torch.Tensor.cuda, torch.Tensor.cpu, torch.Tensor.to
        me = self

        def count(before, after):
            n = after.numel() * after.element_size()
            if after.is_cuda and not before.is_cuda:
                me.up += n
            elif before.is_cuda and not after.is_cuda:
                me.down += n
            return after

        torch.Tensor.cuda = lambda t, *a, **k: count(t, cuda(t, *a, **k))
        torch.Tensor.cpu = lambda t, *a, **k: count(t, cpu(t, *a, **k))
        torch.Tensor.to = lambda t, *a, **k: count(t, to(t, *a, **k))

    def read(self):
        buf = (ct.c_double * 12)()
        self.L.icnv_host_path_stats(buf, 12)
        return self.up + int(buf[5]), self.down + int(buf[7])


CROSSINGS = None


def timed_run(obj, hooked, **kw):
    steps, last = [], [None]
    bytes_last = [CROSSINGS.read()]

    def hook(step, label, _o):
        torch.cuda.synchronize()
        now = time.perf_counter()
        up, down = CROSSINGS.read()
        steps.append({"step": step, "label": label, "s": now - last[0], "bytes_up": up - bytes_last[0][0],
                      "bytes_down": down - bytes_last[0][1]})
        last[0] = now
        bytes_last[0] = (up, down)

    with tempfile.TemporaryDirectory() as tmp:
        torch.cuda.synchronize()
        start_bytes = CROSSINGS.read()
        t0 = last[0] = time.perf_counter()
        out = run(obj, out_dir=os.path.join(tmp, "out"), on_step=hook if hooked else None, **kw)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
        files = sorted(os.listdir(os.path.join(tmp, "out")))
    end_bytes = CROSSINGS.read()
    res = {"total_s": total, "genes_out": int(out.expr_data.shape[0]), "n_files": len(files),
           "bytes_up": end_bytes[0] - start_bytes[0], "bytes_down": end_bytes[1] - start_bytes[1]}
    if hooked:
        res["steps"] = steps
        res["after_last_step_s"] = time.perf_counter() - last[0]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=10000)
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--skip-hmm", action="store_true", help="time the two denoise configurations only")
    ap.add_argument("--leg", choices=("host", "resident", "both"), default="both")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_run.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_run.py needs a GPU")
    torch.cuda.set_device(0)
    device.init(0)
    denoise = dict(HMM=False, denoise=True, no_plot=True)
    hmm = dict(HMM=True, HMM_type="i6", analysis_mode="subclusters", leiden_method="simple", write_expr_matrix=True)
    global CROSSINGS
    CROSSINGS = Crossings()
    warm = make_object(a.genes, min(a.cells, 2000))                                      # warm-up: library, pools, code objects
    timed_run(warm, True, **denoise)
    if a.leg != "host":
        timed_run(warm.to_device(), True, **denoise)
    host_obj = make_object(a.genes, a.cells)
    res = {"bench": "run", "device": torch.cuda.get_device_name(0), "genes": a.genes, "cells": a.cells,
           "date": time.strftime("%Y-%m-%d"), "measured": True, "ref_groups": 2, "obs_groups": 4, "legs": {}}
    for leg in (("host", "resident") if a.leg == "both" else (a.leg,)):
        out = res["legs"][leg] = {}
        obj = host_obj
        if leg == "resident":
            b0, t0 = CROSSINGS.read(), time.perf_counter()
            obj = host_obj.to_device()
            torch.cuda.synchronize()
            b1 = CROSSINGS.read()
            out["to_device"] = {"s": time.perf_counter() - t0, "bytes_up": b1[0] - b0[0], "bytes_down": b1[1] - b0[1]}
        for name, hooked, kw in (("denoise_stepwise", True, denoise), ("hmm_stepwise", True, hmm), ("denoise_fused", False, denoise)):
            if name == "hmm_stepwise" and a.skip_hmm:
                continue
            out[name] = timed_run(obj, hooked, **kw)
            print(f"[bench_run] {leg} {name}: {out[name]['total_s']:.2f} s, {out[name]['bytes_up'] / 1e9:.2f} GB up, "
                  f"{out[name]['bytes_down'] / 1e9:.2f} GB down", file=sys.stderr, flush=True)
        del obj
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
