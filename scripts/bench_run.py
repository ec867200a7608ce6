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
No target: the parent commit has no run() to compare with, and the reference's R is not installed here."""
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

from infercnv_amd import GeneOrder, InfercnvObject, device, run, synth  # noqa: E402


def make_object(G, C):
    x, chr_start = synth.make_matrix_np(G, C)
    counts = np.asfortranarray(np.rint(np.exp2(x) - 1.0).astype(np.int32))
    del x
    refs, obs = synth.groups(C)
    chrs = np.array([f"chr{i + 1}" for i in range(len(chr_start) - 1)])[np.repeat(np.arange(len(chr_start) - 1), np.diff(chr_start))]
    return InfercnvObject(expr_data=counts, count_data=counts, gene_order=GeneOrder(chr=chrs),
                          reference_grouped_cell_indices={f"ref{i}": g for i, g in enumerate(refs)},
                          observation_grouped_cell_indices={f"obs{i}": g for i, g in enumerate(obs)})


def timed_run(obj, hooked, **kw):
    steps, last = [], [None]

    def hook(step, label, _o):
        torch.cuda.synchronize()
        now = time.perf_counter()
        steps.append({"step": step, "label": label, "s": now - last[0]})
        last[0] = now

    with tempfile.TemporaryDirectory() as tmp:
        torch.cuda.synchronize()
        t0 = last[0] = time.perf_counter()
        out = run(obj, out_dir=os.path.join(tmp, "out"), on_step=hook if hooked else None, **kw)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
        files = sorted(os.listdir(os.path.join(tmp, "out")))
    res = {"total_s": total, "genes_out": int(out.expr_data.shape[0]), "n_files": len(files)}
    if hooked:
        res["steps"] = steps
        res["after_last_step_s"] = time.perf_counter() - last[0]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=10000)
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--skip-hmm", action="store_true", help="time the two denoise configurations only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_run.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_run.py needs a GPU")
    torch.cuda.set_device(0)
    device.init(0)
    denoise = dict(HMM=False, denoise=True, no_plot=True)
    hmm = dict(HMM=True, HMM_type="i6", analysis_mode="subclusters", leiden_method="simple", write_expr_matrix=True)
    timed_run(make_object(a.genes, min(a.cells, 2000)), True, **denoise)                 # warm-up: library, pools, code objects
    obj = make_object(a.genes, a.cells)
    res = {"bench": "run", "device": torch.cuda.get_device_name(0), "genes": a.genes, "cells": a.cells,
           "date": time.strftime("%Y-%m-%d"), "measured": True, "ref_groups": 2, "obs_groups": 4}
    res["denoise_stepwise"] = timed_run(obj, True, **denoise)
    if not a.skip_hmm:
        res["hmm_stepwise"] = timed_run(obj, True, **hmm)
    res["denoise_fused"] = timed_run(obj, False, **denoise)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
