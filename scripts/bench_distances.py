#!/usr/bin/env python3
"""Time icnv_cell_distances_dev (R's sequential dist, DESIGN K7) on one tumor group of the bench workload (developer
tool; run on the GPU box).  Reports the kernel's pair-gene rate against the fp64 VALU ideal of 3 non-FMA operations
(sub, mul, add) per pair-gene.
usage: bench_distances.py [cells_in_group] [genes] [out.json]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from infercnv_amd import device, synth
n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
G = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
out = sys.argv[3] if len(sys.argv) > 3 else None
VALU_OPS_PER_S = 78.6e12 / 2     # 78.6 TFLOP/s fp64 vector counts an FMA as 2; one non-FMA op per lane-cycle
torch.cuda.set_device(0); device.init(0)
x, cs = synth.make_matrix_torch(G, n, "cuda")
cells = np.arange(n, dtype=np.int32)
d = device.cell_distances(x, cells); torch.cuda.synchronize()
device.timing_reset(); device.timing_enable(True)
reps = 3
for _ in range(reps): d = device.cell_distances(x, cells)
torch.cuda.synchronize(); device.timing_enable(False)
ms, k = device.timing_get("exact_dist")
ms /= k
nt128 = (n + 127) // 128
DT = 128 if nt128 * (nt128 + 1) // 2 >= 2 * torch.cuda.get_device_properties(0).multi_processor_count else 64   # exact_dist_plan's rule
nt = (n + DT - 1) // DT
pair_genes = n * (n - 1) / 2 * G                        # the contract's work: each unordered pair once
executed = nt * (nt + 1) / 2 * DT * DT * G               # upper-triangular tiles, diagonal tiles in full
ideal_ms = 3 * pair_genes / VALU_OPS_PER_S * 1e3
r = {"bench": "cell_distances", "device": torch.cuda.get_device_name(0), "cells": n, "genes": G, "tile": DT,
     "exact_dist_ms": round(ms, 2), "reps": reps, "pair_genes": pair_genes, "executed_pair_genes": executed,
     "valu_ideal_ms": round(ideal_ms, 2), "fraction_of_valu_ideal": round(ideal_ms / ms, 3),
     "fraction_of_valu_ideal_executed": round(3 * executed / VALU_OPS_PER_S * 1e3 / ms, 3)}
print(json.dumps(r))
if out:
    with open(out, "w") as fh:
        fh.write(json.dumps(r) + "\n")
