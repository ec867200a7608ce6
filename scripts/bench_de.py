#!/usr/bin/env python3
"""Benchmark of the non-DE gene masking (icnv_de_tests_dev / icnv_mask_non_de_dev, DESIGN K12) on
synth.make_matrix_np(10 000, 50 000) with synth.subclusters(C, size=500): 2 normal types of 2 500 cells, 92 observation
subclusters, 184 comparisons.  Prints ONE JSON line (and writes it with --out).

  a   wilcoxon with jitter, through BH                       target <= 150 ms
  b   t (Welch), through BH                                  target <= 30 ms
  c   the full mask_non_DE_genes_basic, data on the device   target <= 200 ms
  d   samples mode: the 4 observation groups of 11 250 cells as single subclusters (report)

Times are wall clock around whole calls (each synchronises) after a warm-up call; the median is reported.  --scipy also
times SciPy's vectorised mannwhitneyu / ttest_ind on the host for 4 comparisons of (a) (context only)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from infercnv_amd import GeneOrder, InfercnvObject, device, synth  # noqa: E402
from infercnv_amd.mask_non_de import _comparisons, mask_non_de_device  # noqa: E402


def timed(fn, reps):
    out, ms = None, []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, ms


def make_obj(G, C, samples_mode=False):
    subs, is_ref, _ = synth.subclusters(C, size=500)
    refs, obs = synth.groups(C)
    obj = InfercnvObject(expr_data=np.zeros((0, 0)), gene_order=GeneOrder(chr=np.array(["1"] * G)),
                         reference_grouped_cell_indices={f"normal_{k}": r for k, r in enumerate(refs)},
                         observation_grouped_cell_indices={f"tumor_{q}": o for q, o in enumerate(obs)})
    if samples_mode:
        obj.tumor_subclusters = {"subclusters": {f"tumor_{q}": {f"tumor_{q}": o} for q, o in enumerate(obs)}}
    else:
        tum = {f"tumor_{q}": {} for q in range(len(obs))}
        obs_sets = [set(o.tolist()) for o in obs]
        n = 0
        for s, r in zip(subs, is_ref):
            if r:
                continue
            q = next(i for i, st in enumerate(obs_sets) if int(s[0]) in st)
            tum[f"tumor_{q}"][f"tumor_{q}.{n}"] = s
            n += 1
        obj.tumor_subclusters = {"subclusters": tum}
    return obj


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=10000)
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scipy", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    device.init(0)
    G, C = a.genes, a.cells
    xh, _ = synth.make_matrix_np(G, C)
    x = torch.from_numpy(np.ascontiguousarray(xh.T)).cuda()
    res = {"bench": "de", "G": G, "C": C, "device": torch.cuda.get_device_name(0)}
    targets = {"a": 150.0, "b": 30.0, "c": 200.0}
    for case, samples in (("a", False), ("b", False), ("c", False), ("d", True)):
        obj = make_obj(G, C, samples)
        groups, pairs, _ = _comparisons(obj)
        if case == "c":
            out = torch.empty_like(x)
            fn = lambda: mask_non_de_device(x, obj, out=out)   # noqa: E731
        else:
            test = "t" if case == "b" else "wilcoxon"
            fn = lambda: device.de_tests(x, groups, pairs, test=test, jitter=True)   # noqa: E731
        fn()
        device.de_stats(reset=True)
        _, ms = timed(fn, a.reps)
        st = device.de_stats()
        r = {"ms": float(np.median(ms)), "ms_all": [round(v, 3) for v in ms], "comparisons": len(pairs),
             "waves_per_call": st["waves"] / a.reps, "segments_hbm_per_call": st["segments_hbm"] / a.reps}
        if case in targets:
            r["target_ms"] = targets[case]
            r["verdict"] = "met" if r["ms"] <= targets[case] else "missed"
        res[case] = r
    if a.scipy:
        from scipy import stats
        obj = make_obj(G, C)
        groups, pairs, _ = _comparisons(obj)
        t0 = time.perf_counter()
        for k, q in pairs[:4]:
            stats.mannwhitneyu(xh[:, groups[k]], xh[:, groups[q]], axis=1, method="asymptotic")
        t1 = time.perf_counter()
        for k, q in pairs[:4]:
            stats.ttest_ind(xh[:, groups[k]], xh[:, groups[q]], axis=1, equal_var=False)
        t2 = time.perf_counter()
        res["scipy_host_ms_per_comparison"] = {"mannwhitneyu": (t1 - t0) * 250.0, "ttest_ind": (t2 - t1) * 250.0}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
