#!/usr/bin/env python3
"""Benchmark of the Bayesian filter of the predicted CNV regions (icnv_bayes_loglik_dev / icnv_bayes_sample_dev, DESIGN K13)
on synth.make_matrix_torch(10 000, 50 000): the smoothing chain's HMM input, the i6 group HMM over synth.subclusters(C, 500),
and the regions that HMM predicts (every run of a non-neutral state of a subcluster within a chromosome).  Prints ONE JSON
line (and writes it with --out).

  loglik   the likelihood pass over all regions, beside device.group_means over the same subclusters in the same run
           (target: <= 2 x its time; group_means reads every cell's column, the pass only the regions' rectangles)
  sample   the sampler, default schedule (500 + 200 + 1 000 iterations, 6 chains): ms per call, ns per iteration per
           (region, chain) of the whole call (throughput) and us per iteration of one workgroup (latency: the call has fewer
           workgroups than the device has slots when that is so), the share of decided cells; the same with the
           decided-cell shortcut off (ICNV_BAYES_DECIDED=0)
  samples  HMM_analysis_mode = "samples": one region set per whole observation group (report)
  restate  --restate N: tests/bayes_restate.py on one core for N regions with a short schedule, extrapolated

Times are wall clock around whole calls (each synchronises) after a warm-up call; the median is reported."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from infercnv_amd import device, synth  # noqa: E402
from infercnv_amd.tumor_subclusters import fnv1a64  # noqa: E402


def timed(fn, reps):
    out, ms = None, []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, ms


def predicted_regions(states, groups, chr_start, neutral):
    """Run-length segmentation per (group, chromosome) of the group's state row (the group HMM gives every cell of a group the
    same states) on the device (icnv_cnv_runs_dev): (first gene, gene count, cells) and a name per non-neutral run -- this
    script's own names, which number the non-neutral runs only."""
    first = torch.as_tensor(np.array([int(g[0]) for g in groups]), device=states.device)
    rec, _ = device.cnv_runs(states[first].contiguous(), chr_start, neutral=neutral)
    rec = rec.cpu().numpy()
    cells = [np.sort(np.asarray(g, dtype=np.int32)) for g in groups]
    regions = [(int(a), int(b - a + 1), cells[q]) for q, a, b in zip(rec[0], rec[2], rec[3])]
    names = [f"chr{c + 1}-region_{i + 1}" for i, c in enumerate(rec[1])]
    return regions, names, [int(v) for v in rec[4]]


def sampler_case(L, off, tokens, sched, reps, K):
    fn = lambda: device.bayes_sample(L, off, tokens, *sched)   # noqa: E731
    fn()
    device.bayes_stats(reset=True)
    _, ms = timed(fn, reps)
    st = device.bayes_stats()
    T = sum(sched)
    med = float(np.median(ms))
    R = len(tokens)
    return {"ms": med, "ms_all": [round(v, 3) for v in ms], "iterations": T,
            "ns_per_iteration_per_region_chain": med * 1e6 / (T * R * K), "us_per_iteration_of_the_call": med * 1e3 / T,
            "rows": st["rows"] // reps, "undecided_rows": st["undecided_rows"] // reps,
            "decided_share": 1.0 - st["undecided_rows"] / max(st["rows"], 1),
            "regions_lds": st["regions_lds"] // reps, "regions_streamed": st["regions_streamed"] // reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=10000)
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--restate", type=int, default=0)
    ap.add_argument("--out")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    device.init(0)
    G, C, K = a.genes, a.cells, 6
    x, chr_start = synth.make_matrix_torch(G, C, "cuda")
    refs, obs = synth.groups(C)
    _, pre = device.smooth_chain(x, chr_start, refs, want_pre_denoise=True)
    del x
    subs, is_ref, _ = synth.subclusters(C, size=500)
    means, sd, logPi, logDelta = synth.hmm_params_i6()
    states, bad = device.viterbi_groups(pre, chr_start, subs, means, [sd / np.sqrt(len(g)) for g in subs], logPi, logDelta)
    hist = torch.bincount(states.flatten().to(torch.int64), minlength=8).cpu().numpy()
    neutral = int(np.argmax(hist))
    mu = np.array(synth.I6_MEANS, dtype=np.float64)
    tau = 1.0 / np.array(synth.I6_SDS, dtype=np.float64) ** 2
    res = {"bench": "bayes", "G": G, "C": C, "K": K, "device": torch.cuda.get_device_name(0), "subclusters": len(subs),
           "state_histogram": hist.tolist(), "neutral_state": neutral, "viterbi_underflows": int(bad.item())}
    sched = (500, 200, 1000)
    for mode, groups in (("subclusters", subs), ("samples", refs + obs)):
        if mode == "samples":
            states, _ = device.viterbi_groups(pre, chr_start, groups, means, [sd / np.sqrt(len(g)) for g in groups], logPi, logDelta)
        regions, names, _ = predicted_regions(states, groups, chr_start, neutral)
        r = {"regions": len(regions)}
        if regions:
            tokens = [fnv1a64(n) for n in names]
            r["genes_per_region_median"] = float(np.median([ng for _, ng, _ in regions]))
            r["matrix_share_read"] = float(sum(ng * len(c) for _, ng, c in regions)) / (G * C)
            fn = lambda: device.bayes_loglik(pre, regions, mu, tau)   # noqa: E731
            (ll, L, off), _ = timed(fn, 1)
            _, ms = timed(fn, a.reps)
            gm = lambda: device.group_means(pre, groups)   # noqa: E731
            gm()
            _, ms_gm = timed(gm, a.reps)
            r["loglik"] = {"ms": float(np.median(ms)), "ms_all": [round(v, 3) for v in ms], "group_means_ms": float(np.median(ms_gm)),
                           "target": "<= 2 x group_means", "verdict": "met" if np.median(ms) <= 2 * np.median(ms_gm) else "missed"}
            del ll
            r["sample"] = sampler_case(L, off, tokens, sched, a.reps, K)
            os.environ["ICNV_BAYES_DECIDED"] = "0"
            r["sample_every_cell"] = sampler_case(L, off, tokens, sched, 1, K)
            del os.environ["ICNV_BAYES_DECIDED"]
            if mode == "subclusters" and a.restate:
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                sys.path.insert(0, os.path.join(ROOT, "oracle"))
                import bayes_restate as br
                Lh = L.cpu().numpy()
                pick = np.linspace(0, len(regions) - 1, a.restate).astype(int)
                short = (10, 5, 15)
                t0 = time.perf_counter()
                for i in pick:
                    br.sample_region(Lh[off[i]:off[i + 1]], tokens[i], K, *short)
                per = (time.perf_counter() - t0) / (len(pick) * K * sum(short))
                r["restatement_one_core"] = {"regions_timed": len(pick), "us_per_iteration_per_region_chain": per * 1e6,
                                             "extrapolated_s_per_call": per * K * sum(sched) * len(regions)}
        res[mode] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
