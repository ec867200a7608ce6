#!/usr/bin/env python3
"""Benchmark of the MCMC convergence diagnostics (icnv_mcmc_diag_dev, DESIGN K31).  Prints ONE JSON line and writes it to
profiles/bench_mcmc_diag.json (--out).  Two shapes, the default schedule (500 + 200 discarded, 1 000 kept, 6 chains), one process:

  subclusters  the regions of scripts/bench_bayes.py (K13): synth.make_matrix_torch(10 000, 50 000), the i6 group HMM over
               synth.subclusters(C, 500), every non-neutral run -- 423 regions at the defaults
  cells        the per-cell slice of scripts/bench_bayes_cells.py (K25): the regions of the first --slice cells of its
               synthetic per-cell states -- 52 845 regions at the defaults

Per shape, medians of three calls after a warm-up, wall clock around calls that synchronise:
  sampler_ms        device.bayes_sample(want_samples=True): what produces the samples
  mcmc_diag_ms      device.mcmc_diag alone on those samples, and its ratio to the sampler -- there is no other yardstick
  diagnostics_s     bayes_net.mcmc_diagnostics end to end (likelihoods, sampler and diagnostics in batches of --max-bytes,
                    download, the log line; no file)
restatement: tests/mcmc_diag_restate.py on --restate regions of the cells shape on one core, EXTRAPOLATED to the shape as a rate
(not a measurement at size)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

import numpy as np  # noqa: E402
import torch  # noqa: E402

SCHED = (500, 200, 1000)
MU = np.array([0.01, 0.5, 1.0, 1.5, 2.0, 3.0])
TAU = 1.0 / np.array([0.1, 0.2, 0.3, 0.3, 0.35, 0.4]) ** 2


def timed(fn, reps=3):
    fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), [round(v, 3) for v in ms]


def measure(name, m, L, off, tokens, max_bytes):
    """m: the MCMCInferCNV object of the shape; L, off, tokens: its likelihoods, for the two device calls alone."""
    from infercnv_amd import bayes_net, device
    K, R = L.shape[1], len(tokens)
    samples = device.bayes_sample(L, off, tokens, *SCHED, seed=7, want_samples=True)[1]
    r = {"regions": R, "K": K, "sample_bytes": int(samples.numel() * 8), "series": R * K * K}
    r["mcmc_diag_ms"], r["mcmc_diag_ms_all"] = timed(lambda: device.mcmc_diag(samples))
    cs, po = device.mcmc_diag(samples)
    po = po.cpu().numpy()
    r["regions_with_rhat_ge_1.1"] = int((po[:, :, 5] >= 1.1).any(axis=1).sum())
    r["min_ess"] = float(np.nanmin(po[:, :, 6]))
    del samples, cs
    r["sampler_ms"], r["sampler_ms_all"] = timed(lambda: device.bayes_sample(L, off, tokens, *SCHED, seed=7, want_samples=True))
    r["diag_over_sampler"] = r["mcmc_diag_ms"] / r["sampler_ms"]
    r["ns_per_series"] = r["mcmc_diag_ms"] * 1e6 / r["series"]
    s, s_all = timed(lambda: bayes_net.mcmc_diagnostics(m, max_sample_bytes=max_bytes))
    r["diagnostics_s"], r["diagnostics_s_all"] = s / 1e3, [round(v / 1e3, 4) for v in s_all]
    r["batches"] = -(-R // max(1, max_bytes // (K * SCHED[2] * K * 8)))
    print(f"[bench_mcmc_diag] {name}: {json.dumps(r)}", file=sys.stderr, flush=True)
    return r


def mcmc_object(obj, x):
    from infercnv_amd import bayes_net
    m = bayes_net.MCMCInferCNV(infercnv_obj=obj)
    m.args = {"HMM_type": "i6", "postMcmcMethod": "removeCNV", "reassignCNVs": True, "out_dir": None, "BayesMaxPNormal": 0, "seed": 7,
              "n_adapt": SCHED[0], "n_burn": SCHED[1], "n_keep": SCHED[2], "keep_samples": False, "by": "cell"}
    m.mu, m.sig, m.x_dev = MU, TAU, x
    return m


def subclusters_object(G, C):
    """-> (the MCMCInferCNV object of the shape, L, off, tokens)."""
    from bench_bayes import predicted_regions
    from infercnv_amd import device, synth
    from infercnv_amd.tumor_subclusters import fnv1a64
    x, chr_start = synth.make_matrix_torch(G, C, "cuda")
    refs, _ = synth.groups(C)
    _, pre = device.smooth_chain(x, chr_start, refs, want_pre_denoise=True)
    del x
    subs, _, _ = synth.subclusters(C, size=500)
    means, sd, logPi, logDelta = synth.hmm_params_i6()
    states, _ = device.viterbi_groups(pre, chr_start, subs, means, [sd / np.sqrt(len(g)) for g in subs], logPi, logDelta)
    neutral = int(np.argmax(torch.bincount(states.flatten().to(torch.int64), minlength=8).cpu().numpy()))
    regions, names, st = predicted_regions(states, subs, chr_start, neutral)
    m = mcmc_object(None, pre)
    m.mu, m.sig = np.array(synth.I6_MEANS, dtype=np.float64), 1.0 / np.array(synth.I6_SDS, dtype=np.float64) ** 2
    m.cnv_regions = names
    m.cell_gene = [{"cnv_regions": n, "Genes": np.arange(g0, g0 + ng), "Cells": c, "State": s} for n, (g0, ng, c), s in zip(names, regions, st)]
    m.cnv_probabilities = [None] * len(names)
    _, L, off = device.bayes_loglik(pre, regions, m.mu, m.sig)
    return m, L, off, [fnv1a64(n) for n in names]


def subclusters_shape(G, C, max_bytes):
    return measure("subclusters", *subclusters_object(G, C), max_bytes)


def cells_object(G, C, share, n_slice):
    """-> (the MCMCInferCNV object of the shape on the table route, L, off, tokens, the number of regions)."""
    from bench_cnv_reports import make_object
    from infercnv_amd import bayes_net, device
    obj = make_object(G, C, share, 2)
    x = torch.randn((C, G), dtype=torch.float64, device="cuda") * 0.3 + 1.0
    t = bayes_net.RegionTable.from_states(obj, obj.expr_data, "cell", 3)
    cut = int(np.searchsorted(t.col, n_slice))                  # by cell a group is a cell: the regions of the first cells
    m = mcmc_object(obj, x)
    bayes_net._attach_table(m, t.take(np.arange(cut)))
    m.cnv_probabilities = bayes_net._LazySeq(cut, lambda r: None)
    t = m.table
    _, L, off = device.bayes_loglik_arrays(x, t.row_first, t.gene_count, t.cell_idx, t.cell_off, MU, TAU)
    return m, L, off, t.token, cut


def cells_shape(G, C, share, n_slice, max_bytes, n_restate):
    from infercnv_amd import bayes_net
    m, L, off, tokens, cut = cells_object(G, C, share, n_slice)
    r = measure("cells", m, L, off, tokens, max_bytes)
    r["cells"] = n_slice
    restate = None
    if n_restate:
        sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
        import mcmc_diag_restate as mr
        pick = np.linspace(0, cut - 1, n_restate).astype(int)
        host = torch.cat([bayes_net._resample(m, int(i), int(i) + 1) for i in pick]).cpu().numpy()
        t0 = time.perf_counter()
        mr.diag(host)
        per = (time.perf_counter() - t0) / len(pick)
        restate = {"regions_timed": len(pick), "ms_per_region_one_core": per * 1e3, "extrapolated_s_for_the_cells_shape": per * cut,
                   "note": "a rate from a few regions, not a measurement at size"}
    return r, restate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=10000)
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--share", type=float, default=0.1)
    ap.add_argument("--slice", type=int, default=2000)
    ap.add_argument("--max-bytes", type=int, default=2 << 30)
    ap.add_argument("--restate", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_mcmc_diag.json"))
    a = ap.parse_args()
    from infercnv_amd import device
    torch.cuda.set_device(0)
    device.init(0)
    res = {"bench": "mcmc_diag", "G": a.genes, "C": a.cells, "device": torch.cuda.get_device_name(0), "schedule": SCHED,
           "max_sample_bytes": a.max_bytes}
    res["subclusters"] = subclusters_shape(a.genes, a.cells, a.max_bytes)
    torch.cuda.empty_cache()
    res["cells"], res["restatement"] = cells_shape(a.genes, a.cells, a.share, a.slice, a.max_bytes, a.restate)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
