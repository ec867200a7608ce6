#!/usr/bin/env python3
"""Benchmark of the per-cell CNV feature table and the run-length segmentation (icnv_cnv_features_dev / icnv_cnv_runs_dev, DESIGN
K14) on the state matrix of scripts/bench_bayes.py's setup: synth.make_matrix_torch(10 000, 50 000), the smoothing chain's HMM
input and the i6 group HMM over synth.subclusters(C, 500).  Prints ONE JSON line (and writes it with --out).

  features  the counting pass: wall ms of the call and the kernel's own ms (the library's event timers), the kernel's share of
            8 TB/s on its algorithmic bytes (G C + outputs); beside it device.state_consensus over the same matrix in the same
            run, which also reads every state byte once (expectation, not a bar: features <= consensus)
  runs      the segmentation by cell (every column, report order) and by subcluster (consensus columns); beside it the host
            baseline: the NumPy loop per (column, chromosome) that scripts/bench_bayes.py carried, fed with a device-to-host
            copy of the same states, copy included -- by cell on the first --host-cells columns (the device is timed on the
            same columns for the ratio, and on all of them)
  add_to_seurat  the whole mirror by subcluster and by cell, split into device time, top-n and file writing

Times are wall clock around whole calls (each synchronises) after a warm-up call; the median is reported."""
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

from infercnv_amd import device, seurat_interaction, synth  # noqa: E402
from infercnv_amd.infercnv_object import GeneOrder, InfercnvObject  # noqa: E402


def timed(fn, reps):
    out, ms = None, []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, ms


def kernel_ms(name, fn, reps):
    """Per-launch milliseconds of one kernel family from the library's event timers, in a window of its own."""
    device.timing_enable(True)
    device.timing_reset()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    ms, n = device.timing_get(name)
    device.timing_enable(False)
    return ms / max(n, 1)


def host_segmentation(rows, chr_start, neutral):
    """The host baseline: run-length segmentation per (column, chromosome) of a host (columns, genes) state array, the loop
    scripts/bench_bayes.py::predicted_regions carried before the device path: (column, first gene, gene count, state) per
    non-neutral run."""
    out = []
    for q in range(rows.shape[0]):
        for c in range(len(chr_start) - 1):
            a, b = int(chr_start[c]), int(chr_start[c + 1])
            if b - a < 2:
                continue
            s = rows[q, a:b]
            cuts = np.concatenate([[0], np.nonzero(s[1:] != s[:-1])[0] + 1, [b - a]])
            for u, v in zip(cuts[:-1], cuts[1:]):
                if s[u] != neutral:
                    out.append((q, a + int(u), int(v - u), int(s[u])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=10000)
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-cells", type=int, default=50000)
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
    del pre
    hist = torch.bincount(states.flatten().to(torch.int64), minlength=8).cpu().numpy()
    s0 = 3
    n_chr = len(chr_start) - 1
    res = {"bench": "cnv_summary", "G": G, "C": C, "K": K, "device": torch.cuda.get_device_name(0), "subclusters": len(subs),
           "state_histogram": hist.tolist(), "center_state": s0, "viterbi_underflows": int(bad.item())}

    # ---- the counting pass beside the consensus
    feat = lambda: device.cnv_features(states, chr_start, K, s0, want_run_counts=True)   # noqa: E731
    cons_fn = lambda: device.state_consensus(states, subs)   # noqa: E731
    feat(), cons_fn()
    (counts, run_counts), ms_f = timed(feat, a.reps)
    cons, ms_c = timed(cons_fn, a.reps)
    kf, kc = kernel_ms("cnvsum_features", feat, a.reps), kernel_ms("state_consensus", cons_fn, a.reps)
    byts = G * C + n_chr * C * 16 + C * 8
    res["features"] = {"ms": float(np.median(ms_f)), "ms_all": [round(v, 3) for v in ms_f], "kernel_ms": kf, "algorithmic_bytes": byts,
                       "kernel_share_of_8TBps": byts / (kf * 1e-3) / 8e12 if kf > 0 else None,
                       "state_consensus_ms": float(np.median(ms_c)), "state_consensus_kernel_ms": kc,
                       "kernel_ratio_features_over_consensus": kf / kc if kc > 0 else None,
                       "expectation": "features kernel <= state_consensus kernel", "verdict": "met" if kf <= kc else "missed",
                       "non_neutral_runs": int(run_counts[:, 1].sum().item()), "runs": int(run_counts[:, 0].sum().item())}

    # ---- the segmentation
    order = np.concatenate([np.asarray(g, dtype=np.int32) for g in refs + obs])
    by_cell = lambda: device.cnv_runs(states, chr_start, neutral=s0, K=K, col_idx=order)   # noqa: E731
    by_cell()
    (rec, n_runs), ms_cell = timed(by_cell, a.reps)
    by_sub = lambda: device.cnv_runs(cons, chr_start, neutral=s0, K=K)   # noqa: E731
    by_sub()
    (rec_sub, _), ms_sub = timed(by_sub, a.reps)
    n_host = min(a.host_cells, C)
    part = states[:n_host]
    dev_part = lambda: device.cnv_runs(part, chr_start, neutral=s0, K=K)   # noqa: E731
    dev_part()
    (rec_part, _), ms_part = timed(dev_part, a.reps)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = host_segmentation(part.cpu().numpy(), chr_start, s0)
    host_s = time.perf_counter() - t0
    got = rec_part.cpu().numpy()
    assert len(host) == got.shape[1] and all((int(got[0, i]), int(got[2, i]), int(got[3, i] - got[2, i] + 1), int(got[4, i])) == h
                                             for i, h in enumerate(host[:100000])), "device and host segmentation differ"
    t0 = time.perf_counter()
    first = torch.as_tensor(np.array([int(g[0]) for g in subs]), device=states.device)
    host_sub = host_segmentation(states[first].cpu().numpy(), chr_start, s0)
    host_sub_s = time.perf_counter() - t0
    assert len(host_sub) == rec_sub.shape[1]
    res["runs"] = {"by_cell": {"ms": float(np.median(ms_cell)), "ms_all": [round(v, 3) for v in ms_cell], "columns": C,
                               "records": int(rec.shape[1]), "runs": int(n_runs),
                               "kernel_ms": kernel_ms("cnvsum_runs", by_cell, 2), "count_kernel_ms": kernel_ms("cnvsum_run_counts", by_cell, 2)},
                   "by_subcluster": {"ms": float(np.median(ms_sub)), "ms_all": [round(v, 3) for v in ms_sub], "columns": len(subs),
                                     "records": int(rec_sub.shape[1]), "host_loop_s": host_sub_s,
                                     "host_over_device": host_sub_s * 1e3 / float(np.median(ms_sub))},
                   "host_baseline_by_cell": {"columns": n_host, "host_loop_s_copy_included": host_s, "device_ms_same_columns": float(np.median(ms_part)),
                                             "host_over_device": host_s * 1e3 / float(np.median(ms_part)),
                                             "note": "both on the first `columns` columns; nothing is extrapolated"}}

    # ---- the whole mirror
    chrs = np.concatenate([np.full(int(chr_start[k + 1] - chr_start[k]), f"chr{k + 1}") for k in range(n_chr)])
    pos = np.concatenate([np.arange(int(chr_start[k + 1] - chr_start[k]), dtype=np.int64) * 100000 + 1 for k in range(n_chr)])
    ref_set = [i for i, r in enumerate(is_ref) if r]
    tree = {"normal": {f"normal_s{i + 1}": np.asarray(subs[q], dtype=np.int32) for i, q in enumerate(ref_set)},
            "tumor": {f"tumor_s{i + 1}": np.asarray(subs[q], dtype=np.int32) for i, q in enumerate(q for q in range(len(subs)) if not is_ref[q])}}
    obj = InfercnvObject(expr_data=np.empty((G, C), dtype=np.uint8), gene_order=GeneOrder(chrs, pos, pos + 50000),
                         reference_grouped_cell_indices={"normal": np.concatenate([np.asarray(g, dtype=np.int32) for g in refs])},
                         observation_grouped_cell_indices={"tumor": np.concatenate([np.asarray(g, dtype=np.int32) for g in obs])},
                         tumor_subclusters={"subclusters": tree})
    res["add_to_seurat"] = {}
    for mode, by_cells in (("by_subcluster", False), ("by_cell", True)):
        with tempfile.TemporaryDirectory() as tmp:
            # three separate runs: the device part alone, get_features (device + top-n), the whole mirror (+ table and files)
            _, ms_dev = timed(lambda: seurat_interaction.device_pass(obj, states, "i6", by_cells), 2)
            _, ms_feat = timed(lambda: seurat_interaction.get_features(obj, states, "i6", by_cells), 1)
            out, ms_all = timed(lambda: seurat_interaction.add_to_seurat(obj, states, tmp, HMM_type="i6", by_cells=by_cells), 1)
            dev_s, feat_s, total = ms_dev[-1] * 1e-3, ms_feat[0] * 1e-3, ms_all[0] * 1e-3
            res["add_to_seurat"][mode] = {"total_s": total, "device_s": dev_s, "top_n_s": feat_s - dev_s, "write_s": total - feat_s,
                                          "note": "top_n_s and write_s are differences of separately timed runs",
                                          "top_loss": len(out["features"]["top_loss"]), "top_dupli": len(out["features"]["top_dupli"]),
                                          "table_bytes": os.path.getsize(os.path.join(tmp, "map_metadata_from_infercnv.txt"))}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
