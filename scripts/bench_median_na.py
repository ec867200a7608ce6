"""What the NA-aware median filter costs (K19), at bench.py configuration 5's shape and by its method.

The input is built as bench.py builds configuration 5's: the synthetic 10 000 x 50 000 matrix through the smoothing chain
(the denoised matrix apply_median_filtering runs on), tiles = synth.subclusters (about 500 cells each), window_size 7;
every leg is warmed up, then timed by a host clock around `steps` calls that end in a device synchronise.  One run times,
interleaved round by round:

  plain        icnv_median_filter_dev                           (its code is untouched: the parent commit's time)
  na_clean     icnv_median_filter_na_dev on the same NaN-free matrix   (expected: plain + one read of the matrix)
  na_1e-6      icnv_median_filter_na_dev with a NaN share of 1e-6
  na_1e-3      icnv_median_filter_na_dev with a NaN share of 1e-3
  stream       a read-only stream of the matrix (torch.sum over its 4 GB)

and writes one JSON object (profiles/bench_median_na.json holds the recorded run).  The overhead of the NaN-free call,
na_clean - plain, is accepted up to 1.5 x the stream time of the same run (the mask stores and one launch).

    python scripts/bench_median_na.py [--genes 10000] [--cells 50000] [--steps 10] [--warmup 3] [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=10000)
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from infercnv_amd import device, sharded, synth
    if not torch.cuda.is_available():
        raise SystemExit("bench_median_na.py needs a GPU: nothing is measured without one")
    torch.cuda.set_device(0)
    device.init(0)
    G, C = args.genes, args.cells
    subs, _, _ = synth.subclusters(C)
    tiles = [np.asarray(g, dtype=np.int32) for g in subs]
    x, chr_start = synth.make_matrix_torch(G, C, "cuda", C_total=C)
    refs, _ = synth.groups(C)
    plan = device.ChainPlan(G, C, chr_start, sharded.localize_groups(refs, 0, C))
    out, _ = sharded.ShardedChain(plan).run(x, want_pre_denoise=False)
    del x, plan
    gen = torch.Generator(device="cuda")
    gen.manual_seed(19)
    inputs = {"plain": out, "na_clean": out}
    n_nan = {}
    for share in (1e-6, 1e-3):
        xn = out.clone()
        n = int(round(share * G * C))
        pos = torch.randint(0, G * C, (n,), device="cuda", generator=gen)
        xn.view(-1)[pos] = float("nan")
        inputs["na_%g" % share] = xn
        n_nan["na_%g" % share] = int(torch.isnan(xn).sum().item())
    res = torch.empty_like(out)
    counts = {}

    def call(leg):
        if leg == "stream":
            return inputs["plain"].sum()
        if leg == "plain":
            return device.median_filter(inputs[leg], chr_start, tiles, 7, out=res)
        _, counts[leg] = device.median_filter(inputs[leg], chr_start, tiles, 7, out=res, na_aware=True, return_na_count=True)

    legs = ["plain", "na_clean", "na_1e-06", "na_0.001", "stream"]
    assert set(legs) - {"stream"} == set(inputs), sorted(inputs)
    for leg in legs:
        for _ in range(args.warmup):
            call(leg)
    torch.cuda.synchronize()
    assert counts["na_clean"] == 0 and all(counts[k] == n_nan[k] for k in n_nan), (counts, n_nan)
    # the NaN-free NA-aware call returns the plain call's matrix
    want = device.median_filter(out, chr_start, tiles, 7)
    call("na_clean")
    torch.cuda.synchronize()
    assert torch.equal(res.view(torch.int64), want.view(torch.int64))
    del want
    ms = {leg: [] for leg in legs}
    for _ in range(args.rounds):          # interleaved rounds in one process
        for leg in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                call(leg)
            torch.cuda.synchronize()
            ms[leg].append((time.perf_counter() - t0) / args.steps * 1e3)
    # the kernel families of one NaN-free and one 1e-3 call (event timers, a run of their own)
    kern = {}
    for leg in ("na_clean", "na_0.001"):
        device.timing_reset()
        device.timing_enable(True)
        for _ in range(3):
            call(leg)
        torch.cuda.synchronize()
        kern[leg] = {}
        for name in ("median_na_scan", "median_na_clean", "median_filter", "median_na_fixup"):
            t, n = device.timing_get(name)
            if n:
                kern[leg][name] = t / n
        device.timing_enable(False)
    med = {leg: float(np.median(v)) for leg, v in ms.items()}
    bytes_matrix = 8.0 * G * C
    result = {
        "what": "icnv_median_filter_na_dev against icnv_median_filter_dev, bench.py configuration 5's input and method",
        "genes": G, "cells": C, "tiles": len(tiles), "window_size": 7, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
        "ms_per_call_median": med, "ms_per_call_rounds": ms, "nan_elements": n_nan,
        "stream": {"what": "torch.sum over the matrix (read-only)", "GB_per_s": bytes_matrix / med["stream"] / 1e6},
        "overhead_nan_free_ms": med["na_clean"] - med["plain"],
        "overhead_nan_free_over_stream": (med["na_clean"] - med["plain"]) / med["stream"],
        "accepted_overhead_over_stream": 1.5,
        "kernel_ms_per_call": kern,
        "scan_GB_per_s": bytes_matrix / kern["na_clean"]["median_na_scan"] / 1e6 if "median_na_scan" in kern["na_clean"] else None,
    }
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
