#!/usr/bin/env python3
"""Writes the corpus that infercnv_amd/csrc/mcmc_diag_host_check (the per-series routines of the K31 diagnostics on the host,
under the sanitizers) runs over: seeded series of tests/mcmc_diag_restate.py and the restatement's outputs for them, in native
byte order:
    "MCMCDIAG", int32 n_cases; per case int32 n_chains, n_keep, int32 windows[3][3] (lo, m, P), float64 x[n_chains][n_keep],
    chain_stats[n_chains][9], pooled[7]
The cases cover the smallest schedule, both parities of the window ends, the lag-50 boundary, the default schedule, the 8 192
limit at 6 and 8 chains, the largest AR order (2 x 4096), a constant series, NaN and tied values with -0.0.

    python scripts/make_mcmc_diag_corpus.py corpus.bin && make -C infercnv_amd/csrc mcmc_diag_check CORPUS=$PWD/corpus.bin
"""
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import mcmc_diag_restate as mr  # noqa: E402

CASES = [("ar1", 3, 20), ("white", 3, 21), ("dirichlet", 6, 50), ("ar1", 6, 51), ("dirichlet", 6, 64), ("white", 2, 100),
         ("dirichlet", 6, 1000), ("ar1", 6, 1365), ("dirichlet", 8, 1024), ("ar1", 2, 4096), ("constant", 3, 100), ("nan", 3, 20),
         ("ties", 4, 37)]


def main(path):
    with open(path, "wb") as f:
        f.write(b"MCMCDIAG" + struct.pack("=i", len(CASES)))
        for i, (kind, m, n) in enumerate(CASES):
            x = np.ascontiguousarray(mr.make_series(kind, m, n, 100 + i))
            if kind == "constant":
                x[1] = mr.make_series("white", 1, n, 7)[0]      # one chain moves: W > 0
            cs = np.array([mr.chain_stats(x[ch]) for ch in range(m)])
            po = np.array(mr.pooled_stats(x, cs))
            win = [v for lo, w in mr.windows(n) for v in (lo, w, mr.max_order(w))]
            f.write(struct.pack("=2i9i", m, n, *win) + x.tobytes() + cs.tobytes() + po.tobytes())
    print(f"{path}: {len(CASES)} cases")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "mcmc_diag_corpus.bin")
