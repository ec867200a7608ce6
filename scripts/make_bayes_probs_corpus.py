#!/usr/bin/env python3
"""Writes the corpus that infercnv_amd/csrc/bayes_probs_host_check (the box statistics of K33 on the host, under the sanitizers)
runs over: the pooled draws of seeded (region, state) series of tests/bayes_probs_restate.py and the restatement's seven fields
for them, in native byte order:
    "BAYESBOX", int32 n_cases; per case int32 N, float64 y[N], box[7]
The cases cover the smallest series (two draws), odd and even lengths, the default schedule, the 8 192 limit, draws planted on
and beyond the fences, a constant series, tied values with both zeros, and NaN.

    python scripts/make_bayes_probs_corpus.py corpus.bin && make -C infercnv_amd/csrc bayes_probs_check CORPUS=$PWD/corpus.bin
"""
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import bayes_probs_restate as pr  # noqa: E402

SHAPES = [(2, 1, 2), (3, 1, 3), (2, 20, 2), (3, 21, 3), (6, 100, 6), (6, 1000, 6), (8, 1024, 8), (5, 37, 4)]   # (n_chains, n_keep, K)


def main(path):
    n_cases = 0
    with open(path, "wb") as f:
        f.write(b"BAYESBOX" + struct.pack("=i", 0))
        for i, (m, n, K) in enumerate(SHAPES):
            s = pr.make_box_samples(3, m, n, K, 200 + i)
            for r in range(3):
                for k in range(K):
                    y = np.ascontiguousarray(s[r, :, :, k]).ravel()
                    f.write(struct.pack("=i", y.size) + y.tobytes() + np.array(pr.box_stats(y), dtype=np.float64).tobytes())
                    n_cases += 1
        f.seek(8)
        f.write(struct.pack("=i", n_cases))
    print(f"{path}: {n_cases} cases")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "bayes_probs_corpus.bin")
