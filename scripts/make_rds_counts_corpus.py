#!/usr/bin/env python3
"""Writes the corpus that infercnv_amd/csrc/rds_counts_host_check (the per-element routines of K34 on the host, under the
sanitizers) runs over: big-endian payloads and the results tests/rds_counts_restate.py gives for them.
    "RCC1"; per record uint8 kind (13 INTSXP, 14 REALSXP, 1 the count test on doubles), uint8 residue of the payload's address
    mod 16, uint16 n (little-endian), the n big-endian elements, n little-endian uint64 results (the doubles' bits; for the
    count test the count, or -1)
Every residue 0 .. 15 with every length 0 .. 70 for both kinds, the special values in front (NA_real_, NaNs with other payloads,
both zeros, the infinities, denormals; NA_integer_, INT_MIN + 1, INT_MAX, 0), and the count test's edge values at every residue.

    python scripts/make_rds_counts_corpus.py rds_counts_corpus.bin && make -C infercnv_amd/csrc rds_counts_check CORPUS=$PWD/rds_counts_corpus.bin
"""
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import rds_counts_restate as rs  # noqa: E402


def record(kind, residue, payload, results):
    return struct.pack("<BBH", kind, residue, len(results)) + payload + np.asarray(results, dtype=np.uint64).astype("<u8").tobytes()


def main(path):
    n_records = 0
    with open(path, "wb") as f:
        f.write(b"RCC1")
        for residue in range(16):
            for n in range(71):
                bits = rs.real_payload(n, 1000 * residue + n)
                payload = bits.astype(">u8").tobytes()
                f.write(record(rs.REAL, residue, payload, rs.column_bits(payload, 0, rs.REAL, n)))
                ints = rs.int_payload(n, 5000 * residue + n)
                payload = ints.astype(">i4").tobytes()
                f.write(record(rs.INT, residue, payload, rs.column_bits(payload, 0, rs.INT, n)))
                n_records += 2
            bits = np.array(rs.COUNT_SPECIALS, dtype=np.uint64)
            counts = np.array([rs.count_of(b) for b in bits], dtype=np.int64).view(np.uint64)
            f.write(record(1, residue, bits.astype(">u8").tobytes(), counts))
            n_records += 1
    print(f"{path}: {n_records} records")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "rds_counts_corpus.bin"))
