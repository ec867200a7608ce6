#!/usr/bin/env python3
"""Writes the corpus that infercnv_amd/csrc/gunzip_host_check (the K30 finder test, measure and marker decoder on the host,
under the sanitizers) runs over: the valid and the malformed raw DEFLATE streams of tests/gunzip_restate.py, each a record
    uint32 valid, uint32 name length, name, uint64 length, compressed bytes, uint64 length, inflated bytes
in native byte order.  A valid record is a WHOLE raw stream (bit 0 to the byte behind BFINAL) and what it inflates to.

    python scripts/make_gunzip_corpus.py corpus.bin && make -C infercnv_amd/csrc gunzip_check CORPUS=$PWD/corpus.bin
"""
import os
import struct
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import gunzip_restate as gr  # noqa: E402
import inflate_restate as ir  # noqa: E402


def records():
    for name, (raw, data) in gr.zlib_streams().items():
        yield name, 1, raw, data
    for name, (raw, data, _) in gr.hand_streams().items():
        yield name, int(data is not None), raw, data or b""
    raw, data = gr.planted_header()
    yield "planted_header", 1, raw, data
    gz = gr.golden_counts_gz()
    yield "golden_counts_matrix", 1, gr.gz_raw(gz), zlib.decompress(gz, 31)
    for name, (stream, _) in ir.malformed().items():
        yield name, 0, stream, b""
        yield name + "_at_bit_3", 0, shifted(stream, 3), b""


def shifted(stream, k):
    """The stream moved k bits up: k zero bits in front."""
    return (int.from_bytes(stream, "little") << k).to_bytes(len(stream) + 1, "little")


def main(path):
    n = 0
    with open(path, "wb") as f:
        for name, valid, comp, data in records():
            if valid:
                assert zlib.decompress(comp, -15) == data, name
            f.write(struct.pack("=II", valid, len(name)) + name.encode() + struct.pack("=Q", len(comp)) + comp + struct.pack("=Q", len(data)) + data)
            n += 1
    print(f"{n} streams written to {path}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "gunzip_corpus.bin")
