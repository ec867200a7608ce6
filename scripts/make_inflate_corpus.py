#!/usr/bin/env python3
"""Writes the corpus that infercnv_amd/csrc/inflate_host_check (the K29 parser on the host, under the sanitizers) runs over: the
valid and the malformed streams of tests/inflate_restate.py, each a record
    uint32 valid, uint32 expected status, uint32 name length, name, uint64 length, compressed bytes, uint64 length, inflated bytes
in native byte order.  A valid record holds ONE unit from byte 0 (bytes behind it are allowed) and what it inflates to.

    python scripts/make_inflate_corpus.py corpus.bin && make -C infercnv_amd/csrc inflate_check CORPUS=$PWD/corpus.bin
"""
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import deflate_restate as dr  # noqa: E402
import inflate_restate as ir  # noqa: E402


def records():
    for name, (stream, data, status) in ir.hand_units().items():
        yield name, 1, status, stream, data
    comp, data = ir.long_unit()
    yield "long_unit", 1, ir.OK_MARKER, comp, data
    for piece in (256, 16384):
        for pname, payload in dr.payloads(piece).items():
            if piece == 16384 and pname not in ("fibonacci", "count_like", "len_piece", "zeros", "match_past_end"):
                continue
            for vname, pieces in ir.zlib_variants(payload, piece).items():
                for i in (0, len(pieces) - 1):
                    yield f"{pname}_{piece}_{vname}_{i}", 1, ir.OK_MARKER, pieces[i], payload[i * piece:(i + 1) * piece]
    stream = ir.sync_flush_stream([b"first part " * 30, b"first part again " * 10])
    first = ir.unit(stream)
    yield "sync_flush_first", 1, ir.OK_MARKER, stream, first[3]
    yield "sync_flush_second", 0, ir.NEEDS_HISTORY, stream[first[1]:], b""
    for name, (stream, status) in ir.malformed().items():
        yield name, 0, status, stream, b""


def main(path):
    n = 0
    with open(path, "wb") as f:
        for name, valid, status, comp, data in records():
            if valid:
                got = ir.unit(comp)
                assert got[0] == status and got[3] == data, name          # the corpus states what the restatement finds
            f.write(struct.pack("=III", valid, status, len(name)) + name.encode() + struct.pack("=Q", len(comp)) + comp +
                    struct.pack("=Q", len(data)) + data)
            n += 1
    print(f"{n} streams written to {path}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "inflate_corpus.bin")
