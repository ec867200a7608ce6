"""Helpers of the K28 tests (tests/test_deflate_host.py, tests/test_gpu_deflate.py): the payloads at which a DEFLATE
compressor can go wrong, the checks every piece must pass under zlib's inflate, and a host stand-in for the device
compressor that produces pieces of the contract's shape (raw zlib with a Z_FULL_FLUSH per piece)."""
from __future__ import annotations

import struct
import zlib

import numpy as np

FINAL_BLOCK = b"\x03\x00"          # an empty final fixed-Huffman block: ends a raw DEFLATE stream on the spot


def be_doubles(a):
    return np.asarray(a, dtype=">f8").tobytes()


def state_like(n_values, seed=1):
    """HMM states as doubles: runs of 1..6 (mostly 3) with geometric lengths."""
    rng = np.random.default_rng(seed)
    out = np.empty(n_values, dtype=np.float64)
    i = 0
    while i < n_values:
        run = int(rng.geometric(1 / 150.0))
        out[i:i + run] = 3.0 if rng.random() < 0.6 else float(rng.integers(1, 7))
        i += run
    return be_doubles(out)


def count_like(n_values, seed=2):
    """Counts as doubles: Poisson(0.15), 86 % zeros."""
    return be_doubles(np.random.default_rng(seed).poisson(0.15, n_values).astype(np.float64))


def denoised_like(n_values, seed=3):
    """Smoothed expression N(1, 0.05) with the noise band (1.5 sd) set to 1.0."""
    x = np.random.default_rng(seed).normal(1.0, 0.05, n_values)
    x[np.abs(x - 1.0) < 0.075] = 1.0
    return be_doubles(x)


def smoothed_like(n_values, seed=4):
    return be_doubles(np.random.default_rng(seed).normal(1.0, 0.05, n_values))


def random_bytes(n, seed=5):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def fibonacci_bytes(piece):
    """Byte frequencies in Fibonacci proportion filling one piece: an unrestricted Huffman tree of these is deeper than 15.  The
    bytes are shuffled (seeded) so that matches do not swallow the literals."""
    fib = [1, 1]
    while sum(fib) + fib[-1] + fib[-2] <= piece:
        fib.append(fib[-1] + fib[-2])
    vals = np.concatenate([np.full(f, i, dtype=np.uint8) for i, f in enumerate(fib)])
    vals = np.concatenate([vals, np.full(piece - vals.size, len(fib) - 1, dtype=np.uint8)])
    np.random.default_rng(6).shuffle(vals)
    return vals.tobytes()


def payloads(piece):
    """name -> bytes: the edge payloads of the issue for the piece size `piece`."""
    rnd = random_bytes(3 * piece + 5, 7)
    out = {f"len_{k}": rnd[:n] for k, n in (("1", 1), ("7", 7), ("8", 8), ("piece_minus_1", piece - 1), ("piece", piece),
                                            ("piece_plus_1", piece + 1), ("3_pieces_plus_5", 3 * piece + 5))}
    out["zeros"] = bytes(2 * piece + 3)                                          # length-258 matches at distance 8 and 1
    out["one_double"] = be_doubles(np.full(piece // 8 + 3, 1.0625))
    out["state_like"] = state_like(3 * piece // 8 + 1)
    out["count_like"] = count_like(3 * piece // 8 + 1)
    out["denoised_like"] = denoised_like(3 * piece // 8 + 1)
    out["smoothed_like"] = smoothed_like(2 * piece // 8)
    out["one_byte_value"] = b"\xab" * piece                                      # a one-symbol literal tree
    out["all_bytes_equal"] = bytes(np.random.default_rng(8).permutation(np.arange(piece, dtype=np.int64) % 256).astype(np.uint8))
    out["fibonacci"] = fibonacci_bytes(piece)
    block = random_bytes(600, 9)
    out["far_repeat"] = block + random_bytes(32768 + 200, 10) + block           # the only repeat lies more than 32 768 bytes back
    out["match_past_end"] = random_bytes(piece - 100, 11) + b"\x11\x22\x33\x44\x55" * 140        # a repeat that runs across the piece's end
    return out


def check_piece(comp: bytes, data: bytes, crc: int, bound: int, where=""):
    """The per-piece checks of the contract."""
    assert len(comp) <= bound, f"{where}: {len(comp)} bytes, the bound is {bound}"
    d = zlib.decompressobj(-15)
    assert d.decompress(comp) == data, f"{where}: the piece does not inflate to its input"
    assert d.unused_data == b"" and not d.eof, f"{where}: a final block, or bytes behind one"
    d = zlib.decompressobj(-15)
    assert d.decompress(comp + FINAL_BLOCK) == data and d.eof and d.unused_data == b"", f"{where}: the piece does not end on a byte boundary"
    assert crc == zlib.crc32(data), f"{where}: CRC {crc:#010x}, zlib says {zlib.crc32(data):#010x}"


def check_stream(packed: bytes, data: bytes):
    d = zlib.decompressobj(-15)
    assert d.decompress(packed + FINAL_BLOCK) == data and d.eof and d.unused_data == b""


def host_pieces(data: bytes, piece: int, level=1):
    """The stand-in: [(compressed piece, crc, input length)] with no BFINAL, no reference before the piece, byte aligned."""
    out = []
    for o in range(0, len(data), piece):
        part = data[o:o + piece]
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        out.append((c.compress(part) + c.flush(zlib.Z_FULL_FLUSH), zlib.crc32(part), len(part)))
    return out


def gzip_parts(blob: bytes):
    """(header, raw deflate stream, crc, isize) of a one-member gzip file with the plain 10-byte header."""
    crc, isize = struct.unpack("<II", blob[-8:])
    return blob[:10], blob[10:-8], crc, isize
