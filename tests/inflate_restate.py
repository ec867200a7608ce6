"""Helpers of the K29 tests (tests/test_inflate_host.py, tests/test_gpu_inflate.py): a plain sequential reader of RFC 1951
written from the RFC, which gives for one unit of the contract (include/icnv.h "INFLATE in independent units") its
(status, end, out_len, bytes); the writers the hand-built streams are made with; the valid and the malformed streams of the
tests; and the four device calls restated on the host for the tests of rds.inflate_gzip's chain walk.

A unit starts on a byte boundary and runs up to and including the first empty stored block, or a block with BFINAL."""
from __future__ import annotations

import functools
import gzip
import io
import struct
import zlib

import numpy as np

import deflate_restate as dr

OK_MARKER, OK_FINAL, TRUNCATED, TOO_LONG, BAD_STREAM, NEEDS_HISTORY = range(6)
MARKER = b"\x00\x00\xff\xff"
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


# ================================================================================================================ the reader
def canonical(lengths):
    """symbol -> (code, length) of the canonical Huffman code of RFC 1951 section 3.2.2."""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def reverse(code, length):
    return int(format(code, f"0{length}b")[::-1], 2) if length else 0


def space_left(lengths):
    """2^15 scaled Kraft space left by the lengths: > 0 incomplete, < 0 over-subscribed."""
    return (1 << 15) - sum(1 << (15 - l) for l in lengths if l)


class _Code:
    """A code as a dict from (the length marker bit | the bits in stream order) to the symbol."""

    def __init__(self, lengths):
        self.table = {(1 << l) | reverse(c, l): s for s, (c, l) in canonical(lengths).items()}
        used = [l for l in lengths if l]
        self.lo, self.hi = (min(used), max(used)) if used else (1, 0)
        self.used = len(used)


class _Dry(Exception):
    pass


class _Bad(Exception):
    def __init__(self, status=BAD_STREAM):
        self.status = status


class _Reader:
    def __init__(self, src, start, limit):
        self.src, self.p, self.limit, self.bb, self.bc = src, start, limit, 0, 0

    def need(self, k):
        if self.bc < k:
            chunk = self.src[self.p:min(self.p + 8, self.limit)]
            self.bb |= int.from_bytes(chunk, "little") << self.bc
            self.bc += 8 * len(chunk)
            self.p += len(chunk)
            if self.bc < k:
                raise _Dry()

    def take(self, k):
        self.need(k)
        v = self.bb & ((1 << k) - 1)
        self.bb >>= k
        self.bc -= k
        return v

    def symbol(self, code):
        """Bit by bit: the first length at which the bits read so far are a code word."""
        if self.bc < 15:
            try:
                self.need(15)
            except _Dry:
                pass
        bb, table = self.bb, code.table
        for l in range(1, 16):
            if l > self.bc:
                raise _Dry()
            if code.lo <= l <= code.hi:
                s = table.get((1 << l) | (bb & ((1 << l) - 1)))
                if s is not None:
                    self.bb >>= l
                    self.bc -= l
                    return s
        raise _Bad()

    def byte_pos(self):
        return (self.p * 8 - self.bc + 7) // 8


def _code_or_bad(lengths, strict):
    left = space_left(lengths)
    used = [l for l in lengths if l]
    if left < 0:
        raise _Bad()
    if left > 0 and (strict or not (len(used) == 0 or used == [1])):
        raise _Bad()
    return _Code(lengths)


FIXED_LIT = _Code([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = _Code([5] * 32)


def _dynamic(r):
    nlen, ndist, ncode = r.take(5) + 257, r.take(5) + 1, r.take(4) + 4
    if nlen > 286 or ndist > 30:
        raise _Bad()
    cl = [0] * 19
    for i in range(ncode):
        cl[CL_ORDER[i]] = r.take(3)
    clc = _code_or_bad(cl, strict=True)
    lengths = []
    while len(lengths) < nlen + ndist:
        s = r.symbol(clc)
        if s < 16:
            lengths.append(s)
            continue
        if s == 16:
            if not lengths:
                raise _Bad()
            value, rep = lengths[-1], 3 + r.take(2)
        elif s == 17:
            value, rep = 0, 3 + r.take(3)
        else:
            value, rep = 0, 11 + r.take(7)
        if len(lengths) + rep > nlen + ndist:
            raise _Bad()
        lengths += [value] * rep
    if lengths[256] == 0:
        raise _Bad()
    return _code_or_bad(lengths[:nlen], strict=False), _code_or_bad(lengths[nlen:], strict=False)


def unit(src, start=0, max_in=None):
    """(status, end, out_len, bytes) of the unit that starts at byte `start` of src.  With a status other than OK_*, end and the
    bytes are where the reader stood."""
    n = len(src)
    limit = n if max_in is None or max_in >= n - start else start + max_in
    dry = TOO_LONG if limit < n else TRUNCATED
    r = _Reader(src, start, limit)
    out = bytearray()
    try:
        while True:
            last, kind = r.take(1), r.take(2)
            if kind == 3:
                raise _Bad()
            if kind == 0:
                q = r.byte_pos()
                r.bb, r.bc, r.p = 0, 0, q
                if q + 4 > limit:
                    raise _Dry()
                ln, nln = struct.unpack_from("<HH", src, q)
                if ln ^ 0xFFFF != nln:
                    raise _Bad()
                r.p = q + 4
                if ln == 0:
                    return (OK_FINAL if last else OK_MARKER), r.p, len(out), bytes(out)
                if r.p + ln > limit:
                    raise _Dry()
                out += src[r.p:r.p + ln]
                r.p += ln
            else:
                lit, dist = (FIXED_LIT, FIXED_DIST) if kind == 1 else _dynamic(r)
                while True:
                    s = r.symbol(lit)
                    if s < 256:
                        out.append(s)
                        continue
                    if s == 256:
                        break
                    if s >= 286:
                        raise _Bad()
                    ln = LEN_BASE[s - 257] + r.take(LEN_EXTRA[s - 257])
                    if dist.used == 0:
                        raise _Bad()
                    d = r.symbol(dist)
                    if d >= 30:
                        raise _Bad()
                    d = DIST_BASE[d] + r.take(DIST_EXTRA[d])
                    if d > len(out):
                        raise _Bad(NEEDS_HISTORY)
                    if d >= ln:
                        out += out[len(out) - d:len(out) - d + ln]
                    else:
                        period = bytes(out[len(out) - d:])
                        out += (period * (ln // d + 1))[:ln]
            if last:
                return OK_FINAL, r.byte_pos(), len(out), bytes(out)
    except _Dry:
        return dry, r.byte_pos(), len(out), bytes(out)
    except _Bad as bad:
        return bad.status, r.byte_pos(), len(out), bytes(out)


@functools.lru_cache(maxsize=None)
def unit_cached(src: bytes, start=0, max_in=None):
    return unit(src, start, max_in)


def candidates(src):
    """The offsets p in [4, len(src)] with src[p - 4:p] the marker, ascending."""
    out, at = [], bytes(src).find(MARKER)
    while at >= 0:
        out.append(at + 4)
        at = bytes(src).find(MARKER, at + 1)
    return out


def chain(src, start=0):
    """[(start, status, end, out_len, bytes)] of the units from `start` on, each begun where the one before ended."""
    out = []
    while True:
        st, end, n, data = unit(src, start)
        out.append((start, st, end, n, data))
        if st != OK_MARKER:
            return out
        start = end


# ================================================================================================================ the writers
class BitWriter:
    def __init__(self):
        self.acc, self.n = 0, 0

    def bits(self, value, k):
        """k bits of value, least significant first (header fields, extra bits)."""
        self.acc |= (value & ((1 << k) - 1)) << self.n
        self.n += k
        return self

    def code(self, pair):
        """A Huffman code word (code, length): most significant bit first."""
        c, l = pair
        return self.bits(reverse(c, l), l)

    def pad(self):
        self.n = -(-self.n // 8) * 8
        return self

    def raw(self, b):
        self.pad()
        for x in b:
            self.bits(x, 8)
        return self

    def bytes(self):
        return self.acc.to_bytes(-(-self.n // 8), "little")


def flat_lengths(symbols):
    """A complete code over the given symbols with lengths that differ by at most one (one symbol: length 1)."""
    k = len(symbols)
    if k == 1:
        return {symbols[0]: 1}
    top = (k - 1).bit_length()
    short = (1 << top) - k
    return {s: (top - 1 if i < short else top) for i, s in enumerate(sorted(symbols))}


def len_token(length):
    c = max(i for i in range(29) if LEN_BASE[i] <= length and (i == 28) == (length == 258))
    return 257 + c, length - LEN_BASE[c], LEN_EXTRA[c]


def dist_token(dist):
    c = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return c, dist - DIST_BASE[c], DIST_EXTRA[c]


def stored_block(w, data, final=False, nlen=None):
    w.bits(1 if final else 0, 1).bits(0, 2).pad()
    ln = len(data)
    return w.raw(struct.pack("<HH", ln, (ln ^ 0xFFFF) if nlen is None else nlen) + bytes(data))


def write_tokens(w, tokens, lit, dist):
    """tokens: ints (literals) and (length, distance) pairs; lit / dist: symbol -> (code, length).  The end-of-block code last."""
    for t in tokens:
        if isinstance(t, int):
            w.code(lit[t])
            continue
        s, ev, eb = len_token(t[0])
        w.code(lit[s]).bits(ev, eb)
        c, ev, eb = dist_token(t[1])
        w.code(dist[c]).bits(ev, eb)
    return w.code(lit[256])


def fixed_block(w, tokens, final=False):
    w.bits(1 if final else 0, 1).bits(1, 2)
    return write_tokens(w, tokens, canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), canonical([5] * 32))


def dynamic_header(w, lit_lens, dist_lens, final=False, nlen=None, ndist=None, cl_lens=None, sequence=None):
    """The header of a dynamic block.  lit_lens / dist_lens: symbol -> length.  By default every length is written as itself (no
    repeat codes) under a complete code-length code over the symbols 0 .. 18; `sequence` replaces the length sequence by a list
    of (code-length symbol, extra value); cl_lens the code-length code's lengths (19 of them)."""
    nlen = max(257, max(lit_lens) + 1) if nlen is None else nlen
    ndist = max(1, max(dist_lens, default=0) + 1) if ndist is None else ndist
    if sequence is None:
        sequence = [(lit_lens.get(s, 0), 0) for s in range(nlen)] + [(dist_lens.get(s, 0), 0) for s in range(ndist)]
    if cl_lens is None:
        cl_lens = [flat_lengths(list(range(19)))[s] for s in range(19)]
    clc = canonical(cl_lens)
    w.bits(1 if final else 0, 1).bits(2, 2).bits(nlen - 257, 5).bits(ndist - 1, 5).bits(19 - 4, 4)
    for s in CL_ORDER:
        w.bits(cl_lens[s], 3)
    for s, extra in sequence:
        w.code(clc[s])
        if s >= 16:
            w.bits(extra, {16: 2, 17: 3, 18: 7}[s])
    return w


def dynamic_block(w, tokens, final=False, extra_dist=()):
    """A dynamic block over exactly the symbols the tokens use (flat codes)."""
    lits = {256} | {t if isinstance(t, int) else len_token(t[0])[0] for t in tokens}
    dists = {dist_token(t[1])[0] for t in tokens if not isinstance(t, int)} | set(extra_dist)
    lit_lens, dist_lens = flat_lengths(sorted(lits)), (flat_lengths(sorted(dists)) if dists else {})
    dynamic_header(w, lit_lens, dist_lens, final)
    full = lambda lens, n: canonical([lens.get(s, 0) for s in range(n)])
    return write_tokens(w, tokens, full(lit_lens, 286), full(dist_lens, 30))


def end_marker(w):
    """The empty stored block of a sync flush."""
    return stored_block(w, b"")


def apply_tokens(tokens):
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return bytes(out)


# ================================================================================================================ the streams
STRATEGIES = {"fixed": zlib.Z_FIXED, "huffman_only": zlib.Z_HUFFMAN_ONLY, "rle": zlib.Z_RLE}
LEVELS = (0, 1, 6, 9)


def pieces_with(data, piece, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8):
    """deflate_restate.host_pieces with a strategy: every piece on its own, ended by a Z_FULL_FLUSH."""
    out = []
    for o in range(0, len(data), piece):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
        out.append(c.compress(data[o:o + piece]) + c.flush(zlib.Z_FULL_FLUSH))
    return out


def zlib_variants(data, piece):
    """name -> list of compressed pieces: the levels through deflate_restate.host_pieces, the strategies at level 6."""
    out = {f"level_{l}": [p[0] for p in dr.host_pieces(data, piece, l)] for l in LEVELS}
    out.update({name: pieces_with(data, piece, 6, st) for name, st in STRATEGIES.items()})
    return out


def hand_units():
    """name -> (stream, expected bytes, expected status): the valid hand-built units of the issue."""
    rng = np.random.default_rng(29)
    out = {}

    def add(name, w, tokens_bytes, status=OK_MARKER):
        out[name] = (w.bytes(), tokens_bytes, status)

    toks = [int(x) for x in rng.integers(0, 256, 300)]
    w = BitWriter()
    lits = flat_lengths(sorted({256} | set(toks)))
    dynamic_header(w, lits, {}, ndist=1)                                    # HDIST = 1: one distance code of length zero
    write_tokens(w, toks, canonical([lits.get(s, 0) for s in range(286)]), {})
    add("literal_only_dynamic", end_marker(w), bytes(toks))

    toks = [65, 66, 67, (3, 3), 68, (5, 3), (9, 3)]
    add("single_distance_code", end_marker(dynamic_block(BitWriter(), toks)), apply_tokens(toks))

    toks = [7, (258, 1), (258, 1), 9, (200, 2), 1, 2, 3, (100, 3), (7, 5), (258, 7)]
    add("distance_1_length_258_and_overlaps", end_marker(dynamic_block(BitWriter(), toks)), apply_tokens(toks))
    add("overlaps_fixed", end_marker(fixed_block(BitWriter(), toks)), apply_tokens(toks))

    head = [int(x) for x in rng.integers(0, 256, 64)]
    toks = head + [(258, 64)] * 126 + [(196, 64)] + [(258, 32768), (64, 32768), (3, 1)]     # 64 + 32 704 = 32 768 bytes, then the far match
    add("distance_32768", end_marker(dynamic_block(BitWriter(), toks)), apply_tokens(toks))

    toks = [72, 105, (6, 2)]
    add("final_unit", dynamic_block(BitWriter(), toks, final=True), apply_tokens(toks), OK_FINAL)
    add("final_fixed_odd_bits", fixed_block(BitWriter(), [1, 2, 3], final=True), bytes([1, 2, 3]), OK_FINAL)
    add("empty_stored_only", end_marker(BitWriter()), b"")
    add("empty_stored_final", stored_block(BitWriter(), b"", final=True), b"", OK_FINAL)
    first = [ord(c) for c in "stored first, "]
    second, third = [ord(c) for c in "then fixed, "] + [(6, 7)], [ord(c) for c in "then dynamic"] + [(12, 12), (20, 40)]
    w = fixed_block(stored_block(BitWriter(), bytes(first)), second)        # the later blocks refer back into the earlier ones
    add("stored_fixed_dynamic", end_marker(dynamic_block(w, third)), apply_tokens(first + second + third))
    return out


@functools.lru_cache(maxsize=None)
def long_unit():
    """About 200 KB of output from one compress() call without flushes: several blocks that start at non-zero bit offsets,
    then the sync flush."""
    rng = np.random.default_rng(31)
    data = dr.denoised_like(9000, 32) + rng.integers(0, 4, 60000, dtype=np.uint8).tobytes() + dr.count_like(8000, 33) + dr.random_bytes(5000, 34)
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 5)                          # memLevel 5: a block every 4 096 symbols
    return c.compress(data) + c.flush(zlib.Z_SYNC_FLUSH), data


def sample_dynamic():
    """One valid dynamic unit with matches, for the cuts and the flips."""
    data = dr.smoothed_like(200, 36) + dr.count_like(200, 35)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    comp = c.compress(data) + c.flush(zlib.Z_SYNC_FLUSH)
    assert comp[0] & 7 == 4                                                 # BFINAL 0, BTYPE 10
    return comp, data


def dynamic_header_bytes(comp):
    """The number of whole bytes the dynamic header of comp's first block spans."""
    r = _Reader(comp, 0, len(comp))
    r.take(3)
    _dynamic(r)
    return r.byte_pos()


def malformed():
    """name -> (stream, expected status): every BAD_STREAM cause of the contract and NEEDS_HISTORY."""
    out = {}
    flat19 = [flat_lengths(list(range(19)))[s] for s in range(19)]
    out["btype_11"] = (bytes([0b110, 0, 0, 0, 0]), BAD_STREAM)
    out["stored_len_nlen"] = (stored_block(BitWriter(), b"abcde", nlen=0x1234).bytes(), BAD_STREAM)
    ok_lit = {65: 1, 256: 1}
    # literal/length code: over-subscribed, incomplete with two codes, no end-of-block
    out["lit_oversubscribed"] = (dynamic_header(BitWriter(), {65: 1, 66: 1, 256: 1}, {}).bytes() + bytes(8), BAD_STREAM)
    out["lit_incomplete"] = (dynamic_header(BitWriter(), {65: 2, 256: 2}, {}).bytes() + bytes(8), BAD_STREAM)
    out["lit_no_end_of_block"] = (dynamic_header(BitWriter(), {65: 1, 66: 1}, {}).bytes() + bytes(8), BAD_STREAM)
    out["dist_oversubscribed"] = (dynamic_header(BitWriter(), ok_lit, {0: 1, 1: 1, 2: 1}).bytes() + bytes(8), BAD_STREAM)
    out["dist_incomplete"] = (dynamic_header(BitWriter(), ok_lit, {0: 2, 1: 2}).bytes() + bytes(8), BAD_STREAM)
    # the code-length code: over-subscribed, incomplete (a single code is not accepted here)
    over = list(flat19)
    over[0] = 1
    out["cl_oversubscribed"] = (dynamic_header(BitWriter(), ok_lit, {}, cl_lens=over, sequence=[]).bytes() + bytes(8), BAD_STREAM)
    single = [0] * 19
    single[1] = 1
    out["cl_incomplete"] = (dynamic_header(BitWriter(), ok_lit, {}, cl_lens=single, sequence=[]).bytes() + bytes(8), BAD_STREAM)
    out["repeat_with_nothing_before"] = (dynamic_header(BitWriter(), ok_lit, {}, sequence=[(16, 0)]).bytes() + bytes(8), BAD_STREAM)
    seq = [(18, 127)] + [(18, 127 - 21)] + [(1, 0)] + [(18, 0)]             # 138 + 117 + 1 = 256 lengths, then 11 zeros past 257 + 1
    out["lengths_past_the_end"] = (dynamic_header(BitWriter(), ok_lit, {}, sequence=seq).bytes() + bytes(8), BAD_STREAM)
    out["hlit_287"] = (dynamic_header(BitWriter(), ok_lit, {}, nlen=287).bytes() + bytes(8), BAD_STREAM)
    out["hdist_31"] = (dynamic_header(BitWriter(), ok_lit, {0: 1, 1: 1}, ndist=31).bytes() + bytes(8), BAD_STREAM)
    fixed_lit = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
    for s in (286, 287):
        out[f"literal_length_symbol_{s}"] = (BitWriter().bits(0, 1).bits(1, 2).code(fixed_lit[65]).code(fixed_lit[s]).bytes() + bytes(8), BAD_STREAM)
    for d in (30, 31):
        w = BitWriter().bits(0, 1).bits(1, 2).code(fixed_lit[65]).code(fixed_lit[65]).code(fixed_lit[65]).code(fixed_lit[257]).code((d, 5))
        out[f"distance_symbol_{d}"] = (w.bytes() + bytes(8), BAD_STREAM)
    lits = flat_lengths([65, 256, 257])
    w = dynamic_header(BitWriter(), lits, {}, ndist=1)
    lit = canonical([lits.get(s, 0) for s in range(286)])
    out["distance_without_a_code"] = (w.code(lit[65]).code(lit[65]).code(lit[65]).code(lit[257]).bytes() + bytes(8), BAD_STREAM)
    w = dynamic_header(BitWriter(), lits, {2: 1})                           # one distance code of length one: the word 0; 1 is no code
    out["bits_that_are_no_code"] = (w.code(lit[65]).code(lit[65]).code(lit[65]).code(lit[257]).bits(0xFFFF, 16).bytes() + bytes(8), BAD_STREAM)
    out["needs_history_first_token"] = (fixed_block(BitWriter(), [(3, 1)]).bytes() + bytes(8), NEEDS_HISTORY)
    out["needs_history_one_short"] = (fixed_block(BitWriter(), [1, 2, 3, (4, 4)]).bytes() + bytes(8), NEEDS_HISTORY)
    return out


def sync_flush_stream(parts, level=6):
    """One compressor, a Z_SYNC_FLUSH behind every part but the last, Z_FINISH at the end: the window is kept, so a later unit
    may refer back into an earlier one."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    out = b""
    for i, part in enumerate(parts):
        out += c.compress(part) + (c.flush(zlib.Z_SYNC_FLUSH) if i + 1 < len(parts) else c.flush(zlib.Z_FINISH))
    return out


def gzip_member(raw_stream, data, header=None):
    from infercnv_amd import rds
    return (rds.GZIP_HEADER if header is None else header) + raw_stream + struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)


def assembled_file(payloads, piece=256, level=1, host_parts=None):
    """(gzip file, inflated bytes) put together as rds.GzipAssembler does: host bytes through one zlib stream with a
    Z_FULL_FLUSH ahead of every payload, every payload as independent pieces (deflate_restate.host_pieces)."""
    from infercnv_amd import rds
    raw = io.BytesIO()
    gz = rds.GzipAssembler(raw)
    host_parts = host_parts or [b"header bytes " * 7] + [b" between " * (i + 2) for i in range(len(payloads))]
    plain = b""
    for i, payload in enumerate(payloads):
        gz.write(host_parts[i])
        plain += host_parts[i]
        out = gz.begin_payload()
        ps = dr.host_pieces(payload, piece, level)
        for comp, _, _ in ps:
            out.write(comp)
        gz.add_pieces(np.array([p[1] for p in ps], dtype=np.uint32), piece, len(payload), sum(len(p[0]) for p in ps))
        plain += payload
    gz.write(host_parts[len(payloads)])
    plain += host_parts[len(payloads)]
    gz.close()
    return raw.getvalue(), plain


def gzipfile_bytes(data, name="object.rds"):
    buf = io.BytesIO()
    with gzip.GzipFile(filename=name, fileobj=buf, mode="wb", mtime=0) as f:
        f.write(data)
    return buf.getvalue()


# ================================================================================================================ the host stand-in
class HostInflate:
    """rds._DeviceInflate on numpy arrays: the four device calls through the reader above, and a count of what was launched."""

    def __init__(self):
        self.calls = {"scan": 0, "measure": 0, "units": 0, "crc": 0}
        self.measured = None

    def upload(self, view):
        return bytes(view)

    def scan(self, src):
        self.calls["scan"] += 1
        return np.array(candidates(src), dtype=np.int64)

    def measure(self, src, start, max_in):
        self.calls["measure"] += 1
        got = [unit(src, int(s), int(max_in)) for s in start]
        self.measured = (np.asarray(start), got)
        return (np.array([g[1] for g in got], dtype=np.int64), np.array([g[2] for g in got], dtype=np.int64),
                np.array([g[0] for g in got], dtype=np.int32))

    def alloc(self, src, nbytes):
        return np.full(nbytes, 0xA5, dtype=np.uint8)

    def units(self, src, start, end, out_off, out_len, out):
        self.calls["units"] += 1
        status = np.empty(len(start), dtype=np.int32)
        for i, (s, e, o, n) in enumerate(zip(start.tolist(), end.tolist(), out_off.tolist(), out_len.tolist())):
            st, got_end, got_n, data = unit(src, s, e - s)
            if (st in (OK_MARKER, OK_FINAL) and (got_end != e or got_n != n)) or st == TOO_LONG:
                st = BAD_STREAM
            if st in (OK_MARKER, OK_FINAL):
                out[o:o + n] = np.frombuffer(data, dtype=np.uint8)
            status[i] = st
        return status

    def crc32_pieces(self, out, piece_bytes):
        self.calls["crc"] += 1
        b = out.tobytes()
        return np.array([zlib.crc32(b[o:o + piece_bytes]) for o in range(0, len(b), piece_bytes)], dtype=np.uint32)

    def stream(self, out):
        from infercnv_amd import rds
        return rds._DeviceStream(lambda lo, hi: out[lo:hi].tobytes(), out.size)


