"""Helpers of the K30 tests (tests/test_gunzip_host.py, tests/test_gpu_gunzip.py): the contract of include/icnv.h "INFLATE with
unknown history" restated sequentially on inflate_restate's RFC 1951 reader and writers -- the candidates of a raw stream, one
unit's (status, end bit, symbols), the tails and the resolve pass -- the streams of the tests, and the device calls restated on
the host for the tests of gunzip.gunzip's chain walk."""
from __future__ import annotations

import functools
import os
import struct
import zlib

import numpy as np

import deflate_restate as dr
import inflate_restate as ir

OK_BOUNDARY, OK_FINAL, TRUNCATED, TOO_LONG, BAD_STREAM = range(5)
W = 32768
MARK = 0x8000
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def reader_at(src, bit, limit):
    r = ir._Reader(src, bit >> 3, limit)
    if bit & 7:
        r.take(bit & 7)
    return r


def bit_pos(r):
    return r.p * 8 - r.bc


# ================================================================================================================ the candidates
def is_candidate(src, bit):
    """BFINAL 0, BTYPE 10 and a dynamic header the reader accepts, entirely inside src."""
    try:
        r = reader_at(src, bit, len(src))
        if r.take(3) != 4:
            return False
        ir._dynamic(r)
        return True
    except (ir._Dry, ir._Bad):
        return False


def candidates(raw):
    """Every candidate bit offset of raw, ascending.  The cheap tests (3 header bits, HLIT, HDIST, the code-length code's Kraft
    sum) are taken over all offsets at once; the reader parses the survivors."""
    raw = bytes(raw)
    n = len(raw)
    if n < 3:
        return []
    bits = np.unpackbits(np.frombuffer(raw + bytes(16), dtype=np.uint8), bitorder="little").astype(np.int64)
    b = np.arange(n * 8)
    field = lambda at, k: sum(bits[b + at + i] << i for i in range(k))
    keep = (field(0, 3) == 4) & (field(3, 5) <= 29) & (field(8, 5) <= 29)
    b = b[keep]
    ncode = field(13, 4) + 4
    kraft = np.zeros(b.size, dtype=np.int64)
    for i in range(19):
        l = field(17 + 3 * i, 3)
        kraft += np.where((i < ncode) & (l > 0), 128 >> l, 0)
    b = b[kraft == 128]
    return [int(x) for x in b if is_candidate(raw, int(x))]


# ================================================================================================================ one unit
def unit(raw, start_bit=0, stops=(), max_in=None):
    """(status, end_bit, symbols) of the unit that starts at bit start_bit of raw and stops ahead of a block header (not its
    first) on an offset in `stops`, or behind BFINAL.  symbols: a list of ints below 256 (bytes) and MARK | w (markers).  With
    a status other than OK_*, end_bit is start_bit."""
    n = len(raw)
    first = start_bit >> 3
    limit = n if max_in is None or max_in >= n - first else first + max_in
    dry = TOO_LONG if limit < n else TRUNCATED
    stops = stops if isinstance(stops, (set, frozenset)) else frozenset(int(s) for s in stops)
    out = []
    try:
        r = reader_at(raw, start_bit, limit)
        blocks = 0
        while True:
            if blocks and bit_pos(r) in stops:
                return OK_BOUNDARY, bit_pos(r), out
            blocks += 1
            last, kind = r.take(1), r.take(2)
            if kind == 3:
                raise ir._Bad()
            if kind == 0:
                q = r.byte_pos()
                r.bb, r.bc, r.p = 0, 0, q
                if q + 4 > limit:
                    raise ir._Dry()
                ln, nln = struct.unpack_from("<HH", raw, q)
                if ln ^ 0xFFFF != nln:
                    raise ir._Bad()
                r.p = q + 4
                if r.p + ln > limit:
                    raise ir._Dry()
                out += raw[r.p:r.p + ln]
                r.p += ln
            else:
                lit, dist = (ir.FIXED_LIT, ir.FIXED_DIST) if kind == 1 else ir._dynamic(r)
                while True:
                    s = r.symbol(lit)
                    if s < 256:
                        out.append(s)
                        continue
                    if s == 256:
                        break
                    if s >= 286:
                        raise ir._Bad()
                    ln = ir.LEN_BASE[s - 257] + r.take(ir.LEN_EXTRA[s - 257])
                    if dist.used == 0:
                        raise ir._Bad()
                    d = r.symbol(dist)
                    if d >= 30:
                        raise ir._Bad()
                    d = ir.DIST_BASE[d] + r.take(ir.DIST_EXTRA[d])
                    q = len(out)
                    if d > q + W:
                        raise ir._Bad()
                    for k in range(ln):                             # one by one: an overlapping match repeats what it wrote
                        at = q + k - d
                        out.append(out[at] if at >= 0 else MARK | (W + at))
            if last:
                return OK_FINAL, (bit_pos(r) + 7) // 8 * 8, out
    except ir._Dry:
        return dry, start_bit, out
    except ir._Bad:
        return BAD_STREAM, start_bit, out


def starts_of(cand):
    return [0] + [c for c in cand if c > 0]


def chain(raw, cand=None, max_in=None):
    """[(start_bit, status, end_bit, symbols)] of the units from bit 0 on, each begun where the one before ended."""
    cand = candidates(raw) if cand is None else cand
    stops, out, at = frozenset(cand), [], 0
    while True:
        st, end, sym = unit(raw, at, stops, max_in)
        out.append((at, st, end, sym))
        if st != OK_BOUNDARY:
            return out
        at = end


# ================================================================================================================ tails, resolve
def _one(v, out, off):
    """The byte of symbol v of a unit placed at off, or None: a marker in front of byte 0."""
    if v < 256:
        return v
    at = off - W + (v & 0x7FFF)
    return None if at < 0 else int(out[at])


def tails(sym, out_off, out_len, out):
    """The last min(W, out_len[i]) symbols of every unit, in order, into the uint8 array out.  Returns (bad, markers)."""
    bad, markers = 0, 0
    for off, ln in zip(out_off, out_len):
        off, ln = int(off), int(ln)
        t0 = off + ln - min(W, ln)
        got = [_one(int(v), out, off) for v in sym[t0:off + ln]]   # (a unit's tail reads only what lies in front of the unit)
        for j, (v, byte) in enumerate(zip(sym[t0:off + ln], got)):
            markers += int(v) >= 256
            if byte is None:
                bad = 1
            else:
                out[t0 + j] = byte
    return bad, markers


def resolve(sym, out_off, out_len, out):
    """Everything in front of the tails into out.  Returns bad."""
    bad = 0
    for off, ln in zip(out_off, out_len):
        off, ln = int(off), int(ln)
        for j in range(off, off + ln - min(W, ln)):
            byte = _one(int(sym[j]), out, off)
            if byte is None:
                bad = 1
            else:
                out[j] = byte
    return bad


def inflate(raw, max_in=None):
    """The whole scheme on the host: (bytes or None, chain units, candidates)."""
    cand = candidates(raw)
    units = chain(raw, cand, max_in)
    if units[-1][1] != OK_FINAL:
        return None, units, cand
    lens = np.array([len(u[3]) for u in units], dtype=np.int64)
    offs = np.cumsum(lens) - lens
    sym = np.array([v for u in units for v in u[3]], dtype=np.uint16)
    out = np.zeros(int(lens.sum()), dtype=np.uint8)
    bad, _ = tails(sym, offs, lens, out)
    bad |= resolve(sym, offs, lens, out)
    return (None if bad else out.tobytes()), units, cand


# ================================================================================================================ the streams
def poisson_tsv(n_bytes, seed):
    rng = np.random.default_rng(seed)
    rows = []
    while sum(len(r) + 1 for r in rows) < n_bytes:
        rows.append("\t".join([f"gene{len(rows)}"] + [str(int(x)) for x in rng.poisson(1.3, 40)]))
    return ("\n".join(rows) + "\n").encode()[:n_bytes]


def mixed(seed=41):
    rng = np.random.default_rng(seed)
    text = b"".join(b"the quick brown fox %d jumps over the lazy dog\n" % int(x) for x in rng.integers(0, 10 ** 6, 500))
    return text + dr.random_bytes(20000, seed + 1) + dr.denoised_like(900, seed + 2) + dr.count_like(2500, seed + 3) + text[:9000]


def raw_deflate(data, level=6, mem_level=8):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level)
    return c.compress(data) + c.flush()


@functools.lru_cache(maxsize=None)
def zlib_streams():
    """name -> (raw stream, data): the tab-separated counts and the mix at memLevel 1, 2, 3, 8 (level 6) and levels 1 and 9."""
    out = {}
    for name, data in (("counts", poisson_tsv(48000, 40)), ("mix", mixed())):
        for mem in (1, 2, 3, 8):
            out[f"{name}_mem{mem}"] = (raw_deflate(data, 6, mem), data)
        for level in (1, 9):
            out[f"{name}_level{level}_mem1"] = (raw_deflate(data, level, 1), data)
    return out


def gz_member(raw, data):
    """A gzip file around a raw stream: a plain header, the stream, CRC-32 and ISIZE."""
    return b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + raw + struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)


def gz_raw(file_bytes):
    """The raw stream of a one-member gzip file."""
    from infercnv_amd import rds
    return bytes(file_bytes[rds.gzip_header_length(file_bytes):len(file_bytes) - 8])


def golden_counts_gz():
    with open(os.path.join(GOLDEN, "create_object_example", "counts_every_8th_gene.matrix.gz"), "rb") as f:
        return f.read()


def hand_streams():
    """name -> (raw stream, expected bytes or None (the `bad` flag), tokens per block): hand-built streams of two or more
    dynamic blocks, so that every block but the first starts a unit.  The second unit's tokens reach into the window."""
    rng = np.random.default_rng(30)
    out = {}

    def build(name, blocks, kinds=None, expect_bad=False, closing=()):
        """Every listed block is written without BFINAL (a dynamic one is a candidate); a final fixed block of the `closing`
        tokens ends the stream, decoded by the unit that runs into it."""
        w = ir.BitWriter()
        for i, toks in enumerate(blocks):
            kind = (kinds or {}).get(i, "dynamic")
            if kind == "dynamic":
                ir.dynamic_block(w, toks)
            elif kind == "fixed":
                ir.fixed_block(w, toks)
            else:
                ir.stored_block(w, bytes(toks))
        ir.fixed_block(w, list(closing), final=True)
        blocks = list(blocks) + [list(closing)]
        data = None if expect_bad else ir.apply_tokens([t for b in blocks for t in b])
        out[name] = (w.bytes(), data, blocks)

    first = [int(x) for x in rng.integers(0, 256, 300)]
    build("first_token_match_marker_w_minus_1", [first, [(3, 1), 65, 66]])
    long_first = [int(x) for x in rng.integers(0, 256, 64)] + [(258, 64)] * 126 + [(196, 64)]      # exactly W bytes
    build("distance_q_plus_w_marker_0", [long_first, [(5, W), 1, 2]])
    build("match_from_window_into_own_bytes", [first, [10, 11, 12, (40, 20)]])
    build("match_copies_markers", [first, [(6, 100), 7, (6, 7), (4, 3)]])
    build("overlap_over_markers", [first, [(2 + 1, 2), (9, 2), (30, 3)]])
    for ln in (7, 8, 258):
        build(f"length_{ln}_over_markers", [first, [(ln, 200), (ln, ln), (ln, 3)]])
    build("empty_fixed_unit_between", [first, [], [(4, 9), 5]], kinds={1: "fixed"})
    # an empty fixed block is no candidate: the unit in front of it runs through it.  An empty DYNAMIC block makes a unit of 0 bytes
    build("unit_of_zero_bytes", [first, [], [(4, 9), 5]])
    build("unit_of_exactly_w", [first, long_first, [(9, W), (3, 1)]])
    build("unit_of_w_plus_1", [first, long_first + [77], [(9, W), (3, 1)]])
    for pad in range(8):                                                    # 9-bit literals: BFINAL's block ends at every bit residue
        build(f"final_after_{pad}_nine_bit_literals", [first, [(3, 5), 6]], closing=[200] * pad)
    build("through_fixed_and_stored", [first, [(5, 17), 3], [(6, 2), 9], list(b"stored bytes"), [(12, 12), (8, 30)]], kinds={2: "fixed", 3: "stored"})
    build("marker_in_first_unit", [[(3, 1), 65], [66, (3, 2)]], expect_bad=True)
    build("marker_in_front_of_byte_0", [[1, 2, 3], [(3, 4), 65]], expect_bad=True)
    return out


def planted_header():
    """(raw stream, data): a stored block whose data holds a valid dynamic header at a byte boundary -- a false candidate."""
    fake = ir.dynamic_block(ir.BitWriter(), [1, 2, 3, (3, 3)]).bytes()
    assert fake[0] & 7 == 4
    a = [int(x) for x in np.random.default_rng(3).integers(0, 256, 200)]
    stored = b"padding " * 5 + fake + b" more padding" * 3
    w = ir.dynamic_block(ir.BitWriter(), a)
    ir.stored_block(w, stored)
    b = [(20, 40), 7, 8, (9, 300)]
    ir.fixed_block(ir.dynamic_block(w, b), [9, 9], final=True)
    return w.bytes(), ir.apply_tokens(a + list(stored) + b + [9, 9])


# ================================================================================================================ the host stand-in
class HostGunzip:
    """gunzip._DeviceGunzip on numpy arrays: the five device calls through the restatement, and a count of what was launched."""

    def __init__(self, free=1 << 40):
        self.calls = {"find": 0, "measure": 0, "symbols": 0, "tails": 0, "resolve": 0, "crc": 0}
        self.free = free

    def available(self):
        return True

    def free_bytes(self):
        return self.free

    def upload(self, view):
        return bytes(view)

    def find(self, src):
        self.calls["find"] += 1
        return np.array(candidates(src), dtype=np.int64)

    def measure(self, src, cand, start, max_in):
        self.calls["measure"] += 1
        stops = frozenset(int(c) for c in cand)
        got = [unit(src, int(s), stops, int(max_in)) for s in start]
        return (np.array([g[1] for g in got], dtype=np.int64), np.array([len(g[2]) for g in got], dtype=np.int64),
                np.array([g[0] for g in got], dtype=np.int32))

    def symbols(self, src, cand, start, end, out_off, out_len, total):
        self.calls["symbols"] += 1
        stops = frozenset(int(c) for c in cand)
        sym = np.full(total, 0xA5A5, dtype=np.uint16)
        status = np.empty(len(start), dtype=np.int32)
        for i, (s, e, o, n) in enumerate(zip(start.tolist(), end.tolist(), out_off.tolist(), out_len.tolist())):
            st, got_end, got = unit(src, s, stops, (e + 7) // 8 - (s >> 3))
            if (st <= OK_FINAL and (got_end != e or len(got) != n)) or st == TOO_LONG:
                st = BAD_STREAM
            if st <= OK_FINAL:
                sym[o:o + n] = got
            status[i] = st
        return sym, status

    def tails(self, sym, out_off, out_len, total):
        self.calls["tails"] += 1
        out = np.full(total, 0xA5, dtype=np.uint8)
        bad, markers = tails(sym, out_off, out_len, out)
        return out, bad, markers

    def resolve(self, sym, out_off, out_len, out):
        self.calls["resolve"] += 1
        return resolve(sym, out_off, out_len, out)

    def crc32_pieces(self, out, piece_bytes):
        self.calls["crc"] += 1
        b = out.tobytes()
        return np.array([zlib.crc32(b[o:o + piece_bytes]) for o in range(0, len(b), piece_bytes)], dtype=np.uint32)

    def stream(self, out):
        from infercnv_amd import rds
        return rds._DeviceStream(lambda lo, hi: out[lo:hi].tobytes(), out.size)
