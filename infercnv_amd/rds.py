"""R's serialisation format: `.rds` files of infercnv objects for R, and R's own read back (DESIGN K27).

R's `add_to_seurat`, `plot_cnv`, `apply_median_filtering` and `plot_per_group` start from an `infercnv` S4 object read with
readRDS.  This module writes such a file from an InfercnvObject (save_infercnv_obj), reads one written by either side
(load_infercnv_obj), and holds the general writer and parser they stand on (write_rds, read_rds), and the walk that finds a
count matrix's payloads in a file for device.read_rds_counts (locate_counts, DESIGN K34).  The byte swap and the
transpose of the matrices run on the device (icnv_xdr_encode_dev / icnv_xdr_decode_dev, include/icnv.h); everything else
-- the format below -- is written and parsed here.  No R exists where this was built: readRDS has never opened one of
these files.  What was checked instead is in tests/test_rds_host.py: literal bytes derived by hand from the format, the
structure of an R-written infercnv object as a skeleton that our file must reproduce, and R's own file read back.

The format (R Internals, "Serialization Formats"), as written here
------------------------------------------------------------------
XDR, version 3, uncompressed unless compress=True -- what saveRDS(compress = FALSE) writes; readRDS detects it.  With
compress=True the same stream inside one gzip member, as saveRDS writes by default: put together by GzipAssembler from
pieces compressed on the device where that route exists (DESIGN K28), by Python's GzipFile otherwise.  Such a file is read
back on the device too (inflate_gzip, DESIGN K29: its flush points make it a chain of independently inflatable units); any
other gzip file -- R's, GzipFile's -- through the host's inflate.

  header   `X\\n`, int32 3, int32 writer version (0x00040000: R 4.0.0), int32 min-reader 0x00030500 (R 3.5.0),
           int32 5, `UTF-8`.  All integers big-endian.
  item     an int32 flag word = type | obj << 8 | has_attr << 9 | has_tag << 10 | gp << 12, then the payload, then -- for
           vectors and S4 objects with has_attr -- the attribute pairlist.
  types    NILVALUE 254 (flag word 0x000000FE, no payload); SYMSXP 1 (one CHARSXP); LISTSXP 2 (attribute pairlists: every
           node 0x00000402 = tagged, then the tag, the value, and the next node; closed by NILVALUE); CHARSXP 9 (int32 byte
           count, bytes); LGLSXP 10, INTSXP 13 (length, int32 each); REALSXP 14 (length, IEEE double each); STRSXP 16
           (length, CHARSXPs); VECSXP 19 (length, items); S4SXP 25 (nothing but its attributes: the slots).
  CHARSXP  gp 64 (ASCII) for pure-ASCII strings: 0x00040009; gp 8 (UTF-8) otherwise: 0x00008009.  NA_character_ is
           0x00000009 with length -1.
  symbols  the first occurrence of a symbol is written in full (0x00000001 + CHARSXP) and numbered from 1 in order of
           appearance; every later one is a REFSXP, the single word (index << 8) | 255.  This is what R does.
  lengths  int32; above 2^31 - 1 the long-vector form: -1, high word, low word (a 10 000 x 250 000 matrix needs it).
  S4       0x00010319: type 25, the object bit, the attribute bit, gp 0x10 (the S4 bit).  The slots are the attributes in
           order, the `class` attribute last: a STRSXP that itself carries the attribute `package` (0x00000210).  A slot
           that is NULL is stored as the symbol `\\001NULL\\001`.
  others   a factor is an INTSXP with the object bit (0x0000030D) and the attributes `levels`, `class`; a data.frame a
           VECSXP with the object bit (0x00000313) and `names`, `row.names`, `class`; a matrix a vector with `dim`,
           `dimnames`; an hclust a VECSXP with the object bit and `names`, `class`.
Every flag word above was confirmed against the bytes of the R-written data/infercnv_object_example.rda of the reference.

Worked example, c(1L, NA):
  58 0A | 00000003 | 00040000 | 00030500 | 00000005 "UTF-8" | 0000000D | 00000002 | 00000001 | 80000000

A NaN's payload is never touched: NA_real_ (0x7FF00000000007A2) survives both directions bit for bit.

The value model
---------------
  None                       NULL
  bool / int / float / str   a vector of length one (LGLSXP, INTSXP, REALSXP, STRSXP)
  numpy array, 1-D           bool -> LGLSXP, integers -> INTSXP (int32; INT_MIN is NA_integer_), floats -> REALSXP, str or
                             object (None is NA_character_) -> STRSXP
  numpy array, 2-D           the rows x cols matrix: the vector of its columns with `dim`
  list / tuple               VECSXP
  dict                       VECSXP with `names`
  RValue(value, attrs)       any of the above with further attributes, in order (`dim` and a dict's `names` are implied
                             and come first)
  RFactor(codes, levels)     0-based codes, -1 is NA
  RS4(cls, package, slots)   an S4 object; a slot None is R's NULL slot
  RDeviceMatrix(t)           a CUDA (cols, rows) float64 / int32 tensor with contiguous rows: R's rows x cols matrix, encoded
                             from where it lives.  A 1-D CUDA tensor is a vector.
read_rds returns the same model: vectors always as numpy arrays (a length-one vector is an array of one), a VECSXP whose only
attribute is a complete set of distinct `names` as a dict.  LANGSXP -- the `call` of an hclust -- is stepped over and
surfaces as RLang(); a symbol as RSymbol(name).

The infercnv object, as R stores it (slot order of the R-written file): expr.data, count.data, gene_order,
reference_grouped_cell_indices, observation_grouped_cell_indices, tumor_subclusters, options, .hspike, class.
  expr.data, count.data   matrices with dim and dimnames (genes, cells); integer dtypes as INTSXP; a scipy sparse matrix as
                          a dgCMatrix (S4 of package Matrix: i, p, Dim, Dimnames, x, factors)
  gene_order              data.frame: chr a factor with levels in order of first appearance, start and stop integer when
                          every value is integral (else double), row.names the gene names
  the group lists         named lists of 1-based integer vectors
  tumor_subclusters       list(hc = ..., subclusters = ...): every subcluster vector a NAMED integer vector (names: its
                          cells' names -- add_to_seurat indexes by them); every HClust a list of class hclust with R's seven
                          names merge, height, order, labels, method, call, dist.method.  `call` is written as NULL: the
                          mirror does not keep R's call, and nothing in the reference reads it.  A Leiden group's list of
                          partition trees is a list, NULL where the mirror holds None.
  options                 a named list: None -> NULL, str / bool / int / float scalars, a list of scalars of one kind as the
                          vector c() makes of them (a vector of R's comes back as a list, one of length one as a scalar),
                          other lists as lists
  .hspike                 a nested object or NULL
Indices are 0-based in the mirror and 1-based in the file.
"""
from __future__ import annotations

import bz2
import gzip
import lzma
import mmap
import os
import struct
import time
import zlib
from dataclasses import dataclass, field

import numpy as np

from .infercnv_object import DeviceMatrix, GeneOrder, InfercnvObject

WRITER_VERSION = 0x00040000
MIN_READER_VERSION = 0x00030500
NILVALUE, REFSXP, ALTREP_SXP = 254, 255, 238
SYMSXP, LISTSXP, LANGSXP, CHARSXP, LGLSXP, INTSXP, REALSXP, STRSXP, VECSXP, S4SXP = 1, 2, 6, 9, 10, 13, 14, 16, 19, 25
OBJ_BIT, ATTR_BIT, TAG_BIT = 1 << 8, 1 << 9, 1 << 10
GP_S4, GP_UTF8, GP_LATIN1, GP_BYTES, GP_ASCII = 1 << 4, 1 << 3, 1 << 2, 1 << 1, 1 << 6
NA_INTEGER = -2 ** 31
NULL_SLOT = "\x01NULL\x01"          # the symbol R stores in a slot that is NULL

DEVICE_THRESHOLD = 1 << 20          # bytes: numeric payloads at or above this are encoded / decoded on the device
CHUNK_BYTES = 64 << 20              # capacity of one streamed chunk


@dataclass
class RValue:
    value: object
    attrs: dict = field(default_factory=dict)


@dataclass
class RFactor:
    codes: np.ndarray
    levels: list
    attrs: dict = field(default_factory=dict)      # attributes beyond levels and class


@dataclass
class RS4:
    cls: str
    package: str
    slots: dict


@dataclass
class RSymbol:
    name: str


@dataclass
class RLang:
    """A language object (LANGSXP) that was stepped over; its content is not kept."""


class RDeviceMatrix:
    """A CUDA (cols, rows) tensor with contiguous rows standing for R's rows x cols matrix."""

    def __init__(self, tensor):
        self.tensor = tensor


# ================================================================================================================ writing
def length_words(n: int) -> bytes:
    """The length field of a vector of n elements."""
    n = int(n)
    if n < 0:
        raise ValueError("negative length")
    if n <= 0x7FFFFFFF:
        return struct.pack(">i", n)
    return struct.pack(">iII", -1, n >> 32, n & 0xFFFFFFFF)


def _is_cuda(v):
    return type(v).__module__.startswith("torch") and hasattr(v, "is_cuda") and v.is_cuda


def _scalar_kind(v):
    if isinstance(v, (bool, np.bool_)):
        return "b"
    if isinstance(v, (int, np.integer)):
        return "i"
    if isinstance(v, (float, np.floating)):
        return "f"
    if isinstance(v, str):
        return "s"
    return None


class _Writer:
    def __init__(self, f, device):
        self.f, self.device = f, device
        self.buf = bytearray()
        self.symbols = {}
        self.stats = []                 # stream_chunks' dicts, one per payload that went through the device

    # ---- bytes
    def flush(self):
        if self.buf:
            self.f.write(bytes(self.buf))
            self.buf.clear()

    def put(self, b):
        self.buf += b
        if len(self.buf) >= 1 << 20:
            self.flush()

    def word(self, v):
        self.put(struct.pack(">I", v & 0xFFFFFFFF))

    # ---- items
    def charsxp(self, s):
        if s is None:
            self.put(struct.pack(">Ii", CHARSXP, -1))
            return
        b = str(s).encode("utf-8")
        self.put(struct.pack(">Ii", CHARSXP | ((GP_ASCII if b.isascii() else GP_UTF8) << 12), len(b)) + b)

    def symbol(self, name):
        idx = self.symbols.get(name)
        if idx is not None:
            self.word((idx << 8) | REFSXP)
            return
        self.symbols[name] = len(self.symbols) + 1
        self.word(SYMSXP)
        self.charsxp(name)

    def attributes(self, attrs):
        for name, value in attrs.items():
            self.word(LISTSXP | TAG_BIT)
            self.symbol(name)
            self.item(value)
        self.word(NILVALUE)

    def strings(self, values, flags=0):
        self.word(STRSXP | flags)
        n = len(values)
        self.put(length_words(n))
        if n >= 256 and all(s is not None for s in values) and "".join(values).isascii():
            # gene and cell names by the ten thousand: all records at once -- 0x00040009, the length, the bytes
            body = np.frombuffer("".join(values).encode("ascii"), dtype=np.uint8)
            lens = np.fromiter(map(len, values), dtype=np.int64, count=n)
            starts = np.cumsum(lens + 8) - (lens + 8)
            head = np.empty((n, 8), dtype=np.uint8)
            head[:, :4] = np.frombuffer(struct.pack(">I", CHARSXP | (GP_ASCII << 12)), dtype=np.uint8)
            head[:, 4:] = lens.astype(">i4").view(np.uint8).reshape(n, 4)
            at = (starts[:, None] + np.arange(8)).ravel()
            out = np.empty(body.size + 8 * n, dtype=np.uint8)
            is_body = np.ones(out.size, dtype=bool)
            is_body[at] = False
            out[at] = head.ravel()
            out[is_body] = body
            self.put(out.tobytes())
            return
        for s in values:
            self.charsxp(s)

    def item(self, v, attrs=None, obj=False):
        """One item; attrs: the attributes to hang on it (in order), obj: the object bit."""
        attrs = dict(attrs or {})
        flags = (OBJ_BIT if obj or "class" in attrs else 0)
        if isinstance(v, RValue):
            return self.item(v.value, {**v.attrs, **attrs}, obj)
        if isinstance(v, RS4):
            self.word(S4SXP | OBJ_BIT | ATTR_BIT | (GP_S4 << 12))
            slots = {k: (RSymbol(NULL_SLOT) if s is None else s) for k, s in v.slots.items()}
            slots["class"] = RValue(np.array([v.cls]), {"package": v.package})
            return self.attributes(slots)
        if isinstance(v, RSymbol):
            return self.symbol(v.name)
        if v is None:
            if attrs:
                raise ValueError("NULL cannot carry attributes")
            return self.word(NILVALUE)
        if isinstance(v, RFactor):
            codes = np.asarray(v.codes, dtype=np.int64)
            ints = np.where(codes < 0, NA_INTEGER, codes + 1).astype(np.int32)
            return self.item(ints, {"levels": np.array(list(v.levels), dtype=object), "class": "factor", **v.attrs, **attrs})
        if isinstance(v, dict):
            attrs = {"names": np.array([str(k) for k in v], dtype=object), **attrs}
            v = list(v.values())
        kind = _scalar_kind(v)
        if kind is not None:
            v = np.array([v], dtype={"b": np.bool_, "i": np.int64, "f": np.float64, "s": object}[kind])
        flags |= ATTR_BIT if attrs or isinstance(v, RDeviceMatrix) or getattr(v, "ndim", 1) == 2 else 0
        if isinstance(v, (list, tuple)):
            self.word(VECSXP | flags)
            self.put(length_words(len(v)))
            for e in v:
                self.item(e)
        elif isinstance(v, RDeviceMatrix):
            t = v.tensor
            attrs = {"dim": np.array([t.shape[1], t.shape[0]], dtype=np.int32), **attrs}
            self.numeric(t, flags)
        elif _is_cuda(v):
            if v.dim() != 1:
                raise ValueError("a CUDA matrix is written as RDeviceMatrix(tensor of shape (cols, rows))")
            self.numeric(v, flags)
        elif isinstance(v, np.ndarray):
            if v.ndim == 2:
                attrs = {"dim": np.array(v.shape, dtype=np.int32), **attrs}
            elif v.ndim != 1:
                raise ValueError("arrays of one or two dimensions only")
            if v.dtype.kind in "USO":
                if v.ndim == 2:
                    v = v.T.ravel()
                self.strings([None if s is None else str(s) for s in v.tolist()], flags)
            else:
                self.numeric(v, flags)
        else:
            raise TypeError(f"cannot write a {type(v).__name__} as an R value")
        if attrs:
            self.attributes(attrs)

    # ---- numeric payloads
    def numeric(self, v, flags):
        """The flag word, the length and the big-endian elements of a host array (1-D, or 2-D rows x cols) or a CUDA tensor
        (1-D, or the (cols, rows) device matrix)."""
        cuda = _is_cuda(v)
        if cuda:
            import torch
            sexp, es = {torch.float64: (REALSXP, 8), torch.int32: (INTSXP, 4)}.get(v.dtype, (None, None))
            if sexp is None:
                raise TypeError("CUDA tensors are written from float64 or int32")
            n = int(v.numel())
        else:
            if v.dtype.kind == "b":
                sexp, v = LGLSXP, v.astype(np.int32)
            elif v.dtype.kind in "iu":
                if v.size and (int(v.min()) < NA_INTEGER or int(v.max()) > 0x7FFFFFFF):
                    raise ValueError("an integer beyond int32 has no INTSXP")
                sexp, v = INTSXP, v.astype(np.int32, copy=False)
            elif v.dtype.kind == "f":
                sexp, v = REALSXP, v.astype(np.float64, copy=False)
            else:
                raise TypeError(f"cannot write dtype {v.dtype}")
            es, n = v.dtype.itemsize, int(v.size)
        self.word(sexp | flags)
        self.put(length_words(n))
        if n == 0:
            return
        on_device = cuda or (self.device is not False and n * es >= DEVICE_THRESHOLD and _device_available())
        if not on_device:
            return self.host_payload(v)
        self.stats.append(_stream_payload(self, v, cuda, n, es))

    def host_payload(self, v):
        """The CPU-testable restatement of the device route: transpose, then swap."""
        self.flush()
        be = v.dtype.newbyteorder(">")
        if v.ndim == 1:
            self.f.write(v.astype(be).tobytes())
            return
        step = max(1, (CHUNK_BYTES // v.dtype.itemsize) // max(v.shape[0], 1))
        for c0 in range(0, v.shape[1], step):        # a block of columns at a time: R's order is column after column
            self.f.write(np.ascontiguousarray(v[:, c0:c0 + step].T).astype(be).tobytes())


def _device_available():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


def _deflate_enabled():
    """ICNV_DEFLATE=0 (environment, read per call): compress=True keeps Python's GzipFile even where a GPU is present."""
    return os.environ.get("ICNV_DEFLATE", "1").strip() != "0"


def _stream_payload(w, v, cuda, n, es):
    """The device route of one numeric payload of n elements of es bytes: v, a CUDA tensor or a host array that is uploaded, is
    encoded chunk by chunk and streamed to the file (text_stream.stream_chunks).  Under a GzipAssembler every chunk is
    compressed where it was encoded -- xdr_encode into a scratch, deflate_pieces, deflate_pack into the streamed buffer -- and
    the packed pieces go to the raw file.  Returns the payload's statistics."""
    import torch
    from . import device as dev, text_stream
    upload_s = 0.0
    if cuda:
        x, layout = v, "cols"
    else:                       # an uploaded host array: a vector as it is, a matrix in its own (rows, cols) layout
        target = w.device if w.device not in (None, True) else "cuda"
        t0 = time.perf_counter()
        x, layout = torch.from_numpy(np.ascontiguousarray(v)).to(target), ("rows" if v.ndim == 2 else "cols")
        torch.cuda.synchronize(x.device)
        upload_s = time.perf_counter() - t0
    w.flush()
    per_chunk = max(1, min(CHUNK_BYTES, -(-n * es // 16) * 16) // es)
    state = {"e": 0}
    gz = w.f if isinstance(w.f, GzipAssembler) else None
    if gz is None:
        def fill(buf):
            e0 = state["e"]
            if e0 >= n:
                return None
            e1 = min(n, e0 + per_chunk)
            dev.xdr_encode(x, layout=layout, e0=e0, e1=e1, out=buf)
            state["e"] = e1
            return (e1 - e0) * es

        return dict(text_stream.stream_chunks(w.f, per_chunk * es, x.device, fill), upload_s=upload_s)

    piece = dev.DEFLATE_PIECE
    max_pieces = -(-per_chunk * es // piece)
    with torch.cuda.device(x.device):
        scratch = torch.empty(per_chunk * es, dtype=torch.uint8, device=x.device)
        slots = torch.empty((max_pieces, dev.deflate_bound(piece)), dtype=torch.uint8, device=x.device)
    extra = {"raw_bytes": 0, "compressed_bytes": 0, "pieces": 0, "stored_pieces": 0, "deflate_s": 0.0}

    def fill(buf):
        e0 = state["e"]
        if e0 >= n:
            return None
        e1 = min(n, e0 + per_chunk)
        raw = dev.xdr_encode(x, layout=layout, e0=e0, e1=e1, out=scratch)
        t0 = time.perf_counter()
        dst, piece_len, piece_crc = dev.deflate_pieces(raw, piece, dst=slots)
        packed = dev.deflate_pack(dst, piece_len, out=buf)              # waits for the stream: the size comes back
        lens = piece_len.cpu().numpy()
        extra["deflate_s"] += time.perf_counter() - t0
        nbytes = (e1 - e0) * es
        gz.add_pieces(piece_crc.cpu().numpy(), piece, nbytes, int(packed.numel()))
        inputs = np.full(lens.size, piece, dtype=np.int64)
        inputs[-1] = nbytes - (lens.size - 1) * piece
        extra["raw_bytes"] += nbytes
        extra["compressed_bytes"] += int(packed.numel())
        extra["pieces"] += int(lens.size)
        extra["stored_pieces"] += int((lens == inputs + 5).sum())       # a Huffman-coded piece is smaller than that
        state["e"] = e1
        return int(packed.numel())

    stats = text_stream.stream_chunks(gz.begin_payload(), max_pieces * dev.deflate_bound(piece), x.device, fill)
    return dict(stats, upload_s=upload_s, **extra)


GZIP_HEADER = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff"      # deflate, no flags, mtime 0, no extra flags, OS unknown


class GzipAssembler:
    """One gzip member (RFC 1952) around ONE raw DEFLATE stream that two compressors write in turn: the small host-side
    parts go through zlib (level 6, raw), every device payload is the packed pieces of icnv_deflate_pieces_dev, written to
    the raw file by the caller between begin_payload() and add_pieces().  A Z_FULL_FLUSH ahead of every payload ends the host
    compressor's block on a byte boundary and empties its window, so it never refers back across bytes it did not see; the
    pieces end on byte boundaries and set no BFINAL; the host compressor's Z_FINISH ends the stream.  The trailer's CRC-32 is
    combined from the host segments' zlib.crc32 and the pieces' CRCs (device.crc32_combine): no host pass over a payload."""

    def __init__(self, raw):
        self.raw = raw
        self.z = zlib.compressobj(6, zlib.DEFLATED, -15)
        self.crc, self.size, self.compressed = 0, 0, 0
        self._raw(GZIP_HEADER)

    def _raw(self, b):
        if b:
            self.raw.write(b)
            self.compressed += len(b)

    def write(self, b):
        """Host bytes of the uncompressed stream."""
        self.crc = zlib.crc32(b, self.crc)
        self.size += len(b)
        self._raw(self.z.compress(b))
        return len(b)

    def begin_payload(self):
        """Ends the host compressor's part; returns the raw file, which the caller writes the packed pieces to."""
        self._raw(self.z.flush(zlib.Z_FULL_FLUSH))
        return self.raw

    def add_pieces(self, piece_crcs, piece_bytes, raw_bytes, compressed_bytes):
        """Accounts for pieces the caller wrote (or is writing) to the raw file: the CRC-32 of every piece's input, the
        common input length of all but the last, the input bytes and the compressed bytes in all."""
        from .device import crc32_combine, crc32_combine_pieces
        n = len(piece_crcs)
        if n == 0:
            return
        last = int(raw_bytes) - (n - 1) * int(piece_bytes)
        if not 0 < last <= piece_bytes:
            raise ValueError("the pieces do not add up to raw_bytes")
        self.crc = crc32_combine(self.crc, crc32_combine_pieces(piece_crcs, piece_bytes, last), raw_bytes)
        self.size += int(raw_bytes)
        self.compressed += int(compressed_bytes)

    def close(self):
        self._raw(self.z.flush(zlib.Z_FINISH))
        self._raw(struct.pack("<II", self.crc & 0xFFFFFFFF, self.size & 0xFFFFFFFF))


def write_rds(value, path, *, compress=False, device=None):
    """Writes `value` (module docstring: the value model) as an .rds file readRDS detects.  path: a file name or a binary
    file object.  Numeric arrays of at least DEVICE_THRESHOLD bytes are uploaded, encoded on the device in chunks of
    CHUNK_BYTES and streamed to the file (text_stream.stream_chunks); a CUDA tensor is encoded from where it lives; smaller
    arrays, and every array with device=False or without a GPU, are encoded with NumPy.  Both routes write the same bytes.
    compress=True writes a gzip file, what saveRDS does by default.  Where the device route exists (device is not False and a
    GPU is present) it is one gzip member with mtime 0 put together by GzipAssembler: the payloads that go through the device
    are compressed there in independent pieces (icnv_deflate_pieces_dev, DESIGN K28), everything else by zlib on the host,
    and the statistics of such a payload gain raw_bytes, compressed_bytes, pieces, stored_pieces and deflate_s.  With
    device=False, without a GPU or with ICNV_DEFLATE=0 in the environment the stream goes through Python's GzipFile on the
    host as before (tens of MB per second).  Either file inflates to the bytes compress=False writes.  Returns the stream
    statistics of the payloads that went through the device."""
    own = isinstance(path, (str, bytes)) or hasattr(path, "__fspath__")
    raw = open(path, "wb") if own else path
    if compress and device is not False and _deflate_enabled() and _device_available():
        f = GzipAssembler(raw)
    else:
        f = gzip.GzipFile(fileobj=raw, mode="wb") if compress else raw
    try:
        w = _Writer(f, device)
        w.put(b"X\n" + struct.pack(">iIIi", 3, WRITER_VERSION, MIN_READER_VERSION, 5) + b"UTF-8")
        w.item(value)
        w.flush()
    finally:
        if compress:
            f.close()
        if own:
            raw.close()
    return w.stats


# ================================================================================================================ reading
class _Reader:
    def __init__(self, buf, return_device=False, device_ok=True):
        self.buf, self.pos, self.n = buf, 0, len(buf)
        self.refs = []
        self.return_device = return_device and device_ok
        self.windowed = isinstance(buf, _DeviceStream)        # the stream lies on the device (inflate_gzip)

    def need(self, k):
        if k < 0 or self.pos + k > self.n:
            raise ValueError(f"truncated file: {k} bytes wanted at byte {self.pos}, {self.n - self.pos} left")

    def int(self):
        self.need(4)
        v = self.buf.int_at(self.pos) if self.windowed else struct.unpack_from(">i", self.buf, self.pos)[0]
        self.pos += 4
        return v

    def length(self):
        n = self.int()
        if n == -1:
            hi, lo = self.int(), self.int()
            n = ((hi & 0xFFFFFFFF) << 32) | (lo & 0xFFFFFFFF)
        if n < 0:
            raise ValueError(f"negative length at byte {self.pos - 4}")
        return n

    def take(self, k):
        self.need(k)
        b = self.buf[self.pos:self.pos + k]
        self.pos += k
        return b

    def header(self):
        container = None
        if self.buf[:5] in (b"RDX2\n", b"RDX3\n"):
            container, self.pos = "rda", 5
        fmt = bytes(self.take(2))
        if fmt != b"X\n":
            raise ValueError(f"only XDR serialisation is read, the file starts with {fmt!r}")
        version = self.int()
        self.int()
        self.int()
        if version == 3:
            self.take(self.int())
        elif version != 2:
            raise ValueError(f"unsupported serialisation version {version}")
        return container

    def attrs(self):
        a = self.item()
        if a is None:
            return {}
        if not isinstance(a, _Pairlist):
            raise ValueError(f"attributes are not a pairlist at byte {self.pos}")
        return a.as_dict()

    def pairlist(self, flags):
        """LISTSXP / LANGSXP nodes along the cdr, iteratively.  Returns a _Pairlist (tags, values, tail, first node's attrs)."""
        out = _Pairlist()
        while True:
            if flags & ATTR_BIT:
                a = self.attrs()
                if not out.tags:
                    out.attrs = a
            tag = self.item() if flags & TAG_BIT else None
            out.tags.append(tag.name if isinstance(tag, RSymbol) else None)
            out.values.append(self.item())
            at = self.pos
            nflags = self.int()
            if nflags & 0xFF in (LISTSXP, LANGSXP):
                flags = nflags
                continue
            self.pos = at
            out.tail = self.item()
            return out

    def item(self):
        at = self.pos
        flags = self.int()
        t = flags & 0xFF
        has_attr = bool(flags & ATTR_BIT)
        if t == NILVALUE:
            return None
        if t == REFSXP:
            idx = (flags >> 8) & 0xFFFFFF
            if idx == 0:
                idx = self.int()
            if not 1 <= idx <= len(self.refs):
                raise ValueError(f"reference {idx} at byte {at} names nothing read so far")
            return self.refs[idx - 1]
        if t == SYMSXP:
            name = self.item()
            sym = RSymbol(name)
            self.refs.append(sym)
            return sym
        if t == LISTSXP:
            return self.pairlist(flags)
        if t == LANGSXP:
            self.pairlist(flags)
            return RLang()
        if t == CHARSXP:
            n = self.int()
            if n == -1:
                return None
            b = bytes(self.take(n))
            gp = flags >> 12
            return b.decode("latin-1") if gp & GP_LATIN1 else b.decode("utf-8", errors="replace")
        if t in (LGLSXP, INTSXP, REALSXP):
            n = self.length()
            v = self.numeric(t, n)
            return self.finish(v, has_attr)
        if t == STRSXP:
            n = self.length()
            vals = [self.item() for _ in range(n)]
            return self.finish(_str_array(vals), has_attr)
        if t == VECSXP:
            n = self.length()
            vals = [self.item() for _ in range(n)]
            return self.finish(vals, has_attr)
        if t == S4SXP:
            slots = self.attrs() if has_attr else {}
            cls = slots.pop("class", None)
            package = ""
            if isinstance(cls, RValue):
                package = _scalar(cls.attrs.get("package"), "")
                cls = cls.value
            slots = {k: (None if isinstance(v, RSymbol) and v.name == NULL_SLOT else v) for k, v in slots.items()}
            return RS4(_scalar(cls, ""), package, slots)
        if t == ALTREP_SXP:
            return self.altrep(at)
        raise ValueError(f"unsupported SEXP type {t} at byte {at}")

    def numeric(self, t, n):
        es = 8 if t == REALSXP else 4
        self.need(n * es)
        pos = self.pos
        self.pos += n * es
        if self.return_device and t != LGLSXP and n * es >= DEVICE_THRESHOLD:
            if self.windowed and self.buf.tensor is not None:
                return _decode_device_stream(self.buf.tensor, pos, n, es)
            return _decode_on_device(self.buf[pos:pos + n * es] if self.windowed else self.buf, 0 if self.windowed else pos, n, es)
        if self.windowed:
            v = np.frombuffer(self.buf[pos:pos + n * es], dtype=">f8" if t == REALSXP else ">i4", count=n)
        else:
            v = np.frombuffer(self.buf, dtype=">f8" if t == REALSXP else ">i4", count=n, offset=pos)
        v = v.astype(v.dtype.newbyteorder("="))
        if t == LGLSXP:
            if (v == NA_INTEGER).any():
                out = np.array([None if x == NA_INTEGER else bool(x) for x in v.tolist()], dtype=object)
                return out
            return v != 0
        return v

    def finish(self, v, has_attr):
        attrs = self.attrs() if has_attr else {}
        if _is_cuda(v) and np.asarray(attrs.get("dim", ())).size != 2:
            v = v.cpu().numpy()                   # only a matrix stays on the device (its attributes follow its payload)
        return _with_attrs(v, attrs)

    def altrep_parts(self, cls):
        """The state and the attributes of an ALTREP object of class `cls`, whose info was just read."""
        return self.item(), self.item()

    def compact_seq(self, cls, seq):
        """What stands for the expanded sequence of a compact_intseq / compact_realseq."""
        return seq

    def altrep(self, at):
        info = self.item()
        cls = info.values[0].name if isinstance(info, _Pairlist) and info.values and isinstance(info.values[0], RSymbol) else None
        state, attr = self.altrep_parts(cls)
        attrs = attr.as_dict() if isinstance(attr, _Pairlist) else {}
        if cls in ("compact_intseq", "compact_realseq"):
            n, start, step = (float(x) for x in np.asarray(state)[:3])
            seq = start + step * np.arange(int(n), dtype=np.float64)
            return _with_attrs(self.compact_seq(cls, seq.astype(np.int32) if cls == "compact_intseq" else seq), attrs)
        if cls == "deferred_string":
            arg = state.values[0] if isinstance(state, _Pairlist) else state
            arg = arg.value if isinstance(arg, RValue) else arg
            arg = np.asarray(arg)
            if arg.dtype.kind in "iu":
                vals = [None if x == NA_INTEGER else str(x) for x in arg.tolist()]
            elif arg.dtype.kind == "f":
                vals = [None if x != x else ("%.15g" % x) for x in arg.tolist()]
            else:
                vals = arg.tolist()
            return _with_attrs(_str_array(vals), attrs)
        if cls in ("wrap_real", "wrap_integer", "wrap_logical", "wrap_string"):
            x = state[0] if isinstance(state, list) else state
            if isinstance(x, RValue) and not attrs:
                return x
            return _with_attrs(x.value if isinstance(x, RValue) else x, {**(x.attrs if isinstance(x, RValue) else {}), **attrs})
        raise ValueError(f"unsupported ALTREP class {cls!r} (SEXP type {ALTREP_SXP}) at byte {at}")


class _Pairlist:
    def __init__(self):
        self.tags, self.values, self.tail, self.attrs = [], [], None, {}

    def as_dict(self):
        return {(t if t is not None else f"__{i}"): v for i, (t, v) in enumerate(zip(self.tags, self.values))}


def _str_array(vals):
    if any(v is None for v in vals):
        return np.array(vals, dtype=object)
    return np.array(vals, dtype=str) if vals else np.array([], dtype=str)


def _scalar(v, default=None):
    if isinstance(v, RValue):
        v = v.value
    if v is None:
        return default
    a = np.asarray(v)
    return a.ravel()[0].item() if a.size else default


def _with_attrs(v, attrs):
    """The value model's form of a vector or list `v` with the attribute dict `attrs`."""
    attrs = dict(attrs)
    if not attrs:
        return v
    if isinstance(v, (RdsPayload, RNoPayload)):    # locate_counts: the vector was not decoded, it only carries its attributes
        return RValue(v, attrs)
    cls = attrs.get("class")
    cls_list = [] if cls is None else [str(c) for c in np.asarray(cls.value if isinstance(cls, RValue) else cls).ravel()]
    if isinstance(v, np.ndarray) and v.dtype.kind in "iu" and "factor" in cls_list and "levels" in attrs:
        levels = [None if s is None else str(s) for s in np.asarray(attrs.pop("levels")).tolist()]
        attrs.pop("class")
        codes = np.where(v == NA_INTEGER, -1, v.astype(np.int64) - 1)
        return RFactor(codes, levels, attrs)
    dim = attrs.get("dim")
    if dim is not None and not isinstance(v, list) and np.asarray(dim).size == 2:
        r, c = (int(x) for x in np.asarray(dim))
        attrs.pop("dim")
        if isinstance(v, np.ndarray):
            v = np.ascontiguousarray(v.reshape(c, r).T)
        else:                                     # decoded on the device: the stream's own order is (cols, rows)
            v = RDeviceMatrix(v.view(c, r))
    if isinstance(v, list) and "names" in attrs:
        names = np.asarray(attrs["names"]).tolist()
        if len(names) == len(v) and all(isinstance(s, str) and s for s in names) and len(set(names)) == len(names):
            attrs.pop("names")
            v = dict(zip(names, v))
    return RValue(v, attrs) if attrs else v


def _decode_on_device(buf, pos, n, es):
    """n big-endian elements at buf[pos:] as a native CUDA vector (icnv_xdr_decode_dev), through two pinned buffers."""
    import torch
    from . import device as dev
    out = torch.empty(n, dtype=torch.float64 if es == 8 else torch.int32, device="cuda")
    per_chunk = max(1, min(CHUNK_BYTES, -(-n * es // 16) * 16) // es)
    pin = [torch.empty(per_chunk * es, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
    stage = [torch.empty(per_chunk * es, dtype=torch.uint8, device="cuda") for _ in range(2)]
    events = [None, None]
    src = np.frombuffer(buf, dtype=np.uint8, count=n * es, offset=pos)
    for i, e0 in enumerate(range(0, n, per_chunk)):
        slot, e1 = i % 2, min(n, e0 + per_chunk)
        if events[slot] is not None:
            events[slot].synchronize()          # the copy out of this pinned buffer has finished
        k = (e1 - e0) * es
        pin[slot].numpy()[:k] = src[e0 * es:e0 * es + k]
        stage[slot][:k].copy_(pin[slot][:k], non_blocking=True)
        events[slot] = torch.cuda.Event()
        events[slot].record()
        dev.xdr_decode(stage[slot], out, e0=e0, e1=e1)
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------------------- gzip inflated on the device (K29)
INFLATE_MAX_IN = 16 << 20           # the most compressed bytes one unit may take (inflate_gzip's max_in)
INFLATE_CRC_PIECE = 1 << 16         # the pieces the inflated stream's CRC-32 is computed in
WINDOW_BYTES = 4 << 20              # the host window of a device-resident stream
_INFLATE_STATS = {"route": "none", "reason": "inflate_gzip has not run"}


class _DeviceStream:
    """The inflated stream where inflate_gzip left it, as the buffer _Reader parses: a host window of WINDOW_BYTES is fetched
    on demand (everything but the payloads is small, and the payloads are decoded from `tensor` device to device).  fetch(lo,
    hi) returns the bytes [lo, hi); tensor: the CUDA uint8 vector itself, or None (a stand-in without one)."""

    def __init__(self, fetch, n, tensor=None):
        self.fetch, self.n, self.tensor = fetch, int(n), tensor
        self.lo, self.win = 0, memoryview(b"")

    def __len__(self):
        return self.n

    def _window(self, pos, k):
        """The offset in the window of stream byte pos, with k bytes from there inside it."""
        if pos < self.lo or pos + k > self.lo + len(self.win):
            self.lo = pos
            self.win = memoryview(self.fetch(pos, min(self.n, pos + max(k, WINDOW_BYTES))))
        return pos - self.lo

    def int_at(self, pos):
        o = self._window(pos, 4)                              # (first: it may replace the window)
        return struct.unpack_from(">i", self.win, o)[0]

    def __getitem__(self, s):
        lo, hi, step = s.indices(self.n)
        if step != 1:
            raise ValueError("contiguous slices only")
        k = max(hi - lo, 0)
        if k > WINDOW_BYTES:                                  # a payload for the host: not through the window
            return memoryview(self.fetch(lo, hi))
        o = self._window(lo, k)
        return self.win[o:o + k]


def _decode_device_stream(stream, pos, n, es):
    """n big-endian elements at byte pos of the CUDA uint8 vector `stream` as a native CUDA vector.  icnv_xdr_decode_dev wants
    its source aligned to the element size and a payload's offset in the stream is arbitrary: the segment goes through an
    aligned staging tensor, CHUNK_BYTES at a time, device to device."""
    import torch
    from . import device as dev
    out = torch.empty(n, dtype=torch.float64 if es == 8 else torch.int32, device=stream.device)
    per_chunk = max(1, min(CHUNK_BYTES, -(-n * es // 16) * 16) // es)
    stage = torch.empty(per_chunk * es, dtype=torch.uint8, device=stream.device)
    for e0 in range(0, n, per_chunk):
        e1 = min(n, e0 + per_chunk)
        k = (e1 - e0) * es
        stage[:k].copy_(stream[pos + e0 * es:pos + e0 * es + k])
        dev.xdr_decode(stage, out, e0=e0, e1=e1)
    return out


class _DeviceBytes:
    """What the device sides of inflate_gzip (K29) and gunzip.gunzip (K30) share: the file's bytes up, the CRC-32 of the
    result, and the result as the stream read_rds parses."""

    def upload(self, view):
        """The bytes of a host buffer as a CUDA uint8 vector, through two pinned buffers."""
        import torch
        n = len(view)
        src = torch.empty(n, dtype=torch.uint8, device="cuda")
        host = np.frombuffer(view, dtype=np.uint8)
        per = min(CHUNK_BYTES, max(n, 1))
        pin = [torch.empty(per, dtype=torch.uint8, pin_memory=True) for _ in range(2 if n > per else 1)]
        events = [None, None]
        for i, o in enumerate(range(0, n, per)):
            slot, k = i % 2, min(per, n - o)
            if events[slot] is not None:
                events[slot].synchronize()
            pin[slot].numpy()[:k] = host[o:o + k]
            src[o:o + k].copy_(pin[slot][:k], non_blocking=True)
            events[slot] = torch.cuda.Event()
            events[slot].record()
        torch.cuda.synchronize()
        return src

    def crc32_pieces(self, out, piece_bytes):
        from . import device as dev
        return dev.crc32_pieces(out, piece_bytes).cpu().numpy()

    def stream(self, out):
        fetch = lambda lo, hi: out[lo:hi].cpu().numpy().tobytes()
        return _DeviceStream(fetch, int(out.numel()), out)


class _DeviceInflate(_DeviceBytes):
    """The device side of inflate_gzip: host arrays are numpy, `src` and `out` stay where upload / alloc put them."""

    def scan(self, src):
        from . import device as dev
        return dev.inflate_scan(src).cpu().numpy()

    def measure(self, src, start, max_in):
        import torch
        from . import device as dev
        end, out_len, status = dev.inflate_measure(src, torch.from_numpy(start).to(src.device), max_in)
        return end.cpu().numpy(), out_len.cpu().numpy(), status.cpu().numpy()

    def alloc(self, src, nbytes):
        import torch
        return torch.empty(nbytes, dtype=torch.uint8, device=src.device)

    def units(self, src, start, end, out_off, out_len, out):
        import torch
        from . import device as dev
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(src.device)
        return dev.inflate_units(src, up(start), up(end), up(out_off), up(out_len), out).cpu().numpy()


def _inflate_backend():
    return _DeviceInflate()


def _inflate_enabled():
    """ICNV_INFLATE=0 (environment, read per call): gzip files are inflated on the host even where a GPU is present."""
    return os.environ.get("ICNV_INFLATE", "1").strip() != "0"


def inflate_stats():
    """What the latest inflate_gzip did: route ("device", or "host" with the reason it gave up), decode_launched, candidates,
    chain_units, false_candidates, compressed_bytes, inflated_bytes, and seconds per phase (upload, scan, measure, chain,
    decode, crc)."""
    return dict(_INFLATE_STATS, seconds=dict(_INFLATE_STATS.get("seconds", {})))


def gzip_header_length(data):
    """The bytes of a gzip member's header (RFC 1952): FEXTRA, FNAME, FCOMMENT and FHCRC are stepped over.  None when the bytes
    are no deflate member's header, or end inside it."""
    n = len(data)
    if n < 10 or bytes(data[:3]) != b"\x1f\x8b\x08" or data[3] & 0xE0:
        return None
    flg, at = data[3], 10
    if flg & 4:                                               # FEXTRA
        if at + 2 > n:
            return None
        at += 2 + struct.unpack_from("<H", data, at)[0]
    for bit in (8, 16):                                       # FNAME, FCOMMENT: zero-terminated
        if flg & bit:
            while at < n and data[at] != 0:
                at += 1
            at += 1
    if flg & 2:                                               # FHCRC
        at += 2
    return at if at <= n else None


def _walk_chain(start, end, status, refusal):
    """The chain of true units among the measured ones (K29's and K30's): from unit 0, the unit that starts where the one
    before it ends, up to the first with status 1 (OK_FINAL).  start is ascending; start and end count alike (bytes, or bits).
    Returns (indices, None), or (None, refusal(i, s)) for the first unit i whose status s is no OK, or which ends (s None) on
    no later unit's start: the wording is the caller's."""
    nxt_l, end_l, st_l, start_l = np.searchsorted(start, end).tolist(), end.tolist(), status.tolist(), start.tolist()
    chain, i = [], 0
    while True:                                               # every step moves forward: j > i
        chain.append(i)
        if st_l[i] == 1:
            return np.asarray(chain, dtype=np.int64), None
        if st_l[i] != 0:
            return None, refusal(i, st_l[i])
        j = nxt_l[i]
        if j <= i or j >= len(start_l) or start_l[j] != end_l[i]:
            return None, refusal(i, None)
        i = j


def _isize_matches(view, total):
    """Does ISIZE, the last 4 bytes of the gzip file `view`, equal `total` inflated bytes mod 2^32 (tested before anything is
    decoded)?"""
    return struct.unpack("<I", bytes(view[len(view) - 4:]))[0] == total & 0xFFFFFFFF


def _crc32_matches(view, be, out, total):
    """Does the CRC-32 of the `total` inflated bytes `out` on the device -- INFLATE_CRC_PIECE pieces there (be.crc32_pieces),
    folded on the host; 0 for no bytes, without a launch -- equal the trailer's, bytes [-8, -4) of the gzip file `view`?"""
    got = 0
    if total:
        from .device import crc32_combine_pieces
        crcs = be.crc32_pieces(out, INFLATE_CRC_PIECE)
        got = crc32_combine_pieces(crcs, INFLATE_CRC_PIECE, total - (len(crcs) - 1) * INFLATE_CRC_PIECE)
    return got == struct.unpack("<I", bytes(view[len(view) - 8:len(view) - 4]))[0]


def inflate_gzip(data, *, max_in=INFLATE_MAX_IN):
    """The inflated stream of a one-member gzip file with flush points -- what write_rds(compress=True) writes on the device
    route -- as a CUDA uint8 tensor (read_rds parses it from there through a _DeviceStream), inflated unit by unit on the
    device (DESIGN K29; the contract of a unit is in include/icnv.h).  data: bytes, an mmap or a path.  The file
    carries no index of its units, so: scan for the flush markers, measure the unit behind every candidate, walk the chain of
    true units from the stream's first byte (end of one = start of the next, up to the unit with BFINAL, with exactly the
    8-byte trailer behind it), decode the chain's units into their places, and check ISIZE and the CRC-32 (computed on the device
    in pieces, folded on the host).  Returns None whenever that does not work out -- too few candidates for the file's size or a
    single unit (no flush points: R's own files), a unit that needs history, is malformed, truncated or longer than max_in, a
    second member, a wrong trailer -- and never raises for the file's content: the host route then succeeds or raises as it
    always did.  inflate_stats() tells what happened."""
    global _INFLATE_STATS
    st = {"route": "host", "reason": "", "decode_launched": False, "candidates": 0, "chain_units": 0, "false_candidates": 0,
          "compressed_bytes": 0, "inflated_bytes": 0, "seconds": {}}
    _INFLATE_STATS = st
    if isinstance(data, (str, os.PathLike)):
        with open(data, "rb") as fh:
            data = mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ) if os.fstat(fh.fileno()).st_size else b""
    out = _inflate_gzip(data, int(max_in), st)
    if out is not None:
        st["route"] = "device"
    return out


def _inflate_gzip(data, max_in, st):
    def give_up(reason):
        st["reason"] = reason
        return None

    clock = time.perf_counter
    view = memoryview(data)
    head = gzip_header_length(view)
    if head is None:
        return give_up("not a gzip header")
    n = len(view) - head                                      # the raw stream and the trailer
    st["compressed_bytes"] = len(view)
    if n < 8 + 2:
        return give_up("truncated file")
    be = _inflate_backend()
    t0 = clock()
    src = be.upload(view[head:])
    t1 = clock()
    cand = np.asarray(be.scan(src), dtype=np.int64)
    t2 = clock()
    st["seconds"].update(upload=t1 - t0, scan=t2 - t1)
    start = np.concatenate([np.zeros(1, dtype=np.int64), cand[cand < n - 8]])
    st["candidates"] = int(start.size)
    if start.size < 2 or start.size * max_in < n:             # some unit must be longer than max_in: a stream without flush points
        return give_up("no flush points: no decode launched")
    end, out_len, status = be.measure(src, start, max_in)
    t3 = clock()
    ok = status <= 1                                          # OK_MARKER, OK_FINAL
    if ok.all() and np.array_equal(end[:-1], start[1:]) and (status[:-1] == 0).all():
        chain = np.arange(start.size)                         # every candidate is a true unit
    else:
        chain, refused = _walk_chain(start, end, status, lambda i, s: f"the unit at byte {head + int(start[i])} " + (
            "does not end on a candidate" if s is None else f"has status {_INFLATE_STATUS[s]}") + ": no decode launched")
        if chain is None:
            return give_up(refused)
    last = int(chain[-1])
    st["seconds"].update(measure=t3 - t2, chain=clock() - t3)
    st["chain_units"], st["false_candidates"] = int(chain.size), int(start.size - chain.size)
    if status[last] != 1:
        return give_up("the chain does not end with a final block: no decode launched")
    if int(end[last]) != n - 8:
        return give_up("the stream is not followed by exactly the 8-byte trailer (a second member?): no decode launched")
    if chain.size < 2:
        return give_up("one unit, no flush points: no decode launched")
    c_start, c_end, c_len = start[chain], end[chain], out_len[chain]
    c_off = np.cumsum(c_len) - c_len
    total = int(c_len.sum())
    if not _isize_matches(view, total):
        return give_up("the trailer's ISIZE does not match: no decode launched")
    st["inflated_bytes"] = total
    t4 = clock()
    out = be.alloc(src, total)
    st["decode_launched"] = True
    got = be.units(src, c_start, c_end, c_off, c_len, out)
    t5 = clock()
    st["seconds"].update(decode=t5 - t4)
    if not np.array_equal(got, status[chain]):
        return give_up("the decode disagrees with the measure")
    crc_ok = _crc32_matches(view, be, out, total)
    st["seconds"].update(crc=clock() - t5)
    if not crc_ok:
        return give_up("the trailer's CRC-32 does not match")
    return out


_INFLATE_STATUS = ("OK_MARKER", "OK_FINAL", "TRUNCATED", "TOO_LONG", "BAD_STREAM", "NEEDS_HISTORY")


def _open_on_device(path):
    """The _DeviceStream of a gzip file that inflate_gzip or, where that gives up, gunzip.gunzip takes, or None: not gzip, no
    GPU, ICNV_INFLATE=0, or turned away by both."""
    if not (_inflate_enabled() and _device_available()):
        return None
    with open(path, "rb") as fh:
        if fh.read(2) != b"\x1f\x8b":
            return None
    out = inflate_gzip(path)
    if out is not None:
        return _inflate_backend().stream(out)
    from . import gunzip                                      # K30: a stream without flush points (R's, GzipFile's)
    opened = gunzip.open_on_device(path)
    return None if opened is None else opened[1]


def _open_bytes(path):
    """(buffer, compressed?): the file's serialised bytes; an uncompressed file is mapped, not read."""
    with open(path, "rb") as fh:
        magic = fh.read(6)
        fh.seek(0)
        for m, fn in ((b"\x1f\x8b", gzip.decompress), (b"\xfd7zXZ\x00", lzma.decompress), (b"BZh", bz2.decompress)):
            if magic.startswith(m):
                try:
                    return fn(fh.read()), True
                except (EOFError, OSError, lzma.LZMAError) as exc:
                    raise ValueError(f"truncated or damaged compressed file: {exc}") from None
        if not magic:
            raise ValueError("truncated file: it is empty")
        return mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ), False


def read_rds(path, *, return_device=False):
    """Reads an .rds file -- ours or R's, formats 2 and 3, uncompressed or gzip / bzip2 / xz (recognised by magic, inflated on
    the host) -- into the value model of the module docstring.  A save()-style container (.rda: RDX2 / RDX3) gives the dict of
    its variables.  REFSXP and the ALTREP classes compact_intseq, compact_realseq, deferred_string and wrap_real / _integer
    / _logical / _string are resolved; LANGSXP surfaces as RLang().  Any other type raises ValueError with the type code and
    the byte offset of its flag word; a file that ends early raises ValueError.  return_device=True: REALSXP / INTSXP
    payloads of at least DEVICE_THRESHOLD bytes of an uncompressed or inflated file are decoded on the device
    (icnv_xdr_decode_dev); a matrix stays there and comes back as RDeviceMatrix of the (cols, rows) tensor, a plain vector is
    copied back.  A gzip file is then first offered to inflate_gzip (DESIGN K29): one written with flush points -- ours, with
    compress=True -- is inflated on the device and parsed from there, the payloads decoded device to device; any other -- R's
    own, GzipFile's: no flush points -- is offered to gunzip.gunzip (DESIGN K30), which inflates any one-member gzip stream of
    at least gunzip.GUNZIP_MIN_BYTES on the device, .rds and gzip .rda alike; what that turns away too falls back to the host's
    inflate (ICNV_GUNZIP=0: K30 off; ICNV_INFLATE=0: both off, always the host).  All routes return the same values."""
    buf = _open_on_device(path) if return_device else None
    if buf is None:
        buf, _ = _open_bytes(path)
    rd = _Reader(buf, return_device)
    container = rd.header()
    top = rd.item()
    if container == "rda":
        if not isinstance(top, _Pairlist):
            raise ValueError("an .rda container holds a tagged pairlist")
        return top.as_dict()
    if isinstance(top, _Pairlist):
        return RValue(top.values, {"names": _str_array([t or "" for t in top.tags])})
    return top


# ---------------------------------------------------------------------------------------------- count matrices (K34)
@dataclass
class RdsPayload:
    """A REALSXP / INTSXP vector where it lies in the serialised stream: `length` big-endian elements of `elem_size` bytes from
    byte `offset` on.  sexp: REALSXP or INTSXP.  value: the decoded array when the vector is below DEVICE_THRESHOLD, else None."""
    offset: int
    elem_size: int
    length: int
    sexp: int
    value: object = None

    @property
    def nbytes(self):
        return self.length * self.elem_size


@dataclass
class RdsCounts:
    """What locate_counts found: kind ("matrix_real", "matrix_int", "data_frame", "dgCMatrix"), the G x C shape, the gene and
    cell names, the payloads (one for a matrix, one per column for a data.frame, i, p and x for a dgCMatrix), nnz (the length
    of x; None for the dense kinds) and container (None, or "rda" with `variable` the name of the one variable)."""
    kind: str
    G: int
    C: int
    genes: list
    cells: list
    payloads: list
    nnz: object = None
    container: object = None
    variable: object = None


@dataclass
class RNoPayload:
    """An ALTREP compact_intseq / compact_realseq met where locate_counts looks for payloads: R stores (length, start, step), so
    the vector has no elements in the stream.  cls: the ALTREP class; value: the expanded sequence."""
    cls: str
    value: object


class _LocatingReader(_Reader):
    """_Reader in the mode of locate_counts.  A REALSXP or INTSXP vector that can be a count payload -- the top-level value, an
    element of a list, a slot of an S4 object, the vector inside an ALTREP wrap_real / wrap_integer -- is recorded as an
    RdsPayload, and decoded only when it is smaller than DEVICE_THRESHOLD.  Everything else is read as always, into plain
    arrays: strings, logicals, every attribute of a vector or list (dim, dimnames, names, row.names, class, levels), and the
    state of the other ALTREP classes (the three numbers of a compact sequence, the argument of a deferred_string).  A compact
    sequence in a payload's place comes back as RNoPayload."""

    def __init__(self, buf):
        super().__init__(buf)
        self.plain = 0                           # > 0 while attributes or ALTREP state are read: numeric() is _Reader's

    def numeric(self, t, n):
        if t == LGLSXP or self.plain:
            return super().numeric(t, n)
        es = 8 if t == REALSXP else 4
        pos = self.pos
        if n * es >= DEVICE_THRESHOLD:
            self.need(n * es)
            self.pos += n * es
            return RdsPayload(pos, es, n, t)
        return RdsPayload(pos, es, n, t, super().numeric(t, n))

    def plainly(self, read):
        self.plain += 1
        try:
            return read()
        finally:
            self.plain -= 1

    def finish(self, v, has_attr):
        return _with_attrs(v, self.plainly(self.attrs) if has_attr else {})

    def altrep_parts(self, cls):
        if cls in ("wrap_real", "wrap_integer"):  # the wrapped vector is a payload like any other; its attributes are not
            return self.item(), self.plainly(self.item)
        return self.plainly(lambda: (self.item(), self.item()))

    def compact_seq(self, cls, seq):
        return seq if self.plain else RNoPayload(cls, seq)


def _small(v, what):
    """The host array of a short vector that locate_counts needs here (the slot Dim)."""
    if isinstance(v, RValue):
        v = v.value
    if isinstance(v, (RdsPayload, RNoPayload)):
        if v.value is None:
            raise ValueError(f"{what}: a vector of {v.length} elements where a short one is expected")
        v = v.value
    return None if v is None else np.asarray(v)


def _name_vector(v):
    """The list of names of a character vector, or None for anything else (NULL, compact integer row.names)."""
    if isinstance(v, RValue):
        v = v.value
    if isinstance(v, np.ndarray) and v.dtype.kind in "US":
        return [str(s) for s in v.tolist()]
    if isinstance(v, np.ndarray) and v.dtype.kind == "O" and all(isinstance(s, str) for s in v.tolist()):
        return list(v.tolist())
    return None


def _dim_names(dn, what):
    """(row names, column names) of a dimnames / Dimnames value: each a list, or None."""
    if dn is None:
        return None, None
    if isinstance(dn, RValue):
        dn = dn.value
    if isinstance(dn, dict):
        dn = list(dn.values())
    if not (isinstance(dn, list) and len(dn) == 2):
        raise ValueError(f"{what}: expected a list of two")
    return _name_vector(dn[0]), _name_vector(dn[1])


def _describe(v):
    """What a value is, for a refusal."""
    if isinstance(v, RS4):
        return f"an S4 object of class {v.cls!r}"
    if isinstance(v, RFactor):
        return "a factor"
    if isinstance(v, RValue):
        cls = v.attrs.get("class")
        if cls is not None and "factor" in [str(c) for c in np.asarray(cls.value if isinstance(cls, RValue) else cls).ravel()]:
            return "a factor"
        if cls is not None:
            return "an object of class " + "/".join(repr(str(c)) for c in np.asarray(cls.value if isinstance(cls, RValue) else cls).ravel())
        return _describe(v.value) + " with the attributes " + ", ".join(v.attrs)
    if isinstance(v, RdsPayload):
        return ("a numeric" if v.sexp == REALSXP else "an integer") + " vector"
    if isinstance(v, RNoPayload):
        return f"an ALTREP {v.cls} (a sequence R stores as length, start and step: it has no elements in the stream)"
    if isinstance(v, np.ndarray):
        return {"U": "a character", "S": "a character", "O": "a character", "b": "a logical"}.get(v.dtype.kind, "a numeric") + (" matrix" if v.ndim == 2 else " vector")
    if isinstance(v, (list, dict)):
        return "a list"
    return "NULL" if v is None else f"a {type(v).__name__}"


def _names_or_given(found, given, n, what, missing):
    if given is not None:
        given = [str(s) for s in given]
        if len(given) != n:
            raise ValueError(f"{what}: {len(given)} names were passed, the matrix has {n}")
        return given
    if found is None:
        raise ValueError(missing)
    if len(found) != n:
        raise ValueError(f"{what}: {len(found)} names for {n}")
    return found


def locate_counts(buf, *, gene_names=None, cell_names=None):
    """Where the count matrix of a serialised stream lies (DESIGN K34): `buf` is what _Reader parses -- an mmap, bytes, or the
    _DeviceStream of a file inflated on the device.  The stream is walked with _Reader, but a REALSXP / INTSXP vector of at
    least DEVICE_THRESHOLD bytes is not decoded: it is recorded as an RdsPayload (byte offset, element size, length); smaller
    ones are recorded AND decoded (RdsPayload.value).  Returns an RdsCounts.

    Accepted: an .rds whose value is a numeric or integer matrix (attributes dim and dimnames only), a data.frame of numeric /
    integer columns of one length with character row.names, or a dgCMatrix (package Matrix: slots i, p, Dim, Dimnames, x,
    factors); and an .rda / .RData container that holds exactly one variable of one of them.  Everything else is a ValueError
    that names what was found: another S4 class, a data.frame column that is a factor, character or logical (with the column's
    name), further attributes on a matrix, compact row.names or missing dimnames / Dimnames (unless gene_names / cell_names are
    passed: they then supply the names, and their lengths must match), columns of unequal length, a Dim that disagrees with
    length(p) - 1, length(i) != length(x).  (length(x) != p[C] needs p: icnv_rds_csc_check_dev tests it on the device.)"""
    rd = _LocatingReader(buf)
    container = rd.header()
    top = rd.item()
    variable = None
    if container == "rda":
        if not isinstance(top, _Pairlist):
            raise ValueError("an .rda container holds a tagged pairlist")
        if len(top.values) != 1:
            raise ValueError(f"the container holds {len(top.values)} variables ({', '.join(str(t) for t in top.tags)}); exactly one count matrix is read")
        variable, top = top.tags[0], top.values[0]
    what = "the file" if variable is None else f"the variable {variable!r}"
    out = RdsCounts("", 0, 0, None, None, [], None, container, variable)
    no_genes = f"{what} has no row names: pass gene_names"
    no_cells = f"{what} has no column names: pass cell_names"
    if isinstance(top, RS4):
        if top.cls != "dgCMatrix":
            raise ValueError(f"{what} holds an S4 object of class {top.cls!r}; of the Matrix classes only dgCMatrix is read")
        sl = top.slots
        for name, sexp in (("i", INTSXP), ("p", INTSXP), ("x", REALSXP)):
            if not (isinstance(sl.get(name), RdsPayload) and sl[name].sexp == sexp):
                raise ValueError(f"{what}: slot {name} of the dgCMatrix is {_describe(sl.get(name))}")
        dim = _small(sl.get("Dim"), "slot Dim")
        if dim is None or dim.size != 2 or int(dim[0]) < 1 or int(dim[1]) < 1:
            raise ValueError(f"{what}: slot Dim of the dgCMatrix is not two positive integers")
        out.kind, out.G, out.C = "dgCMatrix", int(dim[0]), int(dim[1])
        i, p, x = sl["i"], sl["p"], sl["x"]
        if p.length - 1 != out.C:
            raise ValueError(f"{what}: Dim says {out.C} columns, p has {p.length} entries ({p.length - 1} columns)")
        if i.length != x.length:
            raise ValueError(f"{what}: i has {i.length} entries, x has {x.length}")
        if x.length > 0x7FFFFFFF:
            raise ValueError(f"{what}: a dgCMatrix of {x.length} entries is beyond 2^31 - 1")
        g, c = _dim_names(sl.get("Dimnames"), "slot Dimnames")
        if g is None and gene_names is None:
            no_genes = f"{what}: the dgCMatrix has no row names in Dimnames: pass gene_names"
        if c is None and cell_names is None:
            no_cells = f"{what}: the dgCMatrix has no column names in Dimnames: pass cell_names"
        out.payloads, out.nnz = [i, p, x], x.length
    elif isinstance(top, RValue) and isinstance(top.value, RdsPayload):
        extra = [k for k in top.attrs if k not in ("dim", "dimnames")]
        if extra:
            raise ValueError(f"{what} holds a matrix with the attributes {', '.join(extra)} beyond dim and dimnames")
        dim = _small(top.attrs.get("dim"), "dim")
        if dim is None or dim.size != 2:
            raise ValueError(f"{what} holds {_describe(top.value)} that is no matrix (dim has {0 if dim is None else dim.size} entries)")
        pl = top.value
        out.G, out.C = int(dim[0]), int(dim[1])
        if out.G < 1 or out.C < 1 or out.G * out.C != pl.length:
            raise ValueError(f"{what}: dim is {out.G} x {out.C}, the vector has {pl.length} elements")
        out.kind = "matrix_real" if pl.sexp == REALSXP else "matrix_int"
        g, c = _dim_names(top.attrs.get("dimnames"), "dimnames")
        out.payloads = [pl]
    elif isinstance(top, RValue) and isinstance(top.value, (dict, list)) and "data.frame" in [
            str(k) for k in np.asarray(_small(top.attrs.get("class"), "class") if top.attrs.get("class") is not None else []).ravel()]:
        if isinstance(top.value, dict):
            names, cols = list(top.value), list(top.value.values())
        else:
            names, cols = _name_vector(top.attrs.get("names")), top.value
        if not cols:
            raise ValueError(f"{what} holds a data.frame without columns")
        for k, col in enumerate(cols):
            label = repr(names[k]) if names is not None and k < len(names) else f"number {k + 1}"
            if not isinstance(col, RdsPayload):
                raise ValueError(f"{what}: column {label} of the data.frame is {_describe(col)}; only numeric and integer columns stored in full are read")
            if col.length != cols[0].length:
                raise ValueError(f"{what}: column {label} of the data.frame has {col.length} rows, the first column has {cols[0].length}")
        out.kind, out.G, out.C = "data_frame", cols[0].length, len(cols)
        if out.G < 1:
            raise ValueError(f"{what} holds a data.frame without rows")
        g, c = _name_vector(top.attrs.get("row.names")), names
        if g is None and gene_names is None:
            no_genes = f"{what}: the data.frame has compact row.names (no gene names): pass gene_names"
        out.payloads = list(cols)
    else:
        raise ValueError(f"{what} holds {_describe(top)}; a numeric matrix, a data.frame or a dgCMatrix is read")
    out.genes = _names_or_given(g, gene_names, out.G, "gene_names", no_genes)
    out.cells = _names_or_given(c, cell_names, out.C, "cell_names", no_cells)
    return out


def open_counts(path, *, device=True):
    """(buf, route, reason) for locate_counts and device.read_rds_counts: the serialised bytes of `path` and how they were got.
    route "none": an uncompressed file, mapped; "device_k29" / "device_k30": a gzip file inflated on the device (buf is the
    _DeviceStream; _open_on_device); "host": gzip turned away there, bzip2 or xz, inflated by Python -- reason says why."""
    if device:
        buf = _open_on_device(path)
        if buf is not None:
            return buf, ("device_k29" if inflate_stats().get("route") == "device" else "device_k30"), ""
    buf, compressed = _open_bytes(path)
    if not compressed:
        return buf, "none", ""
    with open(path, "rb") as fh:
        gz = fh.read(2) == b"\x1f\x8b"
    if not gz:
        return buf, "host", "not a gzip file"
    if not device or not _device_available():
        return buf, "host", "no device"
    if not _inflate_enabled():
        return buf, "host", "ICNV_INFLATE=0"
    from . import gunzip
    return buf, "host", f"K29: {inflate_stats().get('reason', '')}; K30: {gunzip.gunzip_stats().get('reason', '')}"


def close_counts(buf):
    """Closes the mapping open_counts made of an uncompressed file (nothing to do for bytes or a device stream).  No NumPy view
    of it may be alive."""
    if isinstance(buf, mmap.mmap):
        buf.close()


# ================================================================================================================ infercnv objects
SLOTS = ("expr.data", "count.data", "gene_order", "reference_grouped_cell_indices", "observation_grouped_cell_indices",
         "tumor_subclusters", "options", ".hspike")
HCLUST_NAMES = ("merge", "height", "order", "labels", "method", "call", "dist.method")


def _names(a):
    return np.array([str(s) for s in np.asarray(a).tolist()], dtype=object)


def _matrix_value(m, genes, cells, x_dev=None):
    dimnames = {"dimnames": [genes, cells]}
    if x_dev is None and isinstance(m, DeviceMatrix):       # a resident object (DESIGN K32) is encoded from where it lives
        x_dev = m.float_tensor()
    if x_dev is not None:
        if tuple(x_dev.shape) != (len(cells), len(genes)):
            raise ValueError(f"x_dev has the shape {tuple(x_dev.shape)}, the object's matrix is (cells, genes) = {(len(cells), len(genes))}")
        return RValue(RDeviceMatrix(x_dev), dimnames)
    if m is None:
        return None
    if hasattr(m, "tocsc"):
        s = m.tocsc()
        s.sort_indices()
        return RS4("dgCMatrix", "Matrix", {"i": np.asarray(s.indices, dtype=np.int32), "p": np.asarray(s.indptr, dtype=np.int32),
                                           "Dim": np.array(s.shape, dtype=np.int32), "Dimnames": [genes, cells],
                                           "x": np.asarray(s.data, dtype=np.float64), "factors": []})
    m = np.asarray(m)
    if m.ndim != 2 or m.shape != (len(genes), len(cells)):
        raise ValueError(f"a matrix of shape {m.shape} does not fit {len(genes)} genes x {len(cells)} cells")
    return RValue(m, dimnames)


def _column(v):
    v = np.asarray(v)
    if v.dtype.kind == "f" and np.array_equal(v, np.rint(v)) and (v.size == 0 or np.abs(v).max() <= 0x7FFFFFFF):
        return v.astype(np.int32)
    return v


def _option(v):
    if isinstance(v, dict):
        return {str(k): _option(e) for k, e in v.items()}
    if isinstance(v, (list, tuple)):
        kinds = {_scalar_kind(e) for e in v}
        if v and None not in kinds and (len(kinds) == 1 or kinds == {"i", "f"}):
            kind = "f" if "f" in kinds else kinds.pop()
            return np.array(list(v), dtype={"b": np.bool_, "i": np.int64, "f": np.float64, "s": object}[kind])
        return [_option(e) for e in v]
    if v is None or _scalar_kind(v) is not None or isinstance(v, np.ndarray):
        return v
    raise ValueError(f"slot options: a {type(v).__name__} has no R form here")


def _hclust_value(h):
    if h is None:
        return None
    if isinstance(h, (list, tuple)):
        return [_hclust_value(e) for e in h]
    return RValue({"merge": np.asarray(h.merge, dtype=np.int32).reshape(-1, 2), "height": np.asarray(h.height, dtype=np.float64),
                   "order": np.asarray(h.order, dtype=np.int32), "labels": _names(h.labels), "method": str(h.method),
                   "call": None, "dist.method": str(h.dist_method)}, {"class": "hclust"})


def to_r(obj: InfercnvObject, x_dev=None) -> RS4:
    """The RS4 value of an InfercnvObject (module docstring: the infercnv object as R stores it)."""
    if x_dev is None and obj.expr_data is None:
        raise ValueError("slot expr.data: the object has no matrix and no x_dev was given")
    G, C = (x_dev.shape[1], x_dev.shape[0]) if x_dev is not None else obj.expr_data.shape
    genes = _names(obj.gene_names if obj.gene_names is not None else [f"gene_{i + 1}" for i in range(G)])   # as genes()
    cells = _names(obj.cell_names if obj.cell_names is not None else [f"cell_{i + 1}" for i in range(C)])   # as cells()
    go = obj.gene_order
    chrs = [str(c) for c in np.asarray(go.chr).tolist()]
    levels = list(dict.fromkeys(chrs))
    code = {l: i for i, l in enumerate(levels)}
    frame = {"chr": RFactor(np.array([code[c] for c in chrs], dtype=np.int64), levels)}
    if go.start is not None:
        frame["start"] = _column(go.start)
    if go.stop is not None:
        frame["stop"] = _column(go.stop)
    groups = lambda d: {str(k): np.asarray(v, dtype=np.int64) + 1 for k, v in (d or {}).items()}
    ts = obj.tumor_subclusters
    ts_value = None
    if ts is not None:
        ts_value = {"hc": {str(g): _hclust_value(h) for g, h in (ts.get("hc") or {}).items()},
                    "subclusters": {str(g): {str(s): RValue(np.asarray(idx, dtype=np.int64).ravel() + 1,
                                                            {"names": cells[np.asarray(idx, dtype=np.int64).ravel()]})
                                             for s, idx in subs.items()}
                                    for g, subs in (ts.get("subclusters") or {}).items()}}
        for k in ts:
            if k not in ("hc", "subclusters"):
                raise ValueError(f"slot tumor_subclusters: the entry {k!r} has no R form here")
    slots = {"expr.data": _matrix_value(obj.expr_data, genes, cells, x_dev),
             "count.data": _matrix_value(obj.count_data, genes, cells),
             "gene_order": RValue(frame, {"row.names": genes, "class": "data.frame"}),
             "reference_grouped_cell_indices": groups(obj.reference_grouped_cell_indices),
             "observation_grouped_cell_indices": groups(obj.observation_grouped_cell_indices),
             "tumor_subclusters": ts_value,
             "options": {str(k): _option(v) for k, v in (obj.options or {}).items()},
             ".hspike": None if obj.hspike is None else to_r(obj.hspike)}
    return RS4("infercnv", "infercnv", slots)


def save_infercnv_obj(obj: InfercnvObject, path, *, x_dev=None, compress=False, device=None):
    """saveRDS(infercnv_obj, path): the object as the `infercnv` S4 object R reads (module docstring).  x_dev: the object's
    matrix as the (cells, genes) CUDA float64 tensor when the caller holds it there, as sample_object and plot_per_group
    do: it is encoded from where it lives, nothing is uploaded or transposed, and obj.expr_data is not looked at.  compress,
    device: as write_rds.  Returns write_rds' statistics."""
    return write_rds(to_r(obj, x_dev), path, compress=compress, device=device)


def _plain(v, slot):
    """An options value back in Python's terms."""
    if isinstance(v, dict):
        return {k: _plain(e, slot) for k, e in v.items()}
    if isinstance(v, list):
        return [_plain(e, slot) for e in v]
    if v is None:
        return None
    if isinstance(v, np.ndarray):
        return v.ravel()[0].item() if v.size == 1 else v.tolist()
    raise ValueError(f"slot {slot}: a {type(v).__name__} cannot be held by the mirror")


def _index_vector(v, slot):
    if isinstance(v, RValue) and set(v.attrs) <= {"names"}:
        v = v.value
    if not (isinstance(v, np.ndarray) and v.ndim == 1 and v.dtype.kind in "iuf"):
        raise ValueError(f"slot {slot}: expected an index vector")
    return v.astype(np.int64) - 1


def _hclust_from(v, slot):
    from .tumor_subclusters import HClust
    if v is None:
        return None
    if isinstance(v, list):
        return [_hclust_from(e, slot) for e in v]
    if not (isinstance(v, RValue) and isinstance(v.value, dict) and set(HCLUST_NAMES) - {"call"} <= set(v.value)):
        raise ValueError(f"slot {slot}: expected an hclust object, a list of them or NULL")
    d = v.value
    return HClust(np.asarray(d["merge"], dtype=np.int32).reshape(-1, 2), np.asarray(d["height"], dtype=np.float64),
                  np.asarray(d["order"], dtype=np.int32), np.asarray(d["labels"]), str(_scalar(d["method"])),
                  str(_scalar(d["dist.method"], "euclidean")))


def _matrix_from(v, slot):
    """(matrix, gene names, cell names) of a matrix slot: a numpy array, a CUDA (cells, genes) tensor, or a csc_matrix."""
    genes = cells = None
    if v is None:
        return None, None, None
    if isinstance(v, RS4):
        if v.cls != "dgCMatrix":
            raise ValueError(f"slot {slot}: an S4 object of class {v.cls!r} cannot be held by the mirror")
        import scipy.sparse as sp
        dn = v.slots.get("Dimnames") or [None, None]
        shape = tuple(int(x) for x in v.slots["Dim"])
        m = sp.csc_matrix((np.asarray(v.slots["x"], dtype=np.float64), np.asarray(v.slots["i"]), np.asarray(v.slots["p"])), shape=shape)
        return m, dn[0], dn[1]
    if isinstance(v, RValue) and set(v.attrs) <= {"dimnames"}:
        dn = v.attrs.get("dimnames") or [None, None]
        genes, cells = dn[0], dn[1]
        v = v.value
    if isinstance(v, RDeviceMatrix):
        return v.tensor, genes, cells
    if not (isinstance(v, np.ndarray) and v.ndim == 2 and v.dtype.kind in "iufb"):
        raise ValueError(f"slot {slot}: expected a numeric matrix or a dgCMatrix")
    return v, genes, cells


def from_r(v, return_device=False):
    """The InfercnvObject of an RS4 of class infercnv (with return_device: and its (cells, genes) CUDA matrix)."""
    if isinstance(v, dict):                                   # an .rda container
        found = [e for e in v.values() if isinstance(e, RS4) and e.cls == "infercnv"]
        if len(found) != 1:
            raise ValueError("the container does not hold exactly one infercnv object")
        v = found[0]
    if not (isinstance(v, RS4) and v.cls == "infercnv"):
        raise ValueError("the file does not hold an object of class infercnv")
    for name in v.slots:
        if name not in SLOTS:
            raise ValueError(f"slot {name}: not a slot of the mirror")
    s = {k: (e if k == "expr.data" else _host(e)) for k, e in v.slots.items()}      # only the matrix stays on the device
    for name in ("expr.data", "gene_order"):
        if s.get(name) is None:
            raise ValueError(f"slot {name}: missing")
    expr, genes, cells = _matrix_from(s["expr.data"], "expr.data")
    counts, _, _ = _matrix_from(s.get("count.data"), "count.data")
    if not isinstance(counts, (type(None), np.ndarray)) and not hasattr(counts, "tocsc"):
        counts = np.ascontiguousarray(counts.cpu().numpy().T)    # a count matrix large enough to be decoded on the device
    go = s["gene_order"]
    frame = go.value if isinstance(go, RValue) else go
    if not (isinstance(frame, dict) and "chr" in frame):
        raise ValueError("slot gene_order: expected a data.frame with the column chr")
    chr_col = frame["chr"]
    if isinstance(chr_col, RFactor):
        chr_col = np.array([None if c < 0 else chr_col.levels[c] for c in chr_col.codes.tolist()])
    col = lambda k: None if frame.get(k) is None else (frame[k].astype(np.int64) if frame[k].dtype.kind in "iu" else frame[k])
    if genes is None and isinstance(go, RValue) and np.asarray(go.attrs.get("row.names", np.zeros(0))).dtype.kind in "UO":
        genes = go.attrs["row.names"]

    def groups(name):
        g = s.get(name)
        if g is None or (isinstance(g, list) and not g):
            return {}
        if not isinstance(g, dict):
            raise ValueError(f"slot {name}: expected a named list of index vectors")
        return {k: _index_vector(e, name) for k, e in g.items()}

    ts = s.get("tumor_subclusters")
    ts_out = None
    if ts is not None and not (isinstance(ts, list) and not ts):
        if not isinstance(ts, dict) or set(ts) - {"hc", "subclusters"}:
            raise ValueError("slot tumor_subclusters: expected list(hc = , subclusters = )")
        as_dict = lambda d, what: {} if d is None or (isinstance(d, list) and not d) else d if isinstance(d, dict) else _refuse(what)
        ts_out = {"hc": {g: _hclust_from(h, "tumor_subclusters") for g, h in as_dict(ts.get("hc"), "hc").items()},
                  "subclusters": {g: {k: _index_vector(e, "tumor_subclusters") for k, e in as_dict(subs, "subclusters").items()}
                                  for g, subs in as_dict(ts.get("subclusters"), "subclusters").items()}}
    opts = s.get("options")
    if opts is None or (isinstance(opts, list) and not opts):
        opts = {}
    if not isinstance(opts, dict):
        raise ValueError("slot options: expected a named list")
    hs = s.get(".hspike")
    x_dev = None
    if not isinstance(expr, np.ndarray) and not hasattr(expr, "tocsc"):
        x_dev, expr = expr.double(), None                        # (an integer matrix: R's numeric values all the same)
    if return_device and x_dev is None:
        import torch
        dense = np.asarray(expr.todense()) if hasattr(expr, "tocsc") else expr
        x_dev, expr = torch.from_numpy(np.ascontiguousarray(dense.T).astype(np.float64)).cuda(), None
    elif not return_device and x_dev is not None:
        expr, x_dev = np.ascontiguousarray(x_dev.cpu().numpy().T), None
    obj = InfercnvObject(expr_data=expr, gene_order=GeneOrder(chr_col, col("start"), col("stop")),
                         reference_grouped_cell_indices=groups("reference_grouped_cell_indices"),
                         observation_grouped_cell_indices=groups("observation_grouped_cell_indices"), count_data=counts,
                         tumor_subclusters=ts_out, options=_plain(opts, "options"),
                         hspike=None if hs is None else from_r(hs),
                         gene_names=None if genes is None else np.asarray(genes), cell_names=None if cells is None else np.asarray(cells))
    return (obj, x_dev) if return_device else obj


def _host(v):
    """`v` with every vector or matrix that was decoded on the device copied back to the host."""
    if isinstance(v, RDeviceMatrix):
        return np.ascontiguousarray(v.tensor.cpu().numpy().T)
    if _is_cuda(v):
        return v.cpu().numpy()
    if isinstance(v, RValue):
        return RValue(_host(v.value), {k: _host(a) for k, a in v.attrs.items()})
    if isinstance(v, RS4):
        return RS4(v.cls, v.package, {k: _host(e) for k, e in v.slots.items()})
    if isinstance(v, dict):
        return {k: _host(e) for k, e in v.items()}
    if isinstance(v, list):
        return [_host(e) for e in v]
    return v


def _refuse(what):
    raise ValueError(f"slot tumor_subclusters: {what} is not a named list")


def load_infercnv_obj(path, *, return_device=False):
    """readRDS(path) as an InfercnvObject, from our files and from R's (.rds, or an .rda that holds one infercnv object).  A
    dgCMatrix becomes a scipy.sparse.csc_matrix; indices become 0-based; the names of the subcluster vectors are dropped (they
    are the cells' names).  A slot R allows but the mirror cannot hold raises ValueError naming the slot.
    return_device=True: the matrix is decoded on the device (when it reaches DEVICE_THRESHOLD; uploaded otherwise -- a gzip
    file is inflated there as well: one with flush points, what compress=True writes, by inflate_gzip; any other one-member
    gzip file of at least gunzip.GUNZIP_MIN_BYTES -- R's own .rds and gzip .rda -- by gunzip.gunzip: read_rds) and the pair
    (object with expr_data None, (cells, genes) CUDA float64 matrix) is
    returned, as sample_object(return_device=True) does."""
    return from_r(read_rds(path, return_device=return_device), return_device)
