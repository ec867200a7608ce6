"""Any one-member gzip file inflated on the device (DESIGN K30; the contract is in include/icnv.h "INFLATE with unknown
history"): R's gzfile, Python's GzipFile, the gzip command line, 10x -- streams without flush points, which K29's
rds.inflate_gzip turns away.  A second route, tried only where K29's gives up.  Consumers: rds.read_rds(return_device=True),
so load_infercnv_obj(return_device=True), of .rds and gzip .rda; device.read_table and device.read_mtx on a path ending in
.gz, and through them CreateInfercnvObject and sharded.ShardedCreate.

    find      every bit offset where a non-final dynamic block's header parses: the candidates
    measure   the unit from bit 0 and from every candidate, up to the next listed candidate or BFINAL
    chain     host: end -> start from bit 0, up to the unit with BFINAL exactly in front of the 8-byte trailer
    symbols   the chain's units decoded into 16-bit symbols: a byte, or a marker for a byte of the 32 KiB in front of the unit
    tails     the last 32 KiB of every unit resolved, unit after unit (the one sequential step)
    resolve   everything else, all units at once
    crc       ISIZE and the CRC-32 (rds.INFLATE_CRC_PIECE pieces on the device, folded on the host)

No R has been involved: R's stream is represented by zlib level 6, the code gzfile runs, and by one R-written .rda."""
from __future__ import annotations

import mmap
import os
import time

import numpy as np

from . import rds

GUNZIP_MAX_IN = 16 << 20            # the most compressed bytes one unit may take, as K29's
# Below this many compressed bytes a file is left to the host: the file size from which read_mtx of a MatrixMarket .gz, cut to
# prefixes of whole lines, stays ahead of its host route by more than the spread (21.1 MB on one MI355X,
# profiles/bench_gunzip.json; load_infercnv_obj crosses at 14.5 MB), rounded up to a power of two.  Under it the ~0.09 s of one
# lane walking a ~75 KiB unit twice (measure, symbols) sets the time.
GUNZIP_MIN_BYTES = 1 << 25
W = 32768
_STATUS = ("OK_BOUNDARY", "OK_FINAL", "TRUNCATED", "TOO_LONG", "BAD_STREAM")
_STATS = {"route": "none", "reason": "gunzip has not run"}


class _DeviceGunzip(rds._DeviceBytes):
    """The device side of gunzip: host arrays are numpy; src, sym and out stay on the device.  upload, crc32_pieces and stream
    are the shared base's, as K29's."""

    def available(self):
        import torch
        return torch.cuda.is_available()

    def free_bytes(self):
        import torch
        return int(torch.cuda.mem_get_info()[0])

    def _up(self, src, a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(src.device)

    def find(self, src):
        from . import device as dev
        return dev.gunzip_find(src).cpu().numpy()

    def measure(self, src, cand, start, max_in):
        from . import device as dev
        end, out_len, status = dev.gunzip_measure(src, self._up(src, cand), self._up(src, start), max_in)
        return end.cpu().numpy(), out_len.cpu().numpy(), status.cpu().numpy()

    def symbols(self, src, cand, start, end, out_off, out_len, total):
        import torch
        from . import device as dev
        sym = torch.empty(total, dtype=torch.int16, device=src.device)
        up = lambda a: self._up(src, a)
        return sym, dev.gunzip_symbols(src, up(cand), up(start), up(end), up(out_off), up(out_len), sym).cpu().numpy()

    def tails(self, sym, out_off, out_len, total):
        import torch
        from . import device as dev
        out = torch.empty(total, dtype=torch.uint8, device=sym.device)
        bad, markers = dev.gunzip_tails(sym, self._up(sym, out_off), self._up(sym, out_len), out)
        return out, int(bad.item()), int(markers.item())

    def resolve(self, sym, out_off, out_len, out):
        from . import device as dev
        return int(dev.gunzip_resolve(sym, self._up(sym, out_off), self._up(sym, out_len), out).item())


def _backend():
    return _DeviceGunzip()


def enabled():
    """ICNV_GUNZIP=0 switches this route off alone, ICNV_INFLATE=0 together with K29 (environment, read per call)."""
    return os.environ.get("ICNV_GUNZIP", "1").strip() != "0" and os.environ.get("ICNV_INFLATE", "1").strip() != "0"


def gunzip_stats():
    """What the latest gunzip() did: route ("device", or "host" with the reason it gave up), candidates, chain_units,
    false_candidates, units_short (chain units of fewer than 32 768 bytes), markers_tail (markers the sequential pass
    resolved), compressed_bytes, inflated_bytes, and seconds per phase (upload, find, measure, chain, symbols, tails, resolve,
    crc)."""
    return dict(_STATS, seconds=dict(_STATS.get("seconds", {})))


def gunzip(data, *, max_in=GUNZIP_MAX_IN):
    """The inflated stream of a one-member gzip file written by any deflater, as a CUDA uint8 tensor, or None.  data: bytes, an
    mmap or a path.  Never raises for a file's content: None, with gunzip_stats()["reason"], for a header that is not one
    deflate member's; a file below GUNZIP_MIN_BYTES; fewer than 2 chain units (a fixed- or stored-only stream, or one block:
    nothing to gain); any unit status other than OK; a chain that does not end with BFINAL exactly 8 bytes before the end (a
    second member, bgzip); an ISIZE or CRC-32 mismatch; a marker that points in front of the stream's first byte; a file whose
    compressed + 3 x inflated bytes exceed half of the free device memory; ICNV_GUNZIP=0 or ICNV_INFLATE=0; no GPU.  The caller
    then takes the host route, which succeeds or raises as it always did."""
    return _run(_backend(), data, max_in)


def _run(be, data, max_in):
    global _STATS
    st = {"route": "host", "reason": "", "candidates": 0, "chain_units": 0, "false_candidates": 0, "units_short": 0, "markers_tail": 0,
          "compressed_bytes": 0, "inflated_bytes": 0, "seconds": {}}
    _STATS = st
    if not enabled():
        st["reason"] = "switched off by ICNV_GUNZIP=0 or ICNV_INFLATE=0"
        return None
    if not be.available():
        st["reason"] = "no GPU"
        return None
    out = _gunzip_with(be, data, int(max_in), st)
    if out is not None:
        st["route"] = "device"
    return out


def _gunzip_with(be, data, max_in, st):
    if not isinstance(data, (str, os.PathLike)):
        return _gunzip(be, data, max_in, st)
    with open(data, "rb") as fh:
        if not os.fstat(fh.fileno()).st_size:
            return _gunzip(be, b"", max_in, st)
        mapped = mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ)
    try:
        return _gunzip(be, mapped, max_in, st)
    finally:
        try:
            mapped.close()
        except BufferError:                                   # a view of it is still alive: it closes when that goes
            pass


def _gunzip(be, data, max_in, st):
    def give_up(reason):
        st["reason"] = reason
        return None

    clock = time.perf_counter
    view = memoryview(data)
    st["compressed_bytes"] = len(view)
    head = rds.gzip_header_length(view)
    if head is None:
        return give_up("not a gzip header")
    if len(view) < GUNZIP_MIN_BYTES:
        return give_up(f"below GUNZIP_MIN_BYTES ({GUNZIP_MIN_BYTES})")
    n = len(view) - head - 8                                  # the raw stream
    if n < 3:
        return give_up("truncated file")
    if n > be.free_bytes() // 2:                              # before the first allocation; the exact test follows the measure
        return give_up("the file does not fit: its compressed bytes exceed half of the free device memory")
    t0 = clock()
    src = be.upload(view[head:head + n])
    t1 = clock()
    cand = np.asarray(be.find(src), dtype=np.int64)
    t2 = clock()
    st["seconds"].update(upload=t1 - t0, find=t2 - t1)
    start = np.concatenate([np.zeros(1, dtype=np.int64), cand[cand > 0]])
    st["candidates"] = int(cand.size)
    if start.size < 2:
        return give_up("fewer than 2 units: nothing to gain")
    end, out_len, status = be.measure(src, cand, start, max_in)
    t3 = clock()
    chain, refused = rds._walk_chain(start, end, status, lambda i, s: f"the unit at bit {int(start[i])} " + (
        "does not end on a candidate" if s is None else f"has status {_STATUS[s]}"))
    if chain is None:
        return give_up(refused)
    st["seconds"].update(measure=t3 - t2, chain=clock() - t3)
    st["chain_units"], st["false_candidates"] = int(chain.size), int(start.size - chain.size)
    if int(end[chain[-1]]) != n * 8:
        return give_up("the stream is not followed by exactly the 8-byte trailer (a second member?)")
    if chain.size < 2:
        return give_up("fewer than 2 units: nothing to gain")
    c_start, c_end, c_len = start[chain], end[chain], out_len[chain]
    c_off = np.cumsum(c_len) - c_len
    total = int(c_len.sum())
    st["units_short"] = int((c_len < W).sum())
    if not rds._isize_matches(view, total):
        return give_up("the trailer's ISIZE does not match")
    st["inflated_bytes"] = total
    if n + 3 * total > be.free_bytes() // 2:
        return give_up("the file does not fit: compressed + 3 x inflated bytes exceed half of the free device memory")
    t4 = clock()
    sym, got = be.symbols(src, cand, c_start, c_end, c_off, c_len, total)
    t5 = clock()
    if not np.array_equal(got, status[chain]):
        return give_up("the symbols disagree with the measure")
    out, bad, st["markers_tail"] = be.tails(sym, c_off, c_len, total)
    t6 = clock()
    bad |= be.resolve(sym, c_off, c_len, out)
    t7 = clock()
    st["seconds"].update(symbols=t5 - t4, tails=t6 - t5, resolve=t7 - t6)
    if bad:
        return give_up("a match refers in front of the stream's first byte")
    crc_ok = rds._crc32_matches(view, be, out, total)
    st["seconds"].update(crc=clock() - t7)
    if not crc_ok:
        return give_up("the trailer's CRC-32 does not match")
    return out


def open_on_device(path):
    """(tensor, stream) of a gzip file that gunzip takes -- the CUDA uint8 tensor and K29's _DeviceStream over it -- or None."""
    if not enabled():                                         # (the consumers' switch: gunzip() is not even called)
        return None
    be = _backend()
    out = _run(be, path, GUNZIP_MAX_IN)
    return None if out is None else (out, be.stream(out))
