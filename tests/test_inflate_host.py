"""K29 without a GPU: the RFC 1951 restatement of tests/inflate_restate.py against zlib, its statuses on the malformed streams,
rds.inflate_gzip's chain walk and every one of its fallback decisions with the restatement standing in for the four device calls
(as test_assembler_with_the_host_stand_in does for the compressor), and the reader's window over a device-resident stream."""
import gzip
import struct
import zlib

import numpy as np
import pytest

import deflate_restate as dr
import inflate_restate as ir
from infercnv_amd import rds
from test_deflate_host import objects, stand_in

VARIANTS = [f"level_{l}" for l in ir.LEVELS] + list(ir.STRATEGIES)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("piece", [256, 16384])
def test_restatement_equals_zlib(piece, variant):
    for name, data in dr.payloads(piece).items():
        pieces = ir.zlib_variants(data, piece)[variant]
        assert len(pieces) == -(-len(data) // piece)
        for i, comp in enumerate(pieces):
            want = zlib.decompressobj(-15).decompress(comp)
            assert want == data[i * piece:(i + 1) * piece]
            status, end, out_len, got = ir.unit_cached(comp)
            assert (status, end, out_len) == (ir.OK_MARKER, len(comp), len(want)), (name, i)
            assert got == want, (name, i)
        packed = b"".join(pieces) + dr.FINAL_BLOCK                           # the pieces as one chain, closed by a final block
        walked = ir.chain(packed)
        assert [u[0] for u in walked] == list(np.cumsum([0] + [len(p) for p in pieces]))
        assert walked[-1][1] == ir.OK_FINAL and walked[-1][2] == len(packed) and b"".join(u[4] for u in walked) == data


def test_hand_built_units():
    for name, (stream, data, status) in ir.hand_units().items():
        assert ir.unit(stream + b"\x55\xaa") [:3] == (status, len(stream), len(data)), name      # bytes behind the unit are not looked at
        assert ir.unit(stream)[3] == data, name
        d = zlib.decompressobj(-15)
        assert d.decompress(stream + (b"" if status == ir.OK_FINAL else dr.FINAL_BLOCK)) == data and d.eof, name
    comp, data = ir.long_unit()
    assert ir.unit(comp) ==(ir.OK_MARKER, len(comp), len(data), data) and len(data) > 190_000
    assert ir.unit(b"\x00" * 3 + comp + b"\x00", 3)[:3] == (ir.OK_MARKER, 3 + len(comp), len(data))   # an odd start


def test_malformed_statuses():
    for name, (stream, status) in ir.malformed().items():
        assert ir.unit(stream)[0] == status, name
        if status == ir.BAD_STREAM:                                          # zlib refuses every one of them as well
            with pytest.raises(zlib.error):
                zlib.decompressobj(-15).decompress(stream + bytes(300))
    comp, data = ir.sample_dynamic()
    head = ir.dynamic_header_bytes(comp)
    assert 10 < head < len(comp) - 8
    for cut in list(range(head + 1)) + [head + 3, (head + len(comp)) // 2, len(comp) - 1]:
        assert ir.unit(comp[:cut])[0] == ir.TRUNCATED, cut
    assert ir.unit(comp + b"more", 0, len(comp) - 1)[0] == ir.TOO_LONG
    assert ir.unit(comp + b"more", 0, len(comp))[:3] == (ir.OK_MARKER, len(comp), len(data))
    stream = ir.sync_flush_stream([b"first part " * 30, b"first part again " * 10])
    first = ir.unit(stream)
    assert first[0] == ir.OK_MARKER and ir.unit(stream, first[1])[0] == ir.NEEDS_HISTORY


# ---- inflate_gzip with the stand-in --------------------------------------------------------------------------------------------------------
@pytest.fixture
def host(monkeypatch):
    be = ir.HostInflate()
    monkeypatch.setattr(rds, "_inflate_backend", lambda: be)
    monkeypatch.setattr(rds, "_device_available", lambda: True)
    monkeypatch.delenv("ICNV_INFLATE", raising=False)
    return be


def payload_list(k):
    return [dr.count_like(700, 50), dr.random_bytes(1000, 51), dr.denoised_like(300, 52)][:k]


@pytest.mark.parametrize("k", [0, 1, 3])
def test_assembled_files(host, k):
    blob, plain = ir.assembled_file(payload_list(k))
    assert gzip.decompress(blob) == plain
    out = rds.inflate_gzip(blob)
    stats = rds.inflate_stats()
    if k == 0:                                                               # one zlib stream, one unit: nothing to gain, the host's
        assert out is None and "no flush points" in stats["reason"] and not stats["decode_launched"] and host.calls["units"] == 0
        return
    assert out is not None and out.tobytes() == plain
    pieces = sum(-(-len(p) // 256) for p in payload_list(k))
    assert stats["route"] == "device" and stats["decode_launched"] and stats["inflated_bytes"] == len(plain)
    assert stats["chain_units"] == pieces + k + 1                            # the pieces, a host part ahead of every payload, the last part
    assert stats["candidates"] == stats["chain_units"] + stats["false_candidates"] and stats["compressed_bytes"] == len(blob)
    assert set(stats["seconds"]) == {"upload", "scan", "measure", "chain", "decode", "crc"}
    assert host.calls == {"scan": 1, "measure": 1, "units": 1, "crc": 1}
    assert rds.inflate_gzip(memoryview(blob)).tobytes() == plain


def test_a_false_candidate_that_decodes_is_not_on_the_chain(host):
    small = ir.end_marker(ir.fixed_block(ir.BitWriter(), [1, 2, 3, (5, 2)])).bytes()
    assert ir.unit(small)[0] == ir.OK_MARKER
    payload = dr.random_bytes(20, 53) + ir.MARKER + small + dr.random_bytes(150, 54)    # inside one stored piece of 256
    blob, plain = ir.assembled_file([payload, dr.count_like(100, 55)], level=0)
    out = rds.inflate_gzip(blob)
    stats = rds.inflate_stats()
    assert out is not None and out.tobytes() == plain
    starts, got = host.measured
    at = bytes(blob[10:]).find(ir.MARKER + small) + 4
    i = int(np.searchsorted(starts, at))
    assert starts[i] == at and got[i][0] == ir.OK_MARKER                     # it measures as a valid unit ...
    assert stats["false_candidates"] >= 2 and stats["chain_units"] + stats["false_candidates"] == len(starts)   # ... and is walked past


def test_files_that_are_turned_away(host, tmp_path):
    blob, plain = ir.assembled_file(payload_list(3))
    raw = blob[10:-8]

    def refused(data, words, units=0, **kw):
        before = host.calls["units"]
        assert rds.inflate_gzip(data, **kw) is None
        stats = rds.inflate_stats()
        assert stats["route"] == "host" and words in stats["reason"], stats["reason"]
        assert host.calls["units"] - before == units and stats["decode_launched"] == bool(units)

    # no flush points: R's own files, Python's GzipFile
    r_like = ir.gzipfile_bytes(plain)
    assert gzip.decompress(r_like) == plain
    measures = host.calls["measure"]
    refused(r_like, "no flush points", max_in=1024)                          # fewer candidates than bytes / max_in: not even measured
    assert host.calls["measure"] == measures
    refused(r_like, "no flush points")                                       # one unit that fits max_in: still the host's
    # a later unit refers back into an earlier one
    parts = [b"first part " * 30, b"first part again " * 10, b"and a third " * 5]
    refused(ir.gzip_member(ir.sync_flush_stream(parts), b"".join(parts)), "NEEDS_HISTORY")
    # two members, garbage behind the trailer, a truncated file
    refused(blob + blob, "8-byte trailer")
    refused(blob + b"\x00", "8-byte trailer")
    refused(blob[:-1], "")
    refused(blob[:len(blob) // 2], "")
    refused(blob[:14], "")
    refused(b"", "not a gzip header")
    refused(b"BZh91AY" + blob, "not a gzip header")
    # max_in below the longest unit
    refused(blob, "", max_in=64)
    # the trailer
    crc, isize = struct.unpack("<II", blob[-8:])
    refused(blob[:-8] + struct.pack("<II", crc ^ 1, isize), "CRC-32", units=1)
    refused(blob[:-8] + struct.pack("<II", crc, isize ^ 1), "ISIZE")
    # a header with FNAME (Python's GzipFile), FEXTRA, FCOMMENT and FHCRC round the same stream is stepped over
    named = ir.gzipfile_bytes(b"")
    head = named[:rds.gzip_header_length(named)]
    assert head[3] == 8 and head.endswith(b"object.rds\x00")
    assert rds.inflate_gzip(ir.gzip_member(raw, plain, header=head)).tobytes() == plain
    full = b"\x1f\x8b\x08\x1e" + bytes(6) + struct.pack("<H", 5) + b"extra" + b"name\x00" + b"a comment\x00" + b"\x12\x34"
    assert rds.gzip_header_length(full + b"x") == len(full)
    assert rds.inflate_gzip(ir.gzip_member(raw, plain, header=full)).tobytes() == plain
    assert rds.gzip_header_length(full[:-3]) is None and rds.gzip_header_length(b"\x1f\x8b\x08\x20" + bytes(6)) is None
    # a path
    (tmp_path / "a.gz").write_bytes(blob)
    assert rds.inflate_gzip(tmp_path / "a.gz").tobytes() == plain


def same_value(a, b):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b)
        for k in a:
            same_value(a[k], b[k])
    elif isinstance(a, list):
        assert isinstance(b, list) and len(a) == len(b)
        for x, y in zip(a, b):
            same_value(x, y)
    elif isinstance(a, rds.RValue):
        assert isinstance(b, rds.RValue)
        same_value(a.value, b.value)
        same_value(a.attrs, b.attrs)
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape
        assert a.tobytes() == b.tobytes() if a.dtype.kind in "fiub" else a.tolist() == b.tolist()
    else:
        assert a == b


@pytest.mark.parametrize("name", ["no_payload", "one_payload", "three_payloads"])
def test_read_rds_through_the_window(host, tmp_path, monkeypatch, name):
    """read_rds(return_device=True) over the stream where inflate_gzip left it: every value equals the plain file's, with
    windows far smaller than the payloads, so that reads straddle their edges."""
    value = objects()[name]
    rds.write_rds(value, tmp_path / "plain.rds", device=False)
    monkeypatch.setattr(rds, "_stream_payload", stand_in)                    # the K28 writer's host stand-in
    monkeypatch.setattr(rds, "DEVICE_THRESHOLD", 20_000)
    monkeypatch.setattr(rds, "CHUNK_BYTES", 40_000)
    rds.write_rds(value, tmp_path / "a.rds.gz", compress=True)
    monkeypatch.setattr(rds, "DEVICE_THRESHOLD", 1 << 40)                    # (no GPU here: the payloads are decoded by NumPy)
    want = rds.read_rds(tmp_path / "plain.rds")
    for window in (4 << 20, 1000, 37):
        monkeypatch.setattr(rds, "WINDOW_BYTES", window)
        units = host.calls["units"]
        got = rds.read_rds(tmp_path / "a.rds.gz", return_device=True)
        same_value(want, got)
        assert host.calls["units"] - units == (0 if name == "no_payload" else 1)
        assert rds.inflate_stats()["route"] == ("host" if name == "no_payload" else "device")
    monkeypatch.setenv("ICNV_INFLATE", "0")
    units = host.calls["units"]
    same_value(want, rds.read_rds(tmp_path / "a.rds.gz", return_device=True))
    assert host.calls["units"] == units
    monkeypatch.delenv("ICNV_INFLATE")
    same_value(want, rds.read_rds(tmp_path / "a.rds.gz"))                    # return_device=False: the host route, not asked
    assert host.calls["units"] == units


def test_window_buffer():
    data = dr.random_bytes(5000, 56)
    fetched = []

    def fetch(lo, hi):
        fetched.append((lo, hi))
        return data[lo:hi]

    for window in (16, 100, 1 << 20):
        rds_window = rds.WINDOW_BYTES
        try:
            rds.WINDOW_BYTES = window
            buf = rds._DeviceStream(fetch, len(data))
            assert len(buf) == len(data) and bytes(buf[:5]) == data[:5]
            for pos in (0, 1, 13, 14, 15, 16, 17, 99, 100, 4996):           # ints that straddle the edges of windows of 16 and 100
                assert buf.int_at(pos) == struct.unpack_from(">i", data, pos)[0]
            for lo, hi in ((0, 0), (3, 3), (7, 23), (95, 105), (1, 4001), (4990, 5000), (4990, 6000)):
                assert bytes(buf[lo:hi]) == data[lo:min(hi, 5000)]
            odd = np.frombuffer(buf[1001:1001 + 8 * 300], dtype=">f8", count=300)      # a payload at an odd offset
            assert odd.tobytes() == data[1001:1001 + 2400]
            assert all(0 <= lo <= hi <= len(data) for lo, hi in fetched)
        finally:
            rds.WINDOW_BYTES = rds_window
