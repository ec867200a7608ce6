"""K28 on the host (-m "not gpu"): crc32_combine and its equal-length batch form against zlib.crc32; the gzip assembler of
rds.write_rds driven by a host stand-in for the device compressor (raw zlib with a Z_FULL_FLUSH per piece: pieces of the
contract's shape); rds_checkpoints(compress=True)."""
import gzip
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import deflate_restate as dr  # noqa: E402
from infercnv_amd import device, rds  # noqa: E402

SPLITS = (0, 1, 7, 8, 65535, 65536, 65537)


def test_crc32_combine_against_zlib():
    blob = dr.random_bytes(2 * 65537, 21)
    for la in SPLITS:
        for lb in SPLITS:
            a, b = blob[:la], blob[65537:65537 + lb]
            assert device.crc32_combine(zlib.crc32(a), zlib.crc32(b), lb) == zlib.crc32(a + b), (la, lb)


def zeros_crc(n):
    """CRC-32 of n zero bytes by formula: the register 0xFFFFFFFF moved across n bytes, then the final xor."""
    return device._crc_mul(device.crc32_shift_operator(n), 0xFFFFFFFF) ^ 0xFFFFFFFF


def test_crc32_combine_beyond_2_to_32():
    assert all(zeros_crc(n) == zlib.crc32(bytes(n)) for n in (0, 1, 9, 65536, 1 << 20))     # the formula itself
    op = device.crc32_shift_operator(65536)                  # x^(8 * 2^32) by sixteen squarings of an operator zlib confirmed
    assert device._crc_mul(op, zlib.crc32(b"abc")) ^ zlib.crc32(bytes(65536)) == zlib.crc32(b"abc" + bytes(65536))
    for _ in range(16):
        op = device._crc_mul(op, op)
    big = (1 << 32) + 12345
    assert device.crc32_shift_operator(1 << 32) == op
    assert device.crc32_shift_operator(big) == device._crc_mul(op, device.crc32_shift_operator(12345))
    a = dr.random_bytes(1000, 22)
    want = device._crc_mul(device.crc32_shift_operator(big), zlib.crc32(a)) ^ zeros_crc(big)
    assert device.crc32_combine(zlib.crc32(a), zeros_crc(big), big) == want
    # the same split in two steps of less than 2^32 each, and the all-zero stream against the formula
    half = big // 2
    two_steps = device.crc32_combine(device.crc32_combine(zlib.crc32(a), zeros_crc(half), half), zeros_crc(big - half), big - half)
    assert two_steps == want
    assert device.crc32_combine(zeros_crc(777), zeros_crc(big), big) == zeros_crc(big + 777)


@pytest.mark.parametrize("count", [0, 1, 2, 3, 5, 8, 1000])
def test_crc32_combine_pieces_against_the_pairwise_fold(count):
    piece, last = 256, 100
    data = dr.random_bytes(max(count - 1, 0) * piece + (last if count else 0), 23)
    crcs = [zlib.crc32(data[o:o + piece]) for o in range(0, len(data), piece)]
    assert len(crcs) == count
    fold = 0
    for i, c in enumerate(crcs):
        fold = device.crc32_combine(fold, c, last if i == count - 1 else piece)
    got = device.crc32_combine_pieces(crcs, piece, last)
    assert got == fold == zlib.crc32(data)
    as_int32 = np.array(crcs, dtype=np.uint32).view(np.int32)            # the bit patterns the device hands back
    assert device.crc32_combine_pieces(as_int32, piece, last) == got
    if count:
        whole = dr.random_bytes(count * piece, 24)
        assert device.crc32_combine_pieces([zlib.crc32(whole[o:o + piece]) for o in range(0, len(whole), piece)], piece) == zlib.crc32(whole)


# ---- the assembler ---------------------------------------------------------------------------------------------------------------
def stand_in(w, v, cuda, n, es):
    """rds._stream_payload with the device replaced: NumPy's big-endian column-major bytes, cut into chunks as the device
    route cuts them, every chunk compressed by dr.host_pieces."""
    assert isinstance(w.f, rds.GzipAssembler) and not cuda
    w.flush()
    data = np.asarray(v).astype(v.dtype.newbyteorder(">")).tobytes(order="F" if v.ndim == 2 else "C")
    assert len(data) == n * es
    per_chunk = max(1, min(rds.CHUNK_BYTES, -(-n * es // 16) * 16) // es) * es
    raw = w.f.begin_payload()
    stats = {"chunks": 0, "pieces": 0}
    for o in range(0, len(data), per_chunk):
        pieces = dr.host_pieces(data[o:o + per_chunk], device.DEFLATE_PIECE)
        packed = b"".join(p[0] for p in pieces)
        raw.write(packed)
        w.f.add_pieces([p[1] for p in pieces], device.DEFLATE_PIECE, min(per_chunk, len(data) - o), len(packed))
        stats["chunks"] += 1
        stats["pieces"] += len(pieces)
    return stats


def objects():
    rng = np.random.default_rng(31)
    names = np.array([f"gene_{i}" for i in range(300)], dtype=object)
    big_a = np.round(rng.normal(1, 0.05, size=(300, 41)), 2)
    big_b = rng.poisson(0.15, size=20_000).astype(np.int32)
    big_c = rng.normal(size=(70, 333))
    return {
        "no_payload": {"a": np.arange(5), "names": names, "s": "text"},
        "one_payload": {"a": np.arange(5), "m": rds.RValue(big_a, {"dimnames": [names, None]}), "tail": [1.5, "x", None]},
        "three_payloads": {"m": big_a, "between": names, "counts": big_b, "more": {"k": np.arange(7.0)}, "last": big_c, "end": True},
    }


@pytest.mark.parametrize("name", ["no_payload", "one_payload", "three_payloads"])
def test_assembler_with_the_host_stand_in(tmp_path, monkeypatch, name):
    value = objects()[name]
    rds.write_rds(value, tmp_path / "plain.rds", device=False)
    plain = (tmp_path / "plain.rds").read_bytes()
    monkeypatch.setattr(rds, "_device_available", lambda: True)
    monkeypatch.setattr(rds, "_stream_payload", stand_in)
    monkeypatch.setattr(rds, "DEVICE_THRESHOLD", 20_000)
    monkeypatch.setattr(rds, "CHUNK_BYTES", 40_000)
    stats = rds.write_rds(value, tmp_path / "a.rds.gz", compress=True)
    assert len(stats) == {"no_payload": 0, "one_payload": 1, "three_payloads": 3}[name]
    if stats:
        assert max(s["chunks"] for s in stats) >= 2 and max(s["pieces"] for s in stats) >= 6
    blob = (tmp_path / "a.rds.gz").read_bytes()
    assert gzip.decompress(blob) == plain
    header, stream, crc, isize = dr.gzip_parts(blob)
    assert header == b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff"             # deflate, no flags, mtime 0, XFL 0, OS unknown
    assert crc == zlib.crc32(plain) and isize == len(plain)
    d = zlib.decompressobj(-15)                                              # ONE raw stream that ends where the trailer begins
    assert d.decompress(stream) == plain and d.eof and d.unused_data == b""
    rds.write_rds(value, tmp_path / "b.rds.gz", compress=True)
    assert (tmp_path / "b.rds.gz").read_bytes() == blob                      # reproducible
    assert rds.read_rds(tmp_path / "a.rds.gz") is not None

    # the routes that stay as they were: device=False and ICNV_DEFLATE=0 go through GzipFile, compress=False is untouched
    monkeypatch.setattr(rds, "_stream_payload", lambda *a: pytest.fail("the device route was taken"))
    monkeypatch.setattr(rds, "_device_available", lambda: False)
    rds.write_rds(value, tmp_path / "c.rds.gz", compress=True, device=False)
    assert gzip.decompress((tmp_path / "c.rds.gz").read_bytes()) == plain and (tmp_path / "c.rds.gz").read_bytes()[:10] != blob[:10]
    monkeypatch.setenv("ICNV_DEFLATE", "0")
    monkeypatch.setattr(rds, "_device_available", lambda: name == "no_payload")      # (with payloads GzipFile would need the device)
    rds.write_rds(value, tmp_path / "d.rds.gz", compress=True)
    assert gzip.decompress((tmp_path / "d.rds.gz").read_bytes()) == plain and (tmp_path / "d.rds.gz").read_bytes()[:10] != blob[:10]
    rds.write_rds(value, tmp_path / "e.rds")
    assert (tmp_path / "e.rds").read_bytes() == plain


def test_assembler_refuses_pieces_that_do_not_add_up(tmp_path):
    with open(tmp_path / "x.gz", "wb") as raw:
        gz = rds.GzipAssembler(raw)
        gz.begin_payload()
        with pytest.raises(ValueError):
            gz.add_pieces([1, 2], 256, 256, 10)              # two pieces hold more than 256 bytes
        with pytest.raises(ValueError):
            gz.add_pieces([1, 2], 256, 513, 10)


def test_rds_checkpoints_hands_compress_to_the_default_saver(tmp_path, monkeypatch):
    from infercnv_amd.pipeline import rds_checkpoints
    calls = []

    def recorder(obj, path, **kwargs):
        calls.append((obj, kwargs))
        with open(path, "w") as fh:
            fh.write(obj)

    monkeypatch.setattr(rds, "save_infercnv_obj", recorder)
    rds_checkpoints(str(tmp_path / "a"), compress=True)      # (the directory is only written to by the hook)
    (tmp_path / "a").mkdir()
    hook = rds_checkpoints(str(tmp_path / "a"), compress=True)
    hook(3, "label", "object of step 3")
    assert calls == [("object of step 3", {"compress": True})]
    (tmp_path / "b").mkdir()
    rds_checkpoints(str(tmp_path / "b"))(3, "label", "object of step 3")
    assert calls[-1] == ("object of step 3", {"compress": False})
    own = []
    rds_checkpoints(str(tmp_path / "b"), saver=lambda obj, path: (own.append(obj), open(path, "w").close()), compress=True)(3, "l", "o")
    assert own == ["o"] and len(calls) == 2                  # ignored when a saver is given
