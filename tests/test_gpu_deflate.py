"""K28 on the GPU (-m gpu): icnv_deflate_pieces_dev / icnv_deflate_pack_dev under zlib's inflate -- the code R's gzfile runs --
on the payloads of tests/deflate_restate.py at both ends of the allowed piece size: every piece alone, the guard bytes round
every slot, the CRCs, the packed stream, the refusals, determinism, the size caps; and save_infercnv_obj(compress=True) end to
end against the uncompressed file."""
import ctypes as ct
import gzip
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import deflate_restate as dr  # noqa: E402
from test_gpu_rds import object_257x129  # noqa: E402
from test_rds_host import assert_same_object  # noqa: E402

GUARD = 16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infercnv_amd import device
    torch.cuda.set_device(0)
    device.init(0)
    return device


def run_pieces(dev, data, piece, offset=0):
    """(pieces, crcs, packed, dst, piece_len): data compressed from a src view `offset` bytes into its buffer, into slots with
    GUARD bytes of 0xA5 on either side, which must come back untouched."""
    buf = torch.zeros(len(data) + offset + 8, dtype=torch.uint8, device="cuda")
    buf[offset:offset + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    src = buf[offset:offset + len(data)]
    n_pieces, bound = -(-len(data) // piece), dev.deflate_bound(piece)
    slab = torch.full((n_pieces, bound + 2 * GUARD), 0xA5, dtype=torch.uint8, device="cuda")
    dst, piece_len, piece_crc = dev.deflate_pieces(src, piece, dst=slab[:, GUARD:GUARD + bound])
    packed = dev.deflate_pack(dst, piece_len)
    torch.cuda.synchronize()
    host, lens = slab.cpu().numpy(), piece_len.cpu().numpy()
    crcs = piece_crc.cpu().numpy().view(np.uint32)
    assert (host[:, :GUARD] == 0xA5).all() and (host[:, GUARD + bound:] == 0xA5).all(), "a store outside a slot"
    assert lens.size == n_pieces and (lens >= 6).all() and (lens <= bound).all()
    pieces = [host[i, GUARD:GUARD + int(lens[i])].tobytes() for i in range(n_pieces)]
    return pieces, crcs, packed.cpu().numpy().tobytes(), dst, piece_len


PAYLOAD_NAMES = list(dr.payloads(256))


@pytest.mark.parametrize("end", ["max", "min"])
@pytest.mark.parametrize("name", PAYLOAD_NAMES)
def test_every_piece_under_zlib(dev, name, end):
    piece = dev.DEFLATE_PIECE_MAX if end == "max" else dev.DEFLATE_PIECE_MIN
    assert dev.DEFLATE_PIECE == dev.DEFLATE_PIECE_MAX
    data = dr.payloads(piece)[name]
    pieces, crcs, packed, _, _ = run_pieces(dev, data, piece)
    for i, comp in enumerate(pieces):
        dr.check_piece(comp, data[i * piece:(i + 1) * piece], int(crcs[i]), dev.deflate_bound(piece), f"{name}[{i}]")
    assert packed == b"".join(pieces)
    dr.check_stream(packed, data)
    whole = dev.crc32_combine_pieces(crcs, piece, len(data) - (len(pieces) - 1) * piece)
    assert whole == zlib.crc32(data)


def test_compressible_payloads_are_not_stored(dev):
    """The stored fallback is for incompressible data only: zeros, a repeated double and the state-like stream come out as
    Huffman-coded pieces (smaller than stored), random bytes as stored ones of exactly input + 5 bytes."""
    piece = dev.DEFLATE_PIECE
    for name in ("zeros", "one_double", "state_like", "one_byte_value", "fibonacci"):
        data = dr.payloads(piece)[name]
        pieces, _, _, _, _ = run_pieces(dev, data, piece)
        full = [p for i, p in enumerate(pieces) if len(data[i * piece:(i + 1) * piece]) == piece]
        assert full and all(len(p) < piece // 2 for p in full), name
        assert all(p[0] & 7 == 4 for p in full), name                       # BFINAL 0, BTYPE 10
    data = dr.random_bytes(3 * piece, 41)
    pieces, _, _, _, _ = run_pieces(dev, data, piece)
    assert [len(p) for p in pieces] == [piece + 5] * 3 and all(p[:1] == b"\x00" for p in pieces)


def test_pack_refuses_a_short_buffer(dev):
    from infercnv_amd._lib import ERR_ARG, IcnvError
    data = dr.count_like(3 * dev.DEFLATE_PIECE // 8 + 1)
    _, _, packed, dst, piece_len = run_pieces(dev, data, dev.DEFLATE_PIECE)
    out = torch.full((len(packed) + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    with pytest.raises(IcnvError) as err:
        dev.deflate_pack(dst, piece_len, out=out, out_cap=len(packed) - 1)
    assert err.value.code == ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all())                                        # nothing was written, before or past out_cap
    got = dev.deflate_pack(dst, piece_len, out=out, out_cap=len(packed))    # the exact size is enough
    assert got.cpu().numpy().tobytes() == packed and bool((out[len(packed):] == 0x5A).all())


def test_refusals_before_any_launch(dev):
    from infercnv_amd import _lib
    L = _lib.load()
    assert L.icnv_deflate_bound(255) == -1 and L.icnv_deflate_bound(16385) == -1
    assert L.icnv_deflate_bound(256) == 261 and L.icnv_deflate_bound(16384) == 16389 == dev.deflate_bound(16384)
    for bad in (255, 16385, 0, -1):
        with pytest.raises(ValueError):
            dev.deflate_bound(bad)
    src = torch.zeros(1000, dtype=torch.uint8, device="cuda")
    dst = torch.full((4, 300), 0xA5, dtype=torch.uint8, device="cuda")
    lens = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    crcs = torch.zeros(4, dtype=torch.int32, device="cuda")
    p = lambda t: ct.c_void_p(t.data_ptr())
    call = lambda n, piece, stride: L.icnv_deflate_pieces_dev(p(src), n, piece, p(dst), stride, p(lens), p(crcs), None)
    assert call(1000, 255, 300) == _lib.ERR_ARG and call(1000, 16385, 16390) == _lib.ERR_ARG      # piece_bytes outside the range
    assert call(1000, 256, 260) == _lib.ERR_ARG                                                    # dst_stride below the bound
    assert call(-1, 256, 300) == _lib.ERR_ARG
    total = ct.c_int64(-1)
    assert L.icnv_deflate_pack_dev(p(dst), 0, p(lens), 4, p(dst), 100, ct.byref(total), None) == _lib.ERR_ARG
    torch.cuda.synchronize()
    assert bool((dst == 0xA5).all()) and bool((lens == -1).all())
    assert call(0, 256, 300) == _lib.OK                                                            # an empty call
    got = dev.deflate_pieces(src[:0])
    assert got[0].shape[0] == 0 and got[1].numel() == 0 and dev.deflate_pack(got[0], got[1]).numel() == 0


def test_two_runs_and_an_odd_offset_give_the_same_bytes(dev):
    piece = dev.DEFLATE_PIECE
    data = dr.denoised_like(2 * piece // 8 + 11) + dr.count_like(piece // 8) + dr.random_bytes(777, 42)
    first = run_pieces(dev, data, piece)
    again = run_pieces(dev, data, piece)
    odd = run_pieces(dev, data, piece, offset=3)                            # byte loads instead of dword loads
    for other in (again, odd):
        assert other[0] == first[0] and np.array_equal(other[1], first[1]) and other[2] == first[2]
    dr.check_stream(first[2], data)


@pytest.mark.parametrize("kind", ["state_like", "count_like", "denoised_like"])
def test_size_against_zlib_level_1(dev, kind):
    """A cap that keeps a build without its matcher or its dynamic tables from passing: 1.5 x zlib level 1 on the whole stream
    (zlib level 1 in independent 64 KiB pieces stays within 1.08 x)."""
    data = getattr(dr, kind)(1 << 17)                                       # 1 MiB: 64 pieces
    _, _, packed, _, _ = run_pieces(dev, data, dev.DEFLATE_PIECE)
    dr.check_stream(packed, data)
    ref = len(zlib.compress(data, 1))
    print(f"{kind}: packed {len(packed)}, zlib level 1 {ref}, ratio {len(packed) / ref:.3f}, of the input {len(packed) / len(data):.4f}")
    assert len(packed) <= 1.5 * ref


def test_random_bytes_do_not_grow(dev):
    data = dr.random_bytes(1 << 20, 43)
    _, _, packed, _, _ = run_pieces(dev, data, dev.DEFLATE_PIECE)
    print(f"random bytes: packed {len(packed)} of {len(data)}")
    assert len(packed) <= 1.001 * len(data)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def compressible_object(sparse):
    obj = object_257x129()
    x = obj.expr_data.copy()
    x[np.abs(x) < 1.2] = 1.0                                                # a denoised-like matrix (the special values stay)
    obj.expr_data = x
    if sparse:
        import scipy.sparse as sp
        obj.count_data = sp.csc_matrix(np.random.default_rng(6).poisson(0.15, size=x.shape).astype(np.float64))
    return obj


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("source", ["host", "x_dev"])
def test_save_infercnv_obj_compressed(dev, tmp_path, monkeypatch, sparse, source):
    from infercnv_amd import load_infercnv_obj, rds, save_infercnv_obj
    obj = compressible_object(sparse)
    save_infercnv_obj(obj, tmp_path / "plain.rds", device=False)
    plain = (tmp_path / "plain.rds").read_bytes()
    monkeypatch.setattr(rds, "DEVICE_THRESHOLD", 0)                         # every numeric payload: pieces of a few bytes too
    monkeypatch.setattr(rds, "CHUNK_BYTES", 40_000)                         # 265 KB of expr.data: seven chunks, cut inside columns
    given, kwargs = obj, {}
    if source == "x_dev":
        given = obj.copy()
        given.expr_data = None
        kwargs["x_dev"] = torch.from_numpy(np.ascontiguousarray(obj.expr_data.T)).cuda()
    stats = save_infercnv_obj(given, tmp_path / "dev.rds.gz", compress=True, **kwargs)
    blob = (tmp_path / "dev.rds.gz").read_bytes()
    assert blob[:10] == rds.GZIP_HEADER and gzip.decompress(blob) == plain
    _, stream, crc, isize = dr.gzip_parts(blob)
    assert crc == zlib.crc32(plain) and isize == len(plain)
    d = zlib.decompressobj(-15)                                             # one member, one raw stream
    assert d.decompress(stream) == plain and d.eof and d.unused_data == b""
    assert_same_object(obj, load_infercnv_obj(tmp_path / "dev.rds.gz"))
    assert max(s["chunks"] for s in stats) >= 7
    raw, comp, pieces = (sum(s[k] for s in stats) for k in ("raw_bytes", "compressed_bytes", "pieces"))
    assert pieces > 0 and comp < raw and all(s["deflate_s"] > 0 and 0 <= s["stored_pieces"] <= s["pieces"] for s in stats)
    assert len(blob) < len(plain) // 2
    save_infercnv_obj(given, tmp_path / "again.rds.gz", compress=True, **kwargs)
    assert (tmp_path / "again.rds.gz").read_bytes() == blob                 # reproducible
    monkeypatch.setenv("ICNV_DEFLATE", "0")                                 # the old route: GzipFile round the device's bytes
    old = save_infercnv_obj(given, tmp_path / "old.rds.gz", compress=True, **kwargs)
    assert gzip.decompress((tmp_path / "old.rds.gz").read_bytes()) == plain and all("pieces" not in s for s in old)
    assert (tmp_path / "old.rds.gz").read_bytes()[:10] != rds.GZIP_HEADER
    monkeypatch.delenv("ICNV_DEFLATE")
    save_infercnv_obj(given, tmp_path / "plain_dev.rds", **kwargs)          # compress=False is what it was
    assert (tmp_path / "plain_dev.rds").read_bytes() == plain
