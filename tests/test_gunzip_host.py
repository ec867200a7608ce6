"""K30 on the host: the sequential restatement of tests/gunzip_restate.py against zlib -- zlib's own streams at small
memLevels, the hand-built units, the committed .gz fixtures -- and gunzip.gunzip's chain walk and every way of being turned
away over the HostGunzip stand-in.  No GPU and no library call."""
import os
import struct
import zlib

import numpy as np
import pytest

import gunzip_restate as gr
import inflate_restate as ir
from infercnv_amd import gunzip


@pytest.fixture
def stand_in(monkeypatch):
    be = gr.HostGunzip()
    monkeypatch.setattr(gunzip, "_backend", lambda: be)
    monkeypatch.setattr(gunzip, "GUNZIP_MIN_BYTES", 0)
    monkeypatch.delenv("ICNV_GUNZIP", raising=False)
    monkeypatch.delenv("ICNV_INFLATE", raising=False)
    return be


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(gr.zlib_streams()))
def test_restatement_equals_zlib(name):
    raw, data = gr.zlib_streams()[name]
    got, units, cand = gr.inflate(raw)
    assert got == data == zlib.decompress(raw, -15)
    assert len(units) == len(gr.starts_of(cand)), "a false candidate in zlib's own stream"
    if "mem8" in name:
        assert len(units) == 1
        return
    short = sum(len(u[3]) < gr.W for u in units)                           # a window spans many units (the mix: one unit holds
    assert len(units) >= 5 and short >= len(units) - (0 if name.startswith("counts") else 2)     # the stored random bytes)
    if "mem1" in name and name.startswith("counts"):
        assert {u[0] & 7 for u in units} == set(range(8))                 # unit starts at all eight bit residues
    markers = sum(v >= 256 for u in units for v in u[3])
    assert markers > (0.1 if name.startswith("counts") else 0.02) * len(data)     # history does not die out


def test_mix_runs_through_fixed_and_stored_blocks():
    raw, _ = gr.zlib_streams()["mix_mem1"]
    kinds, r, seen = set(), None, 0
    for at, st, end, sym in gr.chain(raw):
        r = gr.reader_at(raw, at, len(raw))
        r.take(1)
        kinds.add(r.take(2))
        seen += 1
    assert kinds == {2}                                                    # every unit STARTS with a dynamic block ...
    data = zlib.decompress(raw, -15)
    assert len(raw) > 20000 and seen < len(data) // 128                    # ... and the random part went through stored blocks inside units


@pytest.mark.parametrize("name", sorted(gr.hand_streams()))
def test_hand_built_streams(name):
    raw, data, blocks = gr.hand_streams()[name]
    got, units, cand = gr.inflate(raw)
    assert units[-1][1] == gr.OK_FINAL and units[-1][2] == len(raw) * 8
    if data is None:
        assert got is None                                                 # the `bad` flag
        with pytest.raises(zlib.error):
            zlib.decompress(raw, -15)
        return
    assert got == data == zlib.decompress(raw, -15)
    assert len(units) >= 2
    second = units[1][3]
    if name == "first_token_match_marker_w_minus_1":
        assert second[:3] == [gr.MARK | (gr.W - 1)] * 3
    if name == "distance_q_plus_w_marker_0":
        assert second[:5] == [gr.MARK | k for k in range(5)] and len(units[0][3]) == gr.W
    if name == "match_from_window_into_own_bytes":
        assert second[3:20] == [gr.MARK | (gr.W - 17 + k) for k in range(17)] and second[20:23] == [10, 11, 12]
    if name == "overlap_over_markers":
        assert second[:12] == [gr.MARK | (gr.W - 2), gr.MARK | (gr.W - 1)] * 6
    if name == "unit_of_zero_bytes":
        assert [len(u[3]) for u in units] == [300, 0, 5]
    if name in ("unit_of_exactly_w", "unit_of_w_plus_1"):
        assert len(units[1][3]) == gr.W + (name == "unit_of_w_plus_1")


def test_final_block_ends_at_every_bit_residue():
    """The closing fixed block holds k literals of 9 bits, k = 0 .. 7: the bit behind BFINAL's block moves through all eight
    residues, and OK_FINAL's end is that offset rounded up to a whole byte."""
    residues = set()
    for k in range(8):
        raw, data, blocks = gr.hand_streams()[f"final_after_{k}_nine_bit_literals"]
        units = gr.chain(raw)
        st, end, sym = gr.unit(raw, units[-1][0], frozenset(gr.candidates(raw)))
        assert st == gr.OK_FINAL and end == len(raw) * 8 and len(sym) == 4 + k
        first = gr.chain(gr.hand_streams()["final_after_0_nine_bit_literals"][0])[-1]
        assert units[-1][0] == first[0]                                    # the same bits in front of the closing block
        residues.add((9 * k) % 8)
    assert residues == set(range(8))


def test_distance_beyond_q_plus_w_cannot_be_written():
    """d > q + W is BAD_STREAM in the contract.  The 30 distance codes end at 32 768 = W, so with q >= 0 no stream can say it:
    the largest distance at q = 0 gives marker 0, and the codes 30 / 31 are BAD_STREAM of their own."""
    assert ir.DIST_BASE[29] + (1 << ir.DIST_EXTRA[29]) - 1 == gr.W
    raw = ir.fixed_block(ir.BitWriter(), [(3, gr.W)], final=True).bytes()
    assert gr.unit(raw, 0) == (gr.OK_FINAL, len(raw) * 8, [gr.MARK | 0, gr.MARK | 1, gr.MARK | 2])
    for name in ("distance_symbol_30", "distance_symbol_31"):
        assert gr.unit(ir.malformed()[name][0], 0)[0] == gr.BAD_STREAM


def test_planted_header_is_a_false_candidate():
    raw, data = gr.planted_header()
    got, units, cand = gr.inflate(raw)
    assert got == data and len(cand) == 3 and [u[0] for u in units] == [cand[0], cand[2]]
    assert cand[1] % 8 == 0                                                # inside the stored block's data
    st, end, sym = gr.unit(raw, cand[1], frozenset(cand))
    assert st in (gr.OK_BOUNDARY, gr.BAD_STREAM, gr.TRUNCATED)             # measured like any other, never on the chain


def test_committed_fixtures(golden_dir):
    gz = gr.golden_counts_gz()
    got, units, cand = gr.inflate(gr.gz_raw(gz))
    assert got == zlib.decompress(gz, 31) and len(units) == len(cand) == 12
    assert all(len(u[3]) > gr.W for u in units)
    outside = sum(v >= 256 for u in units for v in u[3][:len(u[3]) - gr.W])
    assert outside == 449060                                               # the markers outside the tails
    with open(os.path.join(golden_dir, "infercnv_object_example.rda"), "rb") as f:
        rda = f.read()
    got, units, cand = gr.inflate(gr.gz_raw(rda))
    assert got == zlib.decompress(rda, 31) and len(units) == len(cand) >= 6


@pytest.mark.parametrize("name", sorted(ir.malformed()))
def test_malformed_at_a_bit_offset(name):
    stream, want = ir.malformed()[name]
    for k in (0, 3, 5):
        shifted = (int.from_bytes(stream, "little") << k).to_bytes(len(stream) + 1, "little")
        st, end, sym = gr.unit(shifted, k)
        if want == ir.BAD_STREAM:
            assert st == gr.BAD_STREAM, k
        else:                                                              # K29's NEEDS_HISTORY: markers here, then the zero padding
            assert max(sym) >= gr.MARK


def test_max_in():
    raw, _ = gr.zlib_streams()["counts_mem2"]
    cand = gr.candidates(raw)
    st, end, sym = gr.unit(raw, cand[1], frozenset(cand))
    need = (end + 7) // 8 - (cand[1] >> 3)
    assert st == gr.OK_BOUNDARY
    assert gr.unit(raw, cand[1], frozenset(cand), need)[:2] == (st, end)
    assert gr.unit(raw, cand[1], frozenset(cand), need - 1)[0] == gr.TOO_LONG
    assert gr.unit(raw[:need + (cand[1] >> 3) - 1], cand[1], frozenset(cand))[0] == gr.TRUNCATED


# ---- gunzip.gunzip over the stand-in --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["counts_mem1", "mix_mem1", "mix_level1_mem1", "counts_level9_mem1", "counts_mem3"])
def test_gunzip_takes_zlibs_streams(stand_in, name):
    raw, data = gr.zlib_streams()[name]
    out = gunzip.gunzip(gr.gz_member(raw, data))
    st = gunzip.gunzip_stats()
    assert out is not None and out.tobytes() == data, st
    assert st["route"] == "device" and st["false_candidates"] == 0 and st["chain_units"] == st["candidates"] >= 10
    assert st["units_short"] >= st["chain_units"] - 1 and st["markers_tail"] > 0
    assert st["compressed_bytes"] == len(raw) + 18 and st["inflated_bytes"] == len(data)
    assert set(st["seconds"]) == {"upload", "find", "measure", "chain", "symbols", "tails", "resolve", "crc"}
    assert stand_in.calls == {"find": 1, "measure": 1, "symbols": 1, "tails": 1, "resolve": 1, "crc": 1}


def test_gunzip_takes_a_path_a_gzipfile_and_header_fields(stand_in, tmp_path):
    import gzip
    _, data = gr.zlib_streams()["counts_mem1"]
    c = zlib.compressobj(6, zlib.DEFLATED, 31, 1)                          # zlib's own gzip wrapper
    (tmp_path / "a.gz").write_bytes(c.compress(data) + c.flush())
    assert gunzip.gunzip(tmp_path / "a.gz").tobytes() == data
    raw, _ = gr.zlib_streams()["counts_mem1"]
    named = b"\x1f\x8b\x08\x08\x00\x00\x00\x00\x00\x03counts.tsv\x00" + raw + struct.pack("<II", zlib.crc32(data), len(data))
    assert gunzip.gunzip(named).tobytes() == data                           # FNAME is stepped over
    big = gr.poisson_tsv(400_000, 5)
    (tmp_path / "b.gz").write_bytes(gzip.compress(big, 6))                  # memLevel 8: a block every 16 383 symbols
    out = gunzip.gunzip(str(tmp_path / "b.gz"))
    assert out.tobytes() == big and gunzip.gunzip_stats()["chain_units"] >= 2


def test_planted_header_on_the_chain_walk(stand_in):
    raw, data = gr.planted_header()
    out = gunzip.gunzip(gr.gz_member(raw, data))
    st = gunzip.gunzip_stats()
    assert out.tobytes() == data and st["false_candidates"] == 1 and st["chain_units"] == 2 and st["candidates"] == 3


def turned_away(file_bytes, word, be=None, launched=None):
    assert gunzip.gunzip(file_bytes) is None
    st = gunzip.gunzip_stats()
    assert st["route"] == "host" and word in st["reason"], st
    if launched is not None:
        assert {k for k, v in be.calls.items() if v} == set(launched), be.calls
    return st


def test_turned_away(stand_in, monkeypatch):
    raw, data = gr.zlib_streams()["counts_mem1"]
    good = gr.gz_member(raw, data)
    assert gunzip.gunzip(good) is not None
    calls = lambda: stand_in.calls.update({k: 0 for k in stand_in.calls})
    calls()
    turned_away(b"BZh91AY&SY" + good, "not a gzip header", stand_in, [])
    turned_away(b"\x1f\x8b\x07" + good[3:], "not a gzip header", stand_in, [])
    turned_away(good[:12], "truncated", stand_in, [])
    # nothing to gain: one dynamic block; fixed only; stored only
    one, one_data = gr.zlib_streams()["counts_mem8"]
    turned_away(gr.gz_member(one, one_data), "nothing to gain", stand_in, ["find"])
    calls()
    fixed = zlib.compressobj(6, zlib.DEFLATED, -15, 1, zlib.Z_FIXED)
    turned_away(gr.gz_member(fixed.compress(data) + fixed.flush(), data), "nothing to gain")
    stored = zlib.compressobj(0, zlib.DEFLATED, -15)
    turned_away(gr.gz_member(stored.compress(data) + stored.flush(), data), "nothing to gain")
    # a second member; bytes behind the trailer
    calls()
    turned_away(good + good, "8-byte trailer", stand_in, ["find", "measure"])
    turned_away(good + b"\x00", "8-byte trailer")
    # the trailer
    calls()
    turned_away(good[:-8] + struct.pack("<II", zlib.crc32(data) ^ 1, len(data)), "CRC-32", stand_in, ["find", "measure", "symbols", "tails", "resolve", "crc"])
    calls()
    turned_away(good[:-8] + struct.pack("<II", zlib.crc32(data), len(data) + 1), "ISIZE", stand_in, ["find", "measure"])
    # a unit that is not OK: a cut file runs dry; a budget below the units' length
    turned_away(good[:len(good) // 2], "TRUNCATED")
    assert gunzip.gunzip(good, max_in=64) is None and "TOO_LONG" in gunzip.gunzip_stats()["reason"]
    damaged = bytearray(good)
    damaged[len(good) // 2] ^= 0x10
    assert gunzip.gunzip(bytes(damaged)) is None                             # whatever the flip did, zlib refuses it too
    with pytest.raises(zlib.error):
        zlib.decompress(bytes(damaged), 31)
    # a match in front of the stream's first byte
    for name in ("marker_in_first_unit", "marker_in_front_of_byte_0"):
        bad_raw = gr.hand_streams()[name][0]
        turned_away(gr.gz_member(bad_raw, b""), "", stand_in)
        assert "ISIZE" in gunzip.gunzip_stats()["reason"]                    # (ISIZE 0 is wrong: give it the length the symbols have)
        n_sym = sum(len(u[3]) for u in gr.chain(bad_raw))
        calls()
        turned_away(bad_raw.join([gr.gz_member(b"", b"")[:10], struct.pack("<II", 0, n_sym)]), "in front of the stream's first byte", stand_in,
                    ["find", "measure", "symbols", "tails", "resolve"])
    # a file that does not fit: given up before anything is allocated
    calls()
    stand_in.free = 2 * (len(raw) + 3 * len(data)) - 2
    turned_away(good, "does not fit", stand_in, ["find", "measure"])
    calls()
    stand_in.free = 2 * len(raw) - 2                                         # not even the compressed bytes: nothing is uploaded
    turned_away(good, "does not fit", stand_in, [])
    stand_in.free = 2 * (len(raw) + 3 * len(data))
    assert gunzip.gunzip(good) is not None
    # the switches
    calls()
    monkeypatch.setattr(gunzip, "GUNZIP_MIN_BYTES", len(good) + 1)
    turned_away(good, "GUNZIP_MIN_BYTES", stand_in, [])
    monkeypatch.setattr(gunzip, "GUNZIP_MIN_BYTES", len(good))
    assert gunzip.gunzip(good) is not None
    calls()
    for var in ("ICNV_GUNZIP", "ICNV_INFLATE"):
        monkeypatch.setenv(var, "0")
        turned_away(good, "switched off", stand_in, [])
        monkeypatch.delenv(var)
    assert gunzip.gunzip(good) is not None


def test_without_a_gpu_the_route_is_not_taken(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(gunzip, "GUNZIP_MIN_BYTES", 0)
    raw, data = gr.zlib_streams()["counts_mem1"]
    assert gunzip.gunzip(gr.gz_member(raw, data)) is None and gunzip.gunzip_stats()["reason"] == "no GPU"


def test_small_committed_fixtures_stay_on_the_host(stand_in, monkeypatch, golden_dir):
    monkeypatch.undo()
    assert len(gr.golden_counts_gz()) < gunzip.GUNZIP_MIN_BYTES
    assert os.path.getsize(os.path.join(golden_dir, "infercnv_object_example.rda")) < gunzip.GUNZIP_MIN_BYTES


def test_rds_offers_the_file_only_where_k29_gave_up(monkeypatch, tmp_path):
    """rds._open_on_device: K29 first; its None goes to gunzip.open_on_device; rds.inflate_stats() is K29's own."""
    from infercnv_amd import rds
    raw, data = gr.zlib_streams()["counts_mem1"]
    path = tmp_path / "x.rds"
    path.write_bytes(gr.gz_member(raw, data))
    be = gr.HostGunzip()
    monkeypatch.setattr(gunzip, "_backend", lambda: be)
    monkeypatch.setattr(gunzip, "GUNZIP_MIN_BYTES", 0)
    monkeypatch.setattr(rds, "_device_available", lambda: True)
    monkeypatch.setattr(rds, "_inflate_backend", lambda: ir.HostInflate())
    stream = rds._open_on_device(path)
    assert len(stream) == len(data) and bytes(stream[100:200]) == data[100:200]
    assert rds.inflate_stats()["route"] == "host" and "no flush points" in rds.inflate_stats()["reason"]
    assert gunzip.gunzip_stats()["route"] == "device"
    monkeypatch.setenv("ICNV_GUNZIP", "0")
    assert rds._open_on_device(path) is None
    monkeypatch.setenv("ICNV_INFLATE", "0")
    monkeypatch.setattr(gunzip, "_run", lambda *a, **k: pytest.fail("the device route was taken"))
    assert rds._open_on_device(path) is None
