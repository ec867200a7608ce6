"""K30 on the GPU (-m gpu): icnv_gunzip_find_dev / _measure_dev / _symbols_dev / _tails_dev / _resolve_dev against the sequential
restatement of tests/gunzip_restate.py, element for element -- candidates, statuses, ends, symbols including the marker
values, the resolved bytes -- over zlib's streams at small memLevels, hand-built units, the committed .gz fixtures and the
finder's geometry; gunzip.gunzip end to end; and load_infercnv_obj(return_device=True) of files without flush points.  In the
tests that expect the device route a fallback is a failure."""
import functools
import os
import struct
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gunzip_restate as gr  # noqa: E402
import inflate_restate as ir  # noqa: E402
from infercnv_amd._lib import IcnvError  # noqa: E402

GUARD = 16
TILE_BITS = 256 * 16        # the finder's workgroup tile: 256 lanes times 16 rounds, a lane per bit offset
OK = (gr.OK_BOUNDARY, gr.OK_FINAL)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infercnv_amd import device
    torch.cuda.set_device(0)
    device.init(0)
    return device


def on_device(data, offset=1):
    """data as a CUDA uint8 view `offset` bytes into its buffer (an odd address by default) that ends with the buffer."""
    buf = torch.full((len(data) + offset,), 0x5A, dtype=torch.uint8, device="cuda")
    if len(data):
        buf[offset:] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return buf[offset:]


def i64(values):
    return torch.tensor([int(v) for v in values], dtype=torch.int64, device="cuda")


def all_streams():
    out = {name: raw for name, (raw, _) in gr.zlib_streams().items()}
    out.update({name: raw for name, (raw, _, _) in gr.hand_streams().items()})
    out["planted_header"] = gr.planted_header()[0]
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """(raw, candidates, starts, [(status, end, symbols)] per start) of a named stream: computed once, shared, left unchanged."""
    if name == "golden_counts":
        raw = gr.gz_raw(gr.golden_counts_gz())
    else:
        raw = all_streams()[name]
    cand = gr.candidates(raw)
    starts = gr.starts_of(cand)
    stops = frozenset(cand)
    return raw, cand, starts, [gr.unit(raw, s, stops) for s in starts]


def find(dev, raw):
    got = dev.gunzip_find(on_device(raw))
    torch.cuda.synchronize()
    return got.cpu().numpy().tolist()


def measure(dev, src, cand, starts, max_in=1 << 30):
    end, out_len, status = dev.gunzip_measure(src, i64(cand), i64(starts), max_in)
    torch.cuda.synchronize()
    return end.cpu().numpy(), out_len.cpu().numpy(), status.cpu().numpy()


def symbols(dev, src, cand, starts, ends, lens, shorten_last=0):
    """(status, uint16 symbols, offsets): the units decoded side by side into a vector with GUARD symbols of 0xA5A5 behind the
    last one, which must come back untouched."""
    lens = np.asarray([int(x) for x in lens], dtype=np.int64)
    lens[-1] -= shorten_last
    offs = np.cumsum(lens) - lens
    sym = torch.full((int(lens.sum()) + GUARD,), -23131, dtype=torch.int16, device="cuda")     # 0xA5A5
    status = dev.gunzip_symbols(src, i64(cand), i64(starts), i64(ends), i64(offs), i64(lens), sym)
    torch.cuda.synchronize()
    host = sym.cpu().numpy().view(np.uint16)
    assert (host[int(lens.sum()):] == 0xA5A5).all(), "a store behind the last unit's range"
    return status.cpu().numpy(), host[:int(lens.sum())], offs


# ---- the finder -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(all_streams()) + ["golden_counts"])
def test_find_measure_and_symbols_equal_the_restatement(dev, name):
    raw, cand, starts, ref = reference(name)
    src = on_device(raw)
    got = dev.gunzip_find(src).cpu().numpy().tolist()
    assert got == cand, "candidates"
    end, out_len, status = measure(dev, src, cand, starts)
    assert status.tolist() == [r[0] for r in ref]
    ok = [i for i, r in enumerate(ref) if r[0] in OK]
    assert end[ok].tolist() == [ref[i][1] for i in ok] and out_len[ok].tolist() == [len(ref[i][2]) for i in ok]
    if not ok:
        return
    got_status, sym, offs = symbols(dev, src, cand, [starts[i] for i in ok], end[ok], out_len[ok])
    assert got_status.tolist() == status[ok].tolist()
    for k, i in enumerate(ok):
        want = np.asarray(ref[i][2], dtype=np.uint16)
        assert np.array_equal(sym[offs[k]:offs[k] + want.size], want), f"symbols of the unit at bit {starts[i]}"
    if name.startswith("counts") and "mem1" in name:
        assert {s & 7 for s in starts} == set(range(8))                    # starts at bit offsets 0 .. 7


def chain_of(name):
    raw, cand, starts, ref = reference(name)
    at = {s: r for s, r in zip(starts, ref)}
    units, s = [], 0
    while True:
        units.append(at[s])
        if at[s][0] != gr.OK_BOUNDARY:
            return units
        s = at[s][1]


@pytest.mark.parametrize("name", sorted(all_streams()) + ["golden_counts"])
def test_tails_and_resolve_equal_the_restatement(dev, name):
    units = chain_of(name)
    assert units[-1][0] == gr.OK_FINAL
    lens = np.array([len(u[2]) for u in units], dtype=np.int64)
    offs = np.cumsum(lens) - lens
    host_sym = np.array([v for u in units for v in u[2]], dtype=np.uint16)
    total = int(lens.sum())
    want = np.full(total, 0xA5, dtype=np.uint8)
    want_bad, want_markers = gr.tails(host_sym, offs, lens, want)
    after_tails = want.copy()
    want_bad_2 = gr.resolve(host_sym, offs, lens, want)
    sym = torch.from_numpy(host_sym.view(np.int16).copy()).cuda()
    out = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
    bad, markers = dev.gunzip_tails(sym, i64(offs), i64(lens), out)
    torch.cuda.synchronize()
    assert int(bad.item()) == want_bad and int(markers.item()) == want_markers
    assert np.array_equal(out.cpu().numpy(), after_tails), "the tails pass, the untouched rest included"
    bad = dev.gunzip_resolve(sym, i64(offs), i64(lens), out)
    torch.cuda.synchronize()
    assert int(bad.item()) == want_bad_2
    assert np.array_equal(out.cpu().numpy(), want)
    if not want_bad:
        assert out.cpu().numpy().tobytes() == zlib.decompress(reference(name)[0], -15)
    if name == "golden_counts":
        assert int((host_sym >= 256).sum()) - want_markers == 449060 and (lens > gr.W).all()


# ---- K29's and K30's kernels are one walker and one wavefront copy loop under two policies ---------------------------------------------
@functools.lru_cache(maxsize=None)
def one_unit_streams():
    """name -> (raw stream, K29's end, its bytes): the hand-built units and streams and zlib's streams that are ONE unit for K29
    from byte 0 -- no flush marker in front of BFINAL -- by the restatement."""
    named = {name: v[0] for name, v in ir.hand_units().items()}
    named.update({name: v[0] for name, v in gr.zlib_streams().items()})
    named.update({name: v[0] for name, v in gr.hand_streams().items()})
    units = {name: (raw, ir.unit_cached(raw)) for name, raw in named.items()}
    return {name: (raw, u[1], u[3]) for name, (raw, u) in sorted(units.items()) if u[0] == ir.OK_FINAL}


def block_kinds(raw):
    """What a valid stream holds, by a walk with the restatement's reader and codes: "stored" (a stored block with bytes),
    "fixed", "dynamic", and "wide_periodic": a match of at least 8 bytes (IF_WIDE_MIN: the 64 lanes copy it together) whose
    distance is below its length, so that byte k comes from offset k mod distance."""
    r, kinds = ir._Reader(raw, 0, len(raw)), set()
    while True:
        last, kind = r.take(1), r.take(2)
        if kind == 0:
            q = r.byte_pos()
            ln = struct.unpack_from("<H", raw, q)[0]
            r.bb, r.bc, r.p = 0, 0, q + 4 + ln
            kinds |= {"stored"} if ln else set()
        else:
            lit, dist = (ir.FIXED_LIT, ir.FIXED_DIST) if kind == 1 else ir._dynamic(r)
            while True:
                s = r.symbol(lit)
                if s == 256:
                    break
                kinds.add("fixed" if kind == 1 else "dynamic")
                if s > 256:
                    ln = ir.LEN_BASE[s - 257] + r.take(ir.LEN_EXTRA[s - 257])
                    d = r.symbol(dist)
                    d = ir.DIST_BASE[d] + r.take(ir.DIST_EXTRA[d])
                    kinds |= {"wide_periodic"} if ln >= 8 and d < ln else set()
        if last:
            return kinds


def test_one_unit_is_the_same_for_k29_and_k30(dev):
    """A stream that is one unit for K29 from byte 0 is the same unit for K30 from bit 0 under an EMPTY candidate list: the same
    out_len, the end 8 x K29's, and symbols that are K29's bytes, none a marker -- measured and decoded by both sets of kernels
    on the same bytes, all streams side by side in one buffer (a unit per wavefront, several workgroups)."""
    streams = one_unit_streams()
    kinds = set().union(*(block_kinds(raw) for raw, _, _ in streams.values()))
    assert kinds == {"stored", "fixed", "dynamic", "wide_periodic"} and len(streams) > 8, (kinds, sorted(streams))
    raws = [raw for raw, _, _ in streams.values()]
    starts = np.cumsum([len(r) for r in raws]) - [len(r) for r in raws]
    ends = starts + [end for _, end, _ in streams.values()]
    want = b"".join(data for _, _, data in streams.values())
    lens = np.array([len(data) for _, _, data in streams.values()], dtype=np.int64)
    offs = np.cumsum(lens) - lens
    total = int(lens.sum())
    src = on_device(b"".join(raws))

    end29, len29, st29 = (t.cpu().numpy() for t in dev.inflate_measure(src, i64(starts), 1 << 30))
    end30, len30, st30 = measure(dev, src, [], starts * 8)
    assert (st29 == ir.OK_FINAL).all() and (st30 == gr.OK_FINAL).all()
    assert np.array_equal(end29, ends) and np.array_equal(end30, 8 * end29)
    assert np.array_equal(len29, lens) and np.array_equal(len30, len29)

    out = torch.full((total + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    st29 = dev.inflate_units(src, i64(starts), i64(end29), i64(offs), i64(len29), out[:total])
    st30, sym, _ = symbols(dev, src, [], starts * 8, end30, len30)
    assert (st29.cpu().numpy() == ir.OK_FINAL).all() and (st30 == gr.OK_FINAL).all()
    got = out.cpu().numpy()
    assert (got[total:] == 0xA5).all(), "a store behind the last unit's range"
    assert got[:total].tobytes() == want, "K29's bytes"
    assert (sym < 256).all() and np.array_equal(sym, got[:total]), "K30's symbols are K29's bytes"


@pytest.mark.parametrize("back", [1, 3, 8, 16, 17, 18])
def test_find_a_header_that_straddles_two_workgroups(dev, back):
    """A true header that starts `back` bits before a workgroup's range ends: the 17 bits in front of its code lengths lie in
    one range, across its end, or it starts within the last 17 bits."""
    block = ir.dynamic_block(ir.BitWriter(), [1, 2, 3, (5, 2), 4]).bytes()
    at = 2 * TILE_BITS - back
    raw = (int.from_bytes(block, "little") << at).to_bytes(at // 8 + len(block) + 1, "little")
    got = find(dev, raw)
    assert got == gr.candidates(raw) and at in got


def test_find_a_header_cut_by_the_end_of_the_stream(dev):
    block = ir.dynamic_block(ir.BitWriter(), [1, 2, 3, (5, 2), 4]).bytes()
    r = gr.reader_at(block, 0, len(block))
    r.take(3)
    ir._dynamic(r)
    header_bits = gr.bit_pos(r)
    for lead in (0, 3, TILE_BITS - 40):                                     # the cut header at a tile's end as well
        whole = (int.from_bytes(block, "little") << lead).to_bytes((lead + 7) // 8 + len(block), "little")
        listed = 0
        for n in range(max(1, lead // 8), len(whole) + 1):
            got = find(dev, whole[:n])
            assert got == gr.candidates(whole[:n]), (lead, n)
            assert (lead in got) == (n * 8 >= lead + header_bits), (lead, n)
            listed += lead in got
        assert 0 < listed < len(whole)


def test_find_two_runs_and_a_callers_vector(dev):
    raw, cand, _, _ = reference("mix_mem1")
    src = on_device(raw)
    one, two = dev.gunzip_find(src).cpu().tolist(), dev.gunzip_find(src).cpu().tolist()
    assert one == two == cand
    own = torch.full((len(cand) + 3,), -7, dtype=torch.int64, device="cuda")
    assert dev.gunzip_find(src, cand=own).cpu().tolist() == cand and own[len(cand):].cpu().tolist() == [-7] * 3
    small = torch.full((len(cand) - 1,), -7, dtype=torch.int64, device="cuda")
    with pytest.raises(IcnvError, match="cand_cap"):
        dev.gunzip_find(src, cand=small)
    assert small.cpu().tolist() == [-7] * (len(cand) - 1)                   # nothing was written
    assert dev.gunzip_find(on_device(b"\x04\x00")).numel() == 0            # no room for a header


def test_planted_header_is_listed_measured_and_never_on_the_chain(dev, monkeypatch):
    from infercnv_amd import gunzip
    raw, data = gr.planted_header()
    _, cand, starts, ref = reference("planted_header")
    assert find(dev, raw) == cand and len(cand) == 3
    monkeypatch.setattr(gunzip, "GUNZIP_MIN_BYTES", 0)
    out = gunzip.gunzip(gr.gz_member(raw, data))
    st = gunzip.gunzip_stats()
    assert st["route"] == "device" and st["false_candidates"] == 1 and st["chain_units"] == 2, st
    assert out.cpu().numpy().tobytes() == data


# ---- measure and symbols at the edges ---------------------------------------------------------------------------------------------------------
def test_max_in_below_a_units_length_is_too_long(dev):
    raw, cand, starts, ref = reference("counts_mem2")
    src = on_device(raw)
    need = [(r[1] + 7) // 8 - (s >> 3) for s, r in zip(starts, ref)]
    for delta, want in ((0, None), (-1, gr.TOO_LONG)):
        for i in (0, 1, len(starts) - 2):
            end, out_len, status = measure(dev, src, cand, [starts[i]], need[i] + delta)
            assert status[0] == (ref[i][0] if want is None else want), (i, delta)
            assert status[0] == gr.unit(raw, starts[i], frozenset(cand), need[i] + delta)[0]
    end, out_len, status = measure(dev, on_device(raw[:len(raw) - 3]), cand, [starts[-1]])
    assert status[0] == gr.TRUNCATED


@pytest.mark.parametrize("shift", [1, 3, 5, 7])
def test_malformed_streams_at_a_bit_offset(dev, shift):
    names = sorted(ir.malformed())
    shifted = [(int.from_bytes(ir.malformed()[n][0], "little") << shift).to_bytes(len(ir.malformed()[n][0]) + 1, "little") for n in names]
    raw = b"".join(shifted)
    starts = (np.cumsum([0] + [len(s) for s in shifted[:-1]]) * 8 + shift).tolist()
    src = on_device(raw)
    end, out_len, status = measure(dev, src, [], starts)
    for n, s, got in zip(names, starts, status.tolist()):
        assert got == gr.unit(raw, s)[0], n
        if ir.malformed()[n][1] == ir.BAD_STREAM:
            assert got == gr.BAD_STREAM, n


def test_a_capacity_one_short_is_bad_stream_and_stores_nothing_outside(dev):
    for name in ("mix_mem1", "length_258_over_markers", "through_fixed_and_stored", "unit_of_w_plus_1"):
        raw, cand, starts, ref = reference(name)
        src = on_device(raw)
        for i in range(1, len(starts)):
            if ref[i][0] not in OK or not ref[i][2]:
                continue
            st, sym, _ = symbols(dev, src, cand, [starts[i]], [ref[i][1]], [len(ref[i][2])], shorten_last=1)     # (asserts the guard)
            assert st.tolist() == [gr.BAD_STREAM], (name, i)
        st, sym, _ = symbols(dev, src, cand, [starts[1]], [ref[1][1] - 8], [len(ref[1][2])])
        assert st.tolist() == [gr.BAD_STREAM]                               # an end that comes too early


def test_refusals(dev):
    raw, cand, starts, ref = reference("counts_mem2")
    src = on_device(raw)
    n = len(raw)
    with pytest.raises(IcnvError, match="start is outside"):
        dev.gunzip_measure(src, i64(cand), i64([0, n * 8]), 1 << 20)
    with pytest.raises(IcnvError, match="start is outside"):
        dev.gunzip_measure(src, i64(cand), i64([-1]), 1 << 20)
    sym = torch.zeros(100, dtype=torch.int16, device="cuda")
    for offs, lens in (([0, 60], [50, 40]), ([0, 50], [50, 51]), ([1], [50])):                  # a gap, past the capacity, not from 0
        with pytest.raises(IcnvError, match="prefix sums"):
            dev.gunzip_symbols(src, i64(cand), i64(starts[:len(offs)]), i64([r[1] for r in ref[:len(offs)]]), i64(offs), i64(lens), sym)
        out = torch.zeros(100, dtype=torch.uint8, device="cuda")
        with pytest.raises(IcnvError, match="prefix sums"):
            dev.gunzip_tails(sym, i64(offs), i64(lens), out)
        with pytest.raises(IcnvError, match="prefix sums"):
            dev.gunzip_resolve(sym, i64(offs), i64(lens), out)
    with pytest.raises(IcnvError, match="end outside"):
        dev.gunzip_symbols(src, i64(cand), i64([starts[1]]), i64([starts[1] - 1]), i64([0]), i64([50]), sym)
    with pytest.raises(TypeError):
        dev.gunzip_symbols(src, i64(cand), i64([0]), i64([8]), i64([0]), i64([5]), sym.to(torch.int32))
    with pytest.raises(TypeError):
        dev.gunzip_tails(sym, i64([0]), i64([50]), torch.zeros(99, dtype=torch.uint8, device="cuda"))


# ---- gunzip.gunzip ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def gz(dev, monkeypatch):
    from infercnv_amd import gunzip
    monkeypatch.setattr(gunzip, "GUNZIP_MIN_BYTES", 0)
    monkeypatch.delenv("ICNV_GUNZIP", raising=False)
    monkeypatch.delenv("ICNV_INFLATE", raising=False)
    return gunzip


def test_gunzip_of_zlibs_streams(gz):
    for name, (raw, data) in gr.zlib_streams().items():
        out = gz.gunzip(gr.gz_member(raw, data))
        st = gz.gunzip_stats()
        if "mem8" in name:
            assert out is None and st["route"] == "host" and "nothing to gain" in st["reason"]
            continue
        assert st["route"] == "device", (name, st)
        assert out.is_cuda and out.dtype == torch.uint8 and out.cpu().numpy().tobytes() == data
        assert st["false_candidates"] == 0 and st["chain_units"] == st["candidates"] and st["units_short"] >= st["chain_units"] - 2


def test_gunzip_of_the_committed_fixtures(gz, golden_dir):
    gz_bytes = gr.golden_counts_gz()
    out = gz.gunzip(gz_bytes)
    st = gz.gunzip_stats()
    assert st["route"] == "device" and st["chain_units"] == 12 and st["units_short"] == 0 and st["false_candidates"] == 0, st
    assert out.cpu().numpy().tobytes() == zlib.decompress(gz_bytes, 31)
    path = os.path.join(golden_dir, "infercnv_object_example.rda")
    out = gz.gunzip(path)
    st = gz.gunzip_stats()
    assert st["route"] == "device" and st["false_candidates"] == 0, st
    with open(path, "rb") as f:
        assert out.cpu().numpy().tobytes() == zlib.decompress(f.read(), 31)


def test_gunzip_of_hand_built_streams(gz):
    for name, (raw, data, _) in gr.hand_streams().items():
        n_sym = sum(len(u[2]) for u in chain_of(name))
        trailer = struct.pack("<II", zlib.crc32(data or b""), n_sym)
        out = gz.gunzip(gr.gz_member(b"", b"")[:10] + raw + trailer)
        st = gz.gunzip_stats()
        if data is None:                                                    # a match in front of the stream's start: the host's to refuse
            assert out is None and st["route"] == "host" and "in front of the stream's first byte" in st["reason"], (name, st)
        else:
            assert st["route"] == "device" and out.cpu().numpy().tobytes() == data, (name, st)


def test_gunzip_turned_away(gz, monkeypatch):
    raw, data = gr.zlib_streams()["counts_mem1"]
    good = gr.gz_member(raw, data)
    assert gz.gunzip(good) is not None

    def away(file_bytes, word):
        assert gz.gunzip(file_bytes) is None
        st = gz.gunzip_stats()
        assert st["route"] == "host" and word in st["reason"], st

    away(good + good, "8-byte trailer")
    away(good[:-8] + struct.pack("<II", zlib.crc32(data) ^ 1, len(data)), "CRC-32")
    away(good[:-8] + struct.pack("<II", zlib.crc32(data), len(data) + 1), "ISIZE")
    away(good[:len(good) // 2], "TRUNCATED")
    away(b"\x1f\x8b\x07" + good[3:], "not a gzip header")
    assert gz.gunzip(good, max_in=64) is None and "TOO_LONG" in gz.gunzip_stats()["reason"]
    monkeypatch.setattr(gz, "GUNZIP_MIN_BYTES", len(good) + 1)
    away(good, "GUNZIP_MIN_BYTES")
    monkeypatch.setattr(gz, "GUNZIP_MIN_BYTES", 0)
    for var in ("ICNV_GUNZIP", "ICNV_INFLATE"):
        monkeypatch.setenv(var, "0")
        away(good, "switched off")
        monkeypatch.delenv(var)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True])
def test_load_infercnv_obj_from_a_file_without_flush_points(gz, tmp_path, monkeypatch, sparse):
    import gzip
    from infercnv_amd import load_infercnv_obj, rds, save_infercnv_obj
    from test_gpu_deflate import compressible_object
    from test_rds_host import assert_same_object
    obj = compressible_object(sparse)
    save_infercnv_obj(obj, tmp_path / "plain.rds", device=False)
    plain = (tmp_path / "plain.rds").read_bytes()
    with gzip.GzipFile(tmp_path / "py.rds.gz", "wb") as f:                   # no flush points: what R writes
        f.write(plain)
    monkeypatch.setattr(rds, "DEVICE_THRESHOLD", 20_000)
    monkeypatch.setattr(rds, "CHUNK_BYTES", 40_000)
    monkeypatch.setattr(rds, "WINDOW_BYTES", 3_000)
    want, want_x = load_infercnv_obj(tmp_path / "plain.rds", return_device=True)
    got, got_x = load_infercnv_obj(tmp_path / "py.rds.gz", return_device=True)
    st = gz.gunzip_stats()
    print(f"gunzip_stats: {st}")
    assert st["route"] == "device" and st["chain_units"] >= 2 and st["inflated_bytes"] == len(plain), st
    assert rds.inflate_stats()["route"] == "host"                             # K29 gave up first, and says so
    assert got_x.is_cuda and torch.equal(got_x.view(torch.int64), want_x.view(torch.int64))   # bit for bit
    host_obj = load_infercnv_obj(tmp_path / "plain.rds")

    def same(o, x):
        o.expr_data = np.ascontiguousarray(x.cpu().numpy().T)
        assert np.array_equal(host_obj.expr_data.view(np.int64), o.expr_data.view(np.int64))
        assert_same_object(host_obj, o)

    same(got, got_x)
    # the routes that stay as they were: the switches, a small file, return_device=False
    for var in ("ICNV_GUNZIP", "ICNV_INFLATE"):
        with monkeypatch.context() as m:
            m.setenv(var, "0")
            m.setattr(gz, "_run", lambda *a, **k: pytest.fail("the device route was taken"))
            off, off_x = load_infercnv_obj(tmp_path / "py.rds.gz", return_device=True)
            same(off, off_x)
    with monkeypatch.context() as m:
        m.setattr(gz, "GUNZIP_MIN_BYTES", os.path.getsize(tmp_path / "py.rds.gz") + 1)
        small, small_x = load_infercnv_obj(tmp_path / "py.rds.gz", return_device=True)
        assert gz.gunzip_stats()["route"] == "host" and "GUNZIP_MIN_BYTES" in gz.gunzip_stats()["reason"]
        same(small, small_x)
    assert_same_object(host_obj, load_infercnv_obj(tmp_path / "py.rds.gz"))


def test_turned_away_files_give_what_the_host_route_gives(gz, tmp_path, monkeypatch):
    """Two members, a flipped CRC, a flipped ISIZE, a truncated file, through load_infercnv_obj(return_device=True): gunzip
    turns each away with its reason, and the call ends as it does with ICNV_INFLATE=0 -- the same object, or the same error."""
    import gzip
    from infercnv_amd import load_infercnv_obj, rds, save_infercnv_obj
    from test_gpu_deflate import compressible_object
    from test_rds_host import assert_same_object
    save_infercnv_obj(compressible_object(False), tmp_path / "plain.rds", device=False)
    good = gzip.compress((tmp_path / "plain.rds").read_bytes(), 6)
    crc, isize = struct.unpack("<II", good[-8:])
    cases = {"two_members": (good + good, "8-byte trailer"),
             "flipped_crc": (good[:-8] + struct.pack("<II", crc ^ 1, isize), "CRC-32"),
             "flipped_isize": (good[:-8] + struct.pack("<II", crc, isize ^ 1), "ISIZE"),
             "truncated": (good[:len(good) // 2], "TRUNCATED")}
    monkeypatch.setattr(rds, "DEVICE_THRESHOLD", 20_000)

    def outcome(path):
        try:
            obj, x = load_infercnv_obj(path, return_device=True)
        except Exception as exc:                                            # compared below: type and text
            return None, (type(exc), str(exc))
        obj.expr_data = np.ascontiguousarray(x.cpu().numpy().T)
        return obj, None

    (tmp_path / "good.rds").write_bytes(good)
    assert outcome(tmp_path / "good.rds")[1] is None and gz.gunzip_stats()["route"] == "device"
    for name, (file_bytes, word) in cases.items():
        path = tmp_path / f"{name}.rds"
        path.write_bytes(file_bytes)
        got, got_err = outcome(path)
        st = gz.gunzip_stats()
        assert st["route"] == "host" and word in st["reason"], (name, st)
        with monkeypatch.context() as m:
            m.setenv("ICNV_INFLATE", "0")
            m.setattr(gz, "_run", lambda *a, **k: pytest.fail("the device route was taken"))
            want, want_err = outcome(path)
        assert got_err == want_err, name
        assert (got is None) == (want is None), name
        if got is not None:
            assert np.array_equal(got.expr_data.view(np.int64), want.expr_data.view(np.int64))
            assert_same_object(want, got)
    assert {name: outcome(tmp_path / f"{name}.rds")[1] is None for name in cases} == \
        {"two_members": True, "flipped_crc": False, "flipped_isize": False, "truncated": False}      # what Python's gzip makes of them


def test_load_the_r_written_object(gz, golden_dir, monkeypatch):
    """R's own gzip .rda (save(), compress = TRUE: gzfile, level 6) through the device route, against the arrays extracted from
    it on the host (tests/golden/infercnv_object_example.npz)."""
    from infercnv_amd import load_infercnv_obj, rds
    from test_rds_host import assert_same_object
    path = os.path.join(golden_dir, "infercnv_object_example.rda")
    monkeypatch.setattr(rds, "DEVICE_THRESHOLD", 20_000)
    monkeypatch.setattr(rds, "CHUNK_BYTES", 40_000)
    monkeypatch.setattr(rds, "WINDOW_BYTES", 3_000)
    obj, x = load_infercnv_obj(path, return_device=True)
    st = gz.gunzip_stats()
    assert st["route"] == "device" and st["chain_units"] >= 6 and st["false_candidates"] == 0, st
    d = np.load(os.path.join(golden_dir, "infercnv_object_example.npz"), allow_pickle=False)
    assert x.is_cuda and np.array_equal(np.ascontiguousarray(x.cpu().numpy().T).view(np.int64), d["expr_data"].view(np.int64))
    host_obj = load_infercnv_obj(path)
    obj.expr_data = np.ascontiguousarray(x.cpu().numpy().T)
    assert_same_object(host_obj, obj)
