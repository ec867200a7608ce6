"""K30's second consumer on the GPU (-m gpu): device.read_table and device.read_mtx on a .gz that gunzip.gunzip takes, against
the same file uncompressed -- every returned array bit for bit, with and without cells=, in many chunks, stats["source"] as
stated --, a refused byte with the same line and field, CreateInfercnvObject from a 10x directory of .gz files slot for slot,
and the files that are turned away.  In the tests that expect the device route a fallback is a failure."""
import gzip
import os

import numpy as np
import pytest

import create_object_restate as cor
import sparse_counts_restate as scr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pytest.importorskip("scipy")

import infercnv_amd                                    # noqa: E402
from infercnv_amd import _lib                          # noqa: E402

REFS = ["Microglia/Macrophage", "Oligodendrocytes (non-malignant)"]
BANNER = b"%%MatrixMarket matrix coordinate integer general\n"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infercnv_amd import device
    torch.cuda.set_device(0)
    device.init(0)
    return device


@pytest.fixture
def gz(dev, monkeypatch):
    from infercnv_amd import gunzip
    monkeypatch.setattr(gunzip, "GUNZIP_MIN_BYTES", 0)
    monkeypatch.delenv("ICNV_GUNZIP", raising=False)
    monkeypatch.delenv("ICNV_INFLATE", raising=False)
    return gunzip


@pytest.fixture(scope="module")
def table(golden_dir, tmp_path_factory):
    """The committed counts table (363 KB .gz, 12 units) and the same bytes uncompressed."""
    src = os.path.join(golden_dir, "create_object_example", "counts_every_8th_gene.matrix.gz")
    with gzip.open(src, "rb") as f:
        text = f.read()
    plain = str(tmp_path_factory.mktemp("table") / "counts.matrix")
    with open(plain, "wb") as f:
        f.write(text)
    return {"gz": src, "plain": plain, "text": text}


@pytest.fixture(scope="module")
def mtx(tmp_path_factory):
    """700 x 400 at about 25 %: some 70 000 entries, 800 KB of text -- several DEFLATE blocks at gzip's default settings --
    with blank lines and \\r\\n scattered; plain and .gz hold the same bytes."""
    rng = np.random.default_rng(30)
    m = rng.integers(1, 3000, size=(700, 400)) * (rng.random((700, 400)) < 0.25)
    d = tmp_path_factory.mktemp("mtx")
    plain, packed = str(d / "m.mtx"), str(d / "m.mtx.gz")
    scr.write_mtx(plain, m, eol=lambda k: b"\r\n" if k % 5 == 0 else b"\n", blank_every=7)
    with open(plain, "rb") as f, gzip.open(packed, "wb") as g:
        g.write(f.read())
    return {"plain": plain, "gz": packed, "dense": m}


def same_table(got, want):
    (rows_a, cols_a, x_a, _), (rows_b, cols_b, x_b, _) = got, want
    assert rows_a == rows_b and cols_a == cols_b
    assert x_a.shape == x_b.shape and x_a.dtype == x_b.dtype == torch.float64 and x_a.is_contiguous()
    assert torch.equal(x_a.view(torch.int64), x_b.view(torch.int64))            # bit for bit


@pytest.mark.parametrize("kw", [dict(), dict(chunk_bytes=50_000), dict(cells=[5, 0, 17, 3]), dict(cells=[7, 2], chunk_bytes=30_001)])
def test_read_table_of_a_gz_equals_the_plain_file(dev, gz, table, kw):
    got, want = dev.read_table(table["gz"], **kw), dev.read_table(table["plain"], **kw)
    same_table(got, want)
    assert got[3]["source"] == "device_gunzip" and got[3]["source_reason"] == "", gz.gunzip_stats()
    assert want[3]["source"] == "host"
    assert got[3]["bytes"] == want[3]["bytes"] and got[3]["rows"] == want[3]["rows"] and got[3]["fields"] == want[3]["fields"]
    if "chunk_bytes" in kw:
        assert got[3]["chunks"] >= 15                                          # many chunks, cut at arbitrary (unaligned) lines
    assert len(got[0]) > 1000 and got[2].shape[0] == (len(kw["cells"]) if "cells" in kw else len(got[1]))


def test_read_table_quoted_names_and_crlf(dev, gz, tmp_path):
    """Quoted row and column names, \\r\\n line ends, blank lines, a last line without its end: the names are sliced where
    there is no host copy of a chunk as where there is one."""
    rng = np.random.default_rng(31)
    lines = ["\t".join(f'"c{j}"' for j in range(40))]
    for i in range(3000):
        lines.append("\t".join([f'"gene {i}"' if i % 3 else f"g{i}"] + [str(v) for v in rng.poisson(3.0, 40)]) + ("\r" if i % 4 == 0 else ""))
        if i % 500 == 7:
            lines.append("")
    text = "\n".join(lines).encode()
    (tmp_path / "q.tsv").write_bytes(text)
    with gzip.open(tmp_path / "q.tsv.gz", "wb") as f:
        f.write(text)
    for kw in (dict(), dict(chunk_bytes=9_999), dict(cells=[39, 0], chunk_bytes=20_000)):
        got, want = dev.read_table(str(tmp_path / "q.tsv.gz"), **kw), dev.read_table(str(tmp_path / "q.tsv"), **kw)
        same_table(got, want)
        assert got[3]["source"] == "device_gunzip", gz.gunzip_stats()
        assert got[0][1] == "gene 1" and got[0][0] == "g0" and got[1][0] == "c0"


def csc(counts):
    return (counts.G, counts.C) + tuple(t.cpu().numpy() for t in counts.t[1:])


@pytest.mark.parametrize("kw", [dict(), dict(chunk_bytes=20_000), dict(cells=[3, 399, 0, 17]), dict(cells=[9, 8], chunk_bytes=33_333)])
def test_read_mtx_of_a_gz_equals_the_plain_file(dev, gz, mtx, kw):
    (got, st), (want, st_plain) = dev.read_mtx(mtx["gz"], **kw), dev.read_mtx(mtx["plain"], **kw)
    assert st["source"] == "device_gunzip" and st_plain["source"] == "host", gz.gunzip_stats()
    a, b = csc(got), csc(want)
    assert a[:2] == b[:2] and all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a[2:], b[2:]))
    for key in ("bytes", "entries", "sorted_on_device") + (("entries_kept",) if "cells" in kw else ()):
        assert st[key] == st_plain[key], key
    if "chunk_bytes" in kw:
        assert st["chunks"] >= 20
    if not kw:
        G, C, colptr, rowidx, vals, _ = scr.read_mtx(mtx["plain"])
        assert a[:2] == (G, C) and np.array_equal(a[2], colptr) and np.array_equal(a[3], rowidx) and np.array_equal(a[4], vals)


def raises_the_same(call, plain, packed, kind):
    with pytest.raises(kind) as want:
        call(plain)
    with pytest.raises(kind) as got:
        call(packed)
    assert str(got.value) == str(want.value) and ("line " in str(want.value) or kind is ValueError)
    return str(want.value)


@pytest.mark.parametrize("chunk", [None, 40_000])
def test_a_refused_byte_reports_the_same_line_and_field(dev, gz, table, mtx, tmp_path, chunk):
    lines = table["text"].split(b"\n")
    at = len(lines) // 2
    fields = lines[at].split(b"\t")
    fields[9] = b"1x7"
    lines[at] = b"\t".join(fields)
    lines[at + 300] = lines[at + 300] + b"\tone_too_many"                      # a later refusal loses
    bad = b"\n".join(lines)
    (tmp_path / "bad.matrix").write_bytes(bad)
    with gzip.open(tmp_path / "bad.matrix.gz", "wb") as f:
        f.write(bad)
    text = raises_the_same(lambda p: dev.read_table(p, chunk_bytes=chunk), str(tmp_path / "bad.matrix"), str(tmp_path / "bad.matrix.gz"),
                           _lib.IcnvError)
    assert f"line {at + 1}, field 10" in text and "1x7" in text
    assert gz.gunzip_stats()["route"] == "device"
    with open(mtx["plain"], "rb") as f:
        body = f.read().split(b"\n")
    at = next(k for k in range(40_000, len(body)) if body[k].strip())           # a line that holds an entry
    body[at] = b"2 2 0.5"
    (tmp_path / "bad.mtx").write_bytes(b"\n".join(body))
    with gzip.open(tmp_path / "bad.mtx.gz", "wb") as f:
        f.write(b"\n".join(body))
    text = raises_the_same(lambda p: dev.read_mtx(p, chunk_bytes=chunk), str(tmp_path / "bad.mtx"), str(tmp_path / "bad.mtx.gz"), _lib.IcnvError)
    assert f"line {at + 1}, field 3" in text and gz.gunzip_stats()["route"] == "device"
    # a size line that miscounts: the same ValueError
    body = body[:at] + body[at + 1:]
    (tmp_path / "short.mtx").write_bytes(b"\n".join(body))
    with gzip.open(tmp_path / "short.mtx.gz", "wb") as f:
        f.write(b"\n".join(body))
    assert "the size line says" in raises_the_same(lambda p: dev.read_mtx(p, chunk_bytes=chunk), str(tmp_path / "short.mtx"),
                                                   str(tmp_path / "short.mtx.gz"), ValueError)


@pytest.fixture(scope="module")
def tenx(golden_dir, tmp_path_factory):
    d = os.path.join(golden_dir, "create_object_example")
    genes, cells, x_bits = cor.read_table(os.path.join(d, "counts_every_8th_gene.matrix.gz"))
    x = np.rint(cor.as_double(x_bits)).astype(np.int64)
    out = tmp_path_factory.mktemp("tenx_gz")
    scr.write_mtx(str(out / "matrix.mtx.gz"), x)
    with gzip.open(str(out / "features.tsv.gz"), "wt") as fh:
        fh.write("".join(f"ENSG{i:011d}\t{s}\tGene Expression\n" for i, s in enumerate(genes)))
    with gzip.open(str(out / "barcodes.tsv.gz"), "wt") as fh:
        fh.write("".join(c + "\n" for c in cells))
    return {"dir": str(out), "order": os.path.join(d, "gencode_downsampled.EXAMPLE_ONLY_DONT_REUSE.txt.gz"),
            "annot": os.path.join(d, "oligodendroglioma_annotations_downsampled.txt.gz"), "table": os.path.join(d, "counts_every_8th_gene.matrix.gz")}


def same_slots(a, b):
    dense = lambda m: m.toarray() if hasattr(m, "toarray") else np.ascontiguousarray(m)
    assert type(a.expr_data) is type(b.expr_data)
    assert np.array_equal(dense(a.expr_data).view(np.int64), dense(b.expr_data).view(np.int64))
    assert np.array_equal(dense(a.count_data).view(np.int64), dense(b.count_data).view(np.int64))
    assert list(a.gene_names) == list(b.gene_names) and list(a.cell_names) == list(b.cell_names)
    for slot in ("chr", "start", "stop"):
        assert list(getattr(a.gene_order, slot)) == list(getattr(b.gene_order, slot))
    for da, db in ((a.reference_grouped_cell_indices, b.reference_grouped_cell_indices),
                   (a.observation_grouped_cell_indices, b.observation_grouped_cell_indices)):
        assert list(da) == list(db) and all(np.array_equal(da[k], db[k]) and da[k].dtype == db[k].dtype for k in da)
    assert a.options == b.options and a.validate()


def test_create_object_from_gz_files_slot_for_slot(dev, gz, tenx, monkeypatch):
    """A 10x directory of .gz files and a .gz table, device route against the same calls with ICNV_GUNZIP=0."""
    seen, real = [], gz.gunzip
    monkeypatch.setattr(gz, "gunzip", lambda *a, **k: (seen.append(a), real(*a, **k))[1])
    from_dir = infercnv_amd.CreateInfercnvObject(tenx["dir"], tenx["order"], tenx["annot"], REFS)
    assert len(seen) == 1 and gz.gunzip_stats()["route"] == "device", gz.gunzip_stats()
    from_table = infercnv_amd.CreateInfercnvObject(tenx["table"], tenx["order"], tenx["annot"], REFS)
    assert len(seen) == 2 and gz.gunzip_stats()["route"] == "device", gz.gunzip_stats()
    with monkeypatch.context() as m:
        m.setenv("ICNV_GUNZIP", "0")
        m.setattr(gz, "gunzip", lambda *a, **k: pytest.fail("the device route was taken"))
        same_slots(from_dir, infercnv_amd.CreateInfercnvObject(tenx["dir"], tenx["order"], tenx["annot"], REFS))
        same_slots(from_table, infercnv_amd.CreateInfercnvObject(tenx["table"], tenx["order"], tenx["annot"], REFS))
    assert len(from_dir.gene_names) > 1000


def test_files_that_are_turned_away_take_the_host_route(dev, gz, table, mtx, tmp_path, monkeypatch):
    want_t, want_m = dev.read_table(table["plain"]), dev.read_mtx(mtx["plain"])
    with open(table["gz"], "rb") as f:
        good = f.read()

    def both(expect):
        got = dev.read_table(table["gz"])
        same_table(got, want_t)
        got_m, st = dev.read_mtx(mtx["gz"])
        assert all(np.array_equal(x, y) for x, y in zip(csc(got_m)[2:], csc(want_m[0])[2:]))
        for stats in (got[3], st):
            assert stats["source"] == "host" and expect in stats["source_reason"], stats

    for var in ("ICNV_GUNZIP", "ICNV_INFLATE"):
        with monkeypatch.context() as m:
            m.setenv(var, "0")
            m.setattr(gz, "gunzip", lambda *a, **k: pytest.fail("the device route was taken"))
            both("switched off")
    with monkeypatch.context() as m:
        m.setattr(gz, "GUNZIP_MIN_BYTES", 1 << 30)
        both("GUNZIP_MIN_BYTES")
    # two members: Python's gzip reads both, and so does this reader through it
    (tmp_path / "two.matrix.gz").write_bytes(good + gzip.compress(b""))
    got = dev.read_table(str(tmp_path / "two.matrix.gz"))
    same_table(got, want_t)
    assert got[3]["source"] == "host" and "8-byte trailer" in got[3]["source_reason"]
    # a flipped CRC, a flipped ISIZE, a truncated file: the error Python's gzip raises, as before
    for name, damaged, word in (("crc", good[:-8] + bytes([good[-8] ^ 1]) + good[-7:], "CRC-32"),
                                ("isize", good[:-4] + bytes([good[-4] ^ 1]) + good[-3:], "ISIZE"),
                                ("cut", good[:len(good) // 2], "TRUNCATED")):
        path = str(tmp_path / f"{name}.matrix.gz")
        with open(path, "wb") as f:
            f.write(damaged)
        with pytest.raises(Exception) as got_err:
            dev.read_table(path)
        assert word in gz.gunzip_stats()["reason"], (name, gz.gunzip_stats())
        with monkeypatch.context() as m:
            m.setenv("ICNV_INFLATE", "0")
            with pytest.raises(Exception) as want_err:
                dev.read_table(path)
        assert type(got_err.value) is type(want_err.value) and str(got_err.value) == str(want_err.value), name
