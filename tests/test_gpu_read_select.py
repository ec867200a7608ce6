"""Reading a selection of columns on the GPU (include/icnv.h "reading a selection of columns", DESIGN K26): device.read_table
and device.read_mtx with cells=, the two C entries' map check, and ShardedCreate on the example's inputs.  Every comparison is
bit for bit: against the full read followed by the gather / selector the parent route uses, and against
tests/read_select_restate.py."""
import ctypes as ct
import gzip
import os

import numpy as np
import pytest

import create_object_restate as cor
import read_select_restate as rsr
import sparse_counts_restate as scr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pytest.importorskip("scipy")

import infercnv_amd                                    # noqa: E402
from infercnv_amd import _lib, sharded                 # noqa: E402

REFS = ["Microglia/Macrophage", "Oligodendrocytes (non-malignant)"]
TIE = "9007199254740993"                                # 2^53 + 1: an exact tie, which the device does not certify


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infercnv_amd import device
    torch.cuda.set_device(0)
    device.init(0)
    return device


def bits(x):
    return x.cpu().numpy().view(np.int64)


# ---------------------------------------------------------------------------------------------------------------- dense
FIELDS = ("0", "7", "13", "2.5", "1e3", "-4", "NA", "", "0.125", "12345.678", "+6", "3.", ".5", "NaN", "1e-3")


def write_table(path, n_rows, n_cols, corner, seed, patch=None):
    """A table with "\\r\\n" on every third line, a blank line after every fifth row, NA and empty fields all over; `corner`:
    the header has a label for the row names.  patch: {(row, col): text}."""
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(FIELDS), size=(n_rows, n_cols))
    out = [("\t".join((["gene"] if corner else []) + [f"c{j}" for j in range(n_cols)]) + "\n").encode()]
    for i in range(n_rows):
        row = [FIELDS[k] for k in pick[i]]
        for (r, c), text in (patch or {}).items():
            if r == i:
                row[c] = text
        out.append(("\t".join(['"r%d"' % i if i % 4 == 0 else "r%d" % i] + row)).encode() + (b"\r\n" if i % 3 == 0 else b"\n"))
        if i % 5 == 4:
            out.append(b"\r\n" if i % 2 else b"\n")
    with open(path, "wb") as fh:
        fh.write(b"".join(out))
    return path


def selections(n_cols, seed):
    rng = np.random.default_rng(seed)
    ident = list(range(n_cols))
    out = {"first": [0], "last": [n_cols - 1], "identity": ident, "reversed": ident[::-1], "block": rsr.deal(n_cols, 3, 1, "block") or [0]}
    for size in (1, 64, 65):
        if size <= n_cols:
            out[f"size{size}"] = sorted(rng.permutation(n_cols)[:size].tolist())
    for world in (2, 3, 8):
        for rank in range(min(world, n_cols)):
            out[f"cyclic{world}.{rank}"] = rsr.deal(n_cols, world, rank, "cyclic")
    out["shuffled"] = rng.permutation(n_cols)[:max(1, (2 * n_cols) // 3)].tolist()
    return out


@pytest.mark.parametrize("n_rows", [1, 65, 200])
@pytest.mark.parametrize("n_cols", [1, 2, 63, 64, 65, 130])
def test_selected_table_equals_the_gathered_full_read(dev, tmp_path, n_cols, n_rows):
    for corner in (False, True):
        path = write_table(str(tmp_path / f"t{int(corner)}.tsv"), n_rows, n_cols, corner, seed=1000 * n_cols + n_rows)
        table = cor.read_table(path)
        rows, cols, full, _ = dev.read_table(path)
        assert np.array_equal(bits(full), rsr.table_slice(table, range(n_cols)))
        for name, sel in selections(n_cols, n_cols + n_rows).items():
            for chunk in ((64, 4096) if name in ("identity", "reversed", "cyclic3.0", "shuffled", "last") else (4096,)):
                got_rows, got_cols, x, stats = dev.read_table(path, chunk_bytes=chunk, cells=sel)
                assert (got_rows, got_cols) == (rows, cols) == (table[0], table[1]), name
                assert tuple(x.shape) == (len(sel), n_rows) and x.is_contiguous()
                assert np.array_equal(bits(x), bits(dev.gather_matrix(full, cells=sel))), (name, chunk)
                assert np.array_equal(bits(x), rsr.table_slice(table, sel)), (name, chunk)
                assert stats["fields"] == n_rows * len(sel) and stats["rows"] == n_rows
                if name == "identity":
                    assert np.array_equal(bits(x), bits(full))
                if chunk == 64 and n_rows > 1:
                    assert stats["chunks"] > 1


def test_chunk_boundaries_inside_the_table_and_past_a_segment(dev, tmp_path):
    """One chunk of 200 rows x 130 columns covers several 4096-byte segments; 4096-byte chunks split inside the table."""
    path = write_table(str(tmp_path / "seg.tsv"), 200, 130, True, seed=5)
    assert os.path.getsize(path) > 5 * 4096
    table = cor.read_table(path)
    sel = rsr.deal(130, 8, 3, "cyclic")
    for chunk, chunks in ((4096, None), (None, 1)):
        _, _, x, stats = dev.read_table(path, chunk_bytes=chunk, cells=sel)
        assert np.array_equal(bits(x), rsr.table_slice(table, sel))
        assert stats["chunks"] == chunks if chunks else stats["chunks"] > 5


def test_uncertified_fields_count_only_where_they_are_selected(dev, tmp_path):
    path = write_table(str(tmp_path / "tie.tsv"), 9, 7, False, seed=3, patch={(4, 2): TIE})
    _, _, x, stats = dev.read_table(path, cells=[0, 1, 3, 6])
    assert stats["host_parsed"] == 0 and stats["fields"] == 9 * 4
    _, _, x, stats = dev.read_table(path, cells=[5, 2])
    assert stats["host_parsed"] == 1 and stats["fields"] == 9 * 2
    assert float(x[1, 4]) == float(TIE) and np.array_equal(bits(x), rsr.read_table_cols(path, [5, 2])[2])


def test_more_uncertified_selected_fields_than_one_round_lists(dev, tmp_path):
    """9000 rows x 16 columns of exact ties, 8 columns selected: 72 000 flagged fields, the list holds 65 536."""
    line = "\t".join([TIE] * 16) + "\n"
    path = str(tmp_path / "ties.tsv")
    with open(path, "w") as fh:
        fh.write("\t".join(f"c{j}" for j in range(16)) + "\n" + "".join(f"r{i}\t{line}" for i in range(9000)))
    _, _, x, stats = dev.read_table(path, cells=list(range(1, 16, 2)))
    assert stats["chunks"] == 1 and stats["host_parsed"] == 72000 and stats["collect_rounds"] == 1 and stats["fields"] == 72000
    assert tuple(x.shape) == (8, 9000) and bool((x == float(TIE)).all())


def test_refusals_of_the_selected_table_read(dev, tmp_path):
    good = write_table(str(tmp_path / "good.tsv"), 12, 9, True, seed=8)
    bad = write_table(str(tmp_path / "bad.tsv"), 12, 9, True, seed=8, patch={(7, 4): "12x"})
    with pytest.raises(_lib.IcnvError) as plain:
        dev.read_table(bad)
    assert "line " in str(plain.value) and "field 6" in str(plain.value) and "'12x'" in str(plain.value)
    for chunk in (64, None):
        with pytest.raises(_lib.IcnvError) as got:
            dev.read_table(bad, cells=[8, 4, 0], chunk_bytes=chunk)
        assert got.value.code == _lib.ERR_ARG and str(got.value) == str(plain.value)
        # the same byte in a skipped column: nothing is raised, the result is the slice
        sel = [8, 5, 0, 3]
        _, _, x, _ = dev.read_table(bad, cells=sel, chunk_bytes=chunk)
        assert np.array_equal(bits(x), rsr.table_slice(cor.read_table(good), sel))
        assert np.array_equal(bits(x), rsr.read_table_cols(bad, sel)[2])
    # a ragged row is refused as the plain read refuses it, whatever is selected
    with open(good, "rb") as fh:
        lines = fh.read().split(b"\n")
    assert lines[3].startswith(b"r2\t") and not lines[3].endswith(b"\r")
    lines[3] = lines[3].rsplit(b"\t", 1)[0]                                   # row r2 loses its last field
    ragged = str(tmp_path / "ragged.tsv")
    with open(ragged, "wb") as fh:
        fh.write(b"\n".join(lines))
    with pytest.raises(_lib.IcnvError) as plain:
        dev.read_table(ragged)
    assert "the row has 9 fields, 10 are expected" in str(plain.value)
    for sel in ([0], [8], [3, 1], list(range(9))):
        with pytest.raises(_lib.IcnvError) as got:
            dev.read_table(ragged, cells=sel)
        assert str(got.value) == str(plain.value)


def test_cells_argument_errors(dev, tmp_path):
    path = write_table(str(tmp_path / "t.tsv"), 3, 5, False, seed=1)
    for cells, text in (([], "non-empty"), ([1, 1], "column 1 more than once"), ([-1], "entry -1 is negative")):
        with pytest.raises(ValueError, match=text):
            dev.read_table(str(tmp_path / "absent.tsv"), cells=cells)
        with pytest.raises(ValueError, match=text):
            dev.read_mtx(str(tmp_path / "absent.mtx"), cells=cells)
    with pytest.raises(ValueError, match="read_table: cells entry 5 is not a column of the file, which has 5"):
        dev.read_table(path, cells=[0, 5])
    mtx = str(tmp_path / "m.mtx")
    scr.write_mtx(mtx, np.eye(4, 6, dtype=np.int64))
    with pytest.raises(ValueError, match="read_mtx: cells entry 9 is not a column of the file, which has 6"):
        dev.read_mtx(mtx, cells=[2, 9])


BAD_MAPS = [
    ([0, 1, 1, -1, 2], 3, "entry 2 of the column map names an output column a second time"),
    ([0, 3, 1, -1, 2], 3, "entry 1 of the column map is outside -1 .. n_cols_out - 1"),
    ([0, -2, 1, -1, 2], 3, "entry 1 of the column map is outside -1 .. n_cols_out - 1"),
    ([0, -1, 2, -1, -1], 3, "output column 1 is hit by no entry of the column map"),
]


@pytest.mark.parametrize("col_map,n_out,text", BAD_MAPS)
def test_bad_maps_are_refused_through_the_c_abi(dev, col_map, n_out, text):
    L = _lib.load()
    stream = ct.c_void_p(torch.cuda.current_stream().cuda_stream)
    cmap = torch.tensor(col_map, dtype=torch.int32, device="cuda")
    # dense
    text_host = np.frombuffer(b"r0\t1\t2\t3\t4\t5\nr1\t6\t7\t8\t9\t10\n", dtype=np.uint8).copy()
    text_dev = torch.from_numpy(text_host).cuda()
    out = torch.full((n_out, 4), -77.0, dtype=torch.float64, device="cuda")
    ranges, n_rows = np.full(8, -5, dtype=np.int64), ct.c_int64(-5)
    rc = L.icnv_parse_table_cols_dev(ct.c_void_p(text_dev.data_ptr()), ct.c_void_p(text_host.ctypes.data), text_host.size, b"\t", 5, 1,
                                     ct.c_void_p(out.data_ptr()), 4, 0, 4, ranges.ctypes.data_as(ct.POINTER(ct.c_int64)), ct.byref(n_rows),
                                     ct.c_void_p(cmap.data_ptr()), n_out, stream)
    assert rc == _lib.ERR_ARG and L.icnv_last_error().decode().endswith("parse_table_cols: " + text)
    assert bool((out == -77.0).all()) and n_rows.value == -5 and (ranges == -5).all()
    # triplets
    body = np.frombuffer(b"1 1 5\n2 3 6\n3 5 7\n", dtype=np.uint8).copy()
    body_dev = torch.from_numpy(body).cuda()
    arrays = [torch.full((4,), -77, dtype=torch.int32, device="cuda") for _ in range(3)]
    kept, seen = ct.c_int64(-5), ct.c_int64(-5)
    rc = L.icnv_parse_triplets_cols_dev(ct.c_void_p(body_dev.data_ptr()), ct.c_void_p(body.ctypes.data), body.size, _lib.MM_INTEGER, 3, 5, 1,
                                        *(ct.c_void_p(t.data_ptr()) for t in arrays), 4, ct.byref(kept), ct.c_void_p(cmap.data_ptr()), n_out,
                                        ct.byref(seen), stream)
    assert rc == _lib.ERR_ARG and L.icnv_last_error().decode().endswith("parse_triplets_cols: " + text)
    assert all(bool((t == -77).all()) for t in arrays) and (kept.value, seen.value) == (-5, -5)


def test_a_good_map_through_the_c_abi_and_a_short_capacity(dev):
    body = np.frombuffer(b"1 1 5\n2 3 6\n3 5 7\n1 4 8\n", dtype=np.uint8).copy()
    body_dev = torch.from_numpy(body).cuda()
    cmap = torch.tensor([1, -1, -1, 2, 0], dtype=torch.int32, device="cuda")
    row, col, val = (torch.full((5,), -77, dtype=torch.int32, device="cuda") for _ in range(3))
    with pytest.raises(_lib.IcnvError, match="parse_triplets_cols: 3 entries are kept, capacity is 2"):
        dev.parse_triplets_cols_into(body_dev, body, body.size, _lib.MM_INTEGER, 3, 5, row, col, val, 3, cmap, 3)
    assert bool((row == -77).all())
    assert dev.parse_triplets_cols_into(body_dev, body, body.size, _lib.MM_INTEGER, 3, 5, row, col, val, 1, cmap, 3) == (3, 4)
    assert row.tolist() == [-77, 0, 2, 0, -77] and col.tolist() == [-77, 1, 0, 2, -77] and val.tolist() == [-77, 5, 7, 8, -77]


# ---------------------------------------------------------------------------------------------------------------- MatrixMarket
SPELLINGS = (b"%d", b"+%d", b"%d.0", b"%de0", b"%.15e")


def csc_arrays(counts):
    return tuple(t.cpu().numpy() for t in counts.t[1:])


@pytest.fixture(scope="module")
def mtx_files(dev, tmp_path_factory):
    """The 37 x 29 edge file of tests/test_gpu_sparse_counts.py (every spelling, varied blanks, "\\r\\n", blank lines, no final
    terminator) with two empty columns; a file of more than 4096 entries; the same shuffled.  Each is read in full once."""
    d = tmp_path_factory.mktemp("read_select_mtx")
    rng = np.random.default_rng(22)
    m = rng.integers(1, 500, size=(37, 29)) * (rng.random((37, 29)) < 0.3)
    m[0, 0], m[36, 0], m[0, 28], m[36, 28], m[5, 3] = 7, 8, 9, 10, 2147483647
    m[:, 11] = 0
    m[:, 20] = 0
    edge = str(d / "edge.mtx")
    scr.write_mtx(edge, m, field="real", spell=lambda k, v: SPELLINGS[k % 5] % v, gaps=(b" ", b"\t", b"   ", b" \t "), edge_blanks=True,
                  eol=lambda k: b"\r\n" if k % 5 == 0 else b"\n", blank_every=7, final_newline=False)
    big_m = rng.integers(1, 3000, size=(150, 97)) * (rng.random((150, 97)) < 0.4)
    big, shuffled = str(d / "big.mtx"), str(d / "shuffled.mtx")
    assert len(scr.write_mtx(big, big_m)) > 4096
    scr.write_mtx(shuffled, big_m, order="shuffle", seed=4)
    return {name: {"path": p, "full": dev.read_mtx(p)[0], "C": c, "G": g}
            for name, p, g, c in (("edge", edge, 37, 29), ("big", big, 150, 97), ("shuffled", shuffled, 150, 97))}


def mtx_selections(C):
    out = {"block": rsr.deal(C, 3, 2, "block"), "reversed": list(range(C))[::-1], "identity": list(range(C))}
    for world in (2, 3, 8):
        for rank in range(world):
            out[f"cyclic{world}.{rank}"] = rsr.deal(C, world, rank, "cyclic")
    return out


@pytest.mark.parametrize("name", ["edge", "big", "shuffled"])
def test_selected_mtx_equals_the_selected_full_read(dev, mtx_files, name):
    f = mtx_files[name]
    G, C = f["G"], f["C"]
    n_file = rsr.mtx_entries(f["path"])[2]
    for label, sel in mtx_selections(C).items():
        for chunk in ((64, None) if label in ("cyclic3.1", "reversed") and name != "shuffled" else (None,)):
            counts, stats = dev.read_mtx(f["path"], chunk_bytes=chunk, cells=sel)
            colptr, rowidx, vals, sorted_already, kept = rsr.mtx_slice(f["path"], sel)
            got = csc_arrays(counts)
            assert (counts.G, counts.C) == (G, len(sel)), label
            assert np.array_equal(got[0], colptr) and np.array_equal(got[1], rowidx) and np.array_equal(got[2], vals), (label, chunk)
            want = csc_arrays(dev.csc_select(f["full"], np.arange(G), sel))
            assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got, want)), (label, chunk)
            assert stats["entries"] == n_file and stats["entries_kept"] == kept == len(vals)
            assert stats["sorted_on_device"] == (0 if sorted_already else 1)
            if label == "reversed":
                assert stats["sorted_on_device"] == 1
            if label.startswith("cyclic") and name != "shuffled":
                assert stats["sorted_on_device"] == 0


def test_empty_columns_of_a_selected_mtx(dev, mtx_files):
    f = mtx_files["edge"]
    counts, stats = dev.read_mtx(f["path"], cells=[10, 11, 12])                   # a column with no entries in the middle
    colptr, rowidx, vals, _, kept = rsr.mtx_slice(f["path"], [10, 11, 12])
    got = csc_arrays(counts)
    assert np.array_equal(got[0], colptr) and np.array_equal(got[1], rowidx) and np.array_equal(got[2], vals)
    assert colptr[1] == colptr[2] and kept > 0
    counts, stats = dev.read_mtx(f["path"], cells=[20, 11], chunk_bytes=64)       # every selected column is empty
    got = csc_arrays(counts)
    assert (counts.G, counts.C, counts.nnz) == (37, 2, 0) and got[0].tolist() == [0, 0, 0] and got[1].size == got[2].size == 0
    assert stats["entries_kept"] == 0 and stats["entries"] == rsr.mtx_entries(f["path"])[2] and stats["sorted_on_device"] == 0


def test_triplet_arrays_grow_when_a_selection_keeps_more_than_its_share(dev, tmp_path):
    """One full column among sparse ones: the selection's share of the size line's count is less than the column holds."""
    rng = np.random.default_rng(7)
    m = rng.integers(1, 9, size=(3000, 50)) * (rng.random((3000, 50)) < 0.05)
    m[:, 7] = rng.integers(1, 9, size=3000)
    path = str(tmp_path / "skew.mtx")
    n = len(scr.write_mtx(path, m))
    assert n // 50 + n // 8 + 1024 < 3000
    for sel, chunk in (([7], None), ([30, 7], 4096)):
        counts, stats = dev.read_mtx(path, cells=sel, chunk_bytes=chunk)
        colptr, rowidx, vals, sorted_already, kept = rsr.mtx_slice(path, sel)
        got = csc_arrays(counts)
        assert np.array_equal(got[0], colptr) and np.array_equal(got[1], rowidx) and np.array_equal(got[2], vals)
        assert stats["arrays_grown"] >= 1 and stats["entries"] == n and stats["entries_kept"] == kept >= 3000
        assert stats["sorted_on_device"] == (0 if sorted_already else 1)
    assert dev.read_mtx(path, cells=[3, 4])[1]["arrays_grown"] == 0


def test_refusals_of_the_selected_mtx_read(dev, tmp_path):
    good = [b"%d %d %d" % (1 + k % 37, 1 + k // 37, k + 1) for k in range(40)]                # columns 1 and 2 only
    body = b"\n".join(good[:25]) + b"\n\r\n" + b"2 2 0.5" + b"\r\n" + b"\n".join(good[25:]) + b"\n"
    path = str(tmp_path / "bad.mtx")
    with open(path, "wb") as fh:
        fh.write(b"%%MatrixMarket matrix coordinate integer general\n% one\n37 29 41\n" + body)
    with pytest.raises(_lib.IcnvError) as plain:
        dev.read_mtx(path)
    assert "line 30, field 3: not an integer count" in str(plain.value)
    for sel, chunk in (([0, 5], None), ([5, 7], 64), ([1], None)):                            # column 2 skipped, skipped, selected
        with pytest.raises(_lib.IcnvError) as got:
            dev.read_mtx(path, cells=sel, chunk_bytes=chunk)
        assert got.value.code == _lib.ERR_ARG and str(got.value) == str(plain.value)
    for said in (41, 39):                                                                     # the count of entries SEEN is checked
        with open(path, "wb") as fh:
            fh.write(b"%%MatrixMarket matrix coordinate integer general\n37 29 " + str(said).encode() + b"\n" + b"\n".join(good) + b"\n")
        with pytest.raises(ValueError, match=f"read_mtx: the size line says {said} entries, the body has 40"):
            dev.read_mtx(path, cells=[3, 4])


# ---------------------------------------------------------------------------------------------------------------- ShardedCreate
@pytest.fixture(scope="module")
def example(golden_dir, tmp_path_factory):
    d = os.path.join(golden_dir, "create_object_example")
    out = tmp_path_factory.mktemp("read_select_example")
    plain = str(out / "counts.matrix")
    with gzip.open(os.path.join(d, "counts_every_8th_gene.matrix.gz"), "rb") as src, open(plain, "wb") as dst:
        dst.write(src.read())
    genes, cells, x_bits = cor.read_table(plain)
    mtx = str(out / "counts.mtx")
    scr.write_mtx(mtx, np.rint(cor.as_double(x_bits)).astype(np.int64))       # a count table: the example's values are not integers
    return {"dense": plain, "mtx": mtx, "genes": genes, "cells": cells,
            "order": os.path.join(d, "gencode_downsampled.EXAMPLE_ONLY_DONT_REUSE.txt.gz"),
            "annot": os.path.join(d, "oligodendroglioma_annotations_downsampled.txt.gz")}


@pytest.fixture(scope="module")
def singles(dev, example):
    """The single-rank CreateInfercnvObject results the sharded ones are held to, made once per (route, options)."""
    made = {}

    def get(route, kw):
        key = (route, tuple(sorted((k, str(v)) for k, v in kw.items())))
        if key not in made:
            names = dict(gene_names=example["genes"], cell_names=example["cells"]) if route == "mtx" else {}
            made[key] = infercnv_amd.CreateInfercnvObject(example[route], example["order"], example["annot"], REFS, return_device=True,
                                                          **names, **kw)
        return made[key]
    return get


OPTIONS = [dict(), dict(max_cells_per_group=20, seed=3), dict(min_max_counts_per_cell=(8000, 12000))]


@pytest.mark.parametrize("kw", OPTIONS)
@pytest.mark.parametrize("route", ["dense", "mtx"])
def test_sharded_create_equals_the_single_rank_object(dev, example, singles, route, kw):
    single, x_single = singles(route, kw)
    names = dict(gene_names=example["genes"], cell_names=example["cells"]) if route == "mtx" else {}
    C_file = len(example["cells"])
    if "min_max_counts_per_cell" in kw:
        assert len(single.cell_names) < C_file                                  # the filter drops cells
    for world in (1, 2, 3):
        for how in ("cyclic", "block"):
            ranks = [sharded.ShardedCreate(example[route], example["order"], example["annot"], REFS, rank=r, world=world, deal=how,
                                           **names, **kw) for r in range(world)]
            sums = ranks[0].place([sc.read() for sc in ranks])
            shards = [sc.finish(sums) for sc in ranks]
            rsr.check_shards(single, shards, C_file, world, how)
            for _, x_local, shard in shards:
                J = shard["global_index"]
                if route == "mtx":
                    want = csc_arrays(dev.csc_select(x_single, np.arange(x_single.G), J))
                    assert all(np.array_equal(a, b) for a, b in zip(csc_arrays(x_local), want))
                else:
                    assert np.array_equal(bits(x_local), bits(x_single)[J])
            if world == 3 and how == "cyclic":                                   # the gathered sums are the single rank's, exactly
                from infercnv_amd import create_object as co
                rows = co.order_reduce(example["genes"], co.read_gene_order(example["order"]))[0]
                if route == "mtx":
                    full = dev.ingest_col_sums(dev.read_mtx(example["mtx"])[0], rows)
                else:
                    full = dev.col_sums(dev.gather_matrix(dev.read_table(example["dense"])[2], genes=rows))
                assert np.array_equal(sums.view(np.int64), full.cpu().numpy().view(np.int64))


@pytest.mark.parametrize("route", ["dense", "mtx"])
def test_run_without_a_process_group_is_create_infercnv_object(dev, example, singles, route):
    kw = OPTIONS[1]
    single, x_single = singles(route, kw)
    names = dict(gene_names=example["genes"], cell_names=example["cells"]) if route == "mtx" else {}
    obj, x, shard = sharded.ShardedCreate(example[route], example["order"], example["annot"], REFS, rank=0, world=1, **names, **kw).run()
    rsr.same_object(obj, single)
    assert obj.count_data is obj.expr_data and type(obj.expr_data) is type(single.expr_data)
    assert shard["global_index"].tolist() == list(range(len(single.cell_names))) and shard["C_total"] == len(single.cell_names)
    if route == "mtx":
        assert all(np.array_equal(a, b) for a, b in zip(csc_arrays(x), csc_arrays(x_single)))
    else:
        assert np.array_equal(bits(x), bits(x_single))
