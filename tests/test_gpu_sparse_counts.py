"""Sparse count matrices on the GPU (include/icnv.h "sparse count matrices", DESIGN K22): the triplet parser, the CSC builder,
the CSC selector and the sparse route of CreateInfercnvObject against the restatement of tests/sparse_counts_restate.py.  Bit
equality throughout.  The example's matrix holds values that are not integers, which the sparse route refuses; both routes get
its values rounded to integers."""
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
SPELLINGS = (b"%d", b"+%d", b"%d.0", b"%de0", b"%.15e")
BANNER = b"%%MatrixMarket matrix coordinate integer general\n"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infercnv_amd import device
    torch.cuda.set_device(0)
    device.init(0)
    return device


def arrays(counts):
    return tuple(t.cpu().numpy() for t in counts.t[1:])


def same_csc(counts, G, C, colptr, rowidx, vals):
    got = arrays(counts)
    assert (counts.G, counts.C) == (G, C)
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.int32
    assert np.array_equal(got[0], colptr) and np.array_equal(got[1], rowidx) and np.array_equal(got[2], vals)


def read_both(dev, path, **kw):
    counts, stats = dev.read_mtx(path, **kw)
    G, C, colptr, rowidx, vals, sorted_already = scr.read_mtx(path)
    same_csc(counts, G, C, colptr, rowidx, vals)
    assert stats["sorted_on_device"] == (0 if sorted_already else 1) and stats["entries"] == len(vals)
    return counts, stats


# ---- parser edge shapes ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_file(tmp_path_factory):
    """37 x 29 at about 30 %: the corners, an explicit 0, 2147483647, every spelling, varied blanks, "\\r\\n" and blank lines
    scattered, no terminator on the last line."""
    rng = np.random.default_rng(22)
    m = rng.integers(1, 500, size=(37, 29)) * (rng.random((37, 29)) < 0.3)
    m[0, 0], m[36, 0], m[0, 28], m[36, 28], m[5, 3] = 7, 8, 9, 10, 2147483647
    m[9, 4] = 0
    d = tmp_path_factory.mktemp("edge")
    kw = dict(field="real", spell=lambda k, v: SPELLINGS[k % 5] % v, gaps=(b" ", b"\t", b"   ", b" \t "), edge_blanks=True,
              eol=lambda k: b"\r\n" if k % 5 == 0 else b"\n", blank_every=7, final_newline=False, keep_zero=[(9, 4)])
    plain, gz = str(d / "edge.mtx"), str(d / "edge.mtx.gz")
    entries = scr.write_mtx(plain, m, **kw)
    scr.write_mtx(gz, m, **kw)
    assert (9, 4, 0) in entries and os.path.getsize(plain) > 4096 and not open(plain, "rb").read().endswith(b"\n")
    return {"plain": plain, "gz": gz, "dense": m}


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    """700 x 400 at about 25 %: some 70 000 entries, more than one workgroup in every pass and more than 65 536 entries in one
    chunk.  The restatement's reading is shared by the tests."""
    rng = np.random.default_rng(23)
    m = rng.integers(1, 3000, size=(700, 400)) * (rng.random((700, 400)) < 0.25)
    path = str(tmp_path_factory.mktemp("big") / "big.mtx")
    entries = scr.write_mtx(path, m, spell=lambda k, v: SPELLINGS[k % 3] % v)
    assert len(entries) > 65536
    return {"path": path, "dense": m, "csc": scr.read_mtx(path)}


@pytest.mark.parametrize("chunk", [64, 100, 4096, None])
def test_edge_file_in_chunks(dev, edge_file, chunk):
    counts, stats = read_both(dev, edge_file["plain"], chunk_bytes=chunk)
    assert np.array_equal(counts.to_dense().cpu().numpy().T, edge_file["dense"].astype(np.float64))
    assert stats["chunks"] >= (2 if chunk else 1) and stats["sorted_on_device"] == 0


def test_gz_of_the_edge_file(dev, edge_file):
    read_both(dev, edge_file["gz"], chunk_bytes=1000)


def test_big_file_in_one_chunk(dev, big):
    counts, stats = dev.read_mtx(big["path"])
    same_csc(counts, *big["csc"][:5])
    assert stats["chunks"] == 1 and stats["entries"] > 65536 and stats["sorted_on_device"] == 0


def test_pattern_file(dev, edge_file, tmp_path):
    path = str(tmp_path / "p.mtx")
    scr.write_mtx(path, edge_file["dense"], field="pattern", gaps=(b" ", b"\t\t"), blank_every=9)
    counts, _ = read_both(dev, path)
    assert set(arrays(counts)[2].tolist()) == {1}


REFUSED_LINES = [
    (b"0 2 4", "field 1: not an index in 1 .. 37: '0'"),
    (b"38 2 4", "field 1: not an index in 1 .. 37: '38'"),
    (b"2 30 4", "field 2: not an index in 1 .. 29: '30'"),
    (b"2 2 -1", "field 3: not an integer count in 0 .. 2147483647: '-1'"),
    (b"2 2 0.5", "field 3: not an integer count in 0 .. 2147483647: '0.5'"),
    (b"2 2 2147483648", "field 3: not an integer count in 0 .. 2147483647: '2147483648'"),
    (b"2 2", "field 2: 2 fields where 3 are expected: '2 2'"),
    (b"% a comment", "field 1: a comment line inside the body: '% a comment'"),
]


@pytest.mark.parametrize("bad,text", REFUSED_LINES)
@pytest.mark.parametrize("chunk", [64, None])
def test_refusals_name_line_and_field(dev, tmp_path, bad, text, chunk):
    good = [b"%d %d %d" % (1 + k % 37, 1 + k // 37, k + 1) for k in range(40)]
    body = b"\n".join(good[:25]) + b"\n\r\n" + bad + b"\r\n" + b"\n".join(good[25:]) + b"\n0 0 0\n"       # a later refusal loses
    path = str(tmp_path / "bad.mtx")
    with open(path, "wb") as fh:
        fh.write(BANNER + b"% one\n% two\n37 29 42\n" + body)
    with pytest.raises(scr.Refusal) as want:
        scr.read_mtx(path)
    assert str(want.value) == "line 31, " + text
    with pytest.raises(_lib.IcnvError) as got:
        dev.read_mtx(path, chunk_bytes=chunk)
    assert got.value.code == _lib.ERR_ARG and str(got.value).endswith("parse_triplets: " + str(want.value))


@pytest.mark.parametrize("said", [41, 39])
def test_size_line_that_miscounts(dev, tmp_path, said):
    path = str(tmp_path / "count.mtx")
    with open(path, "wb") as fh:
        fh.write(BANNER + b"37 29 %d\n" % said + b"".join(b"%d %d 5\n" % (1 + k % 37, 1 + k // 37) for k in range(40)))
    with pytest.raises(ValueError, match=f"the size line says {said} entries, the body has 40"):
        dev.read_mtx(path)
    with pytest.raises(ValueError, match=f"the size line says {said} entries, the body has 40"):
        scr.read_mtx(path)


def test_outputs_are_untouched_by_a_refused_chunk_and_capacity_is_kept(dev):
    text = b"1 1 5\n2 1 6\n3 1 x\n"
    host = np.frombuffer(text, dtype=np.uint8).copy()
    t = torch.from_numpy(host).cuda()
    row, col, val = (torch.full((4,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    with pytest.raises(_lib.IcnvError, match="line 3, field 3"):
        dev.parse_triplets_into(t, host, len(text), _lib.MM_INTEGER, 5, 5, row, col, val, 0)
    with pytest.raises(_lib.IcnvError, match="the chunk has 2 entries, capacity is 1"):
        dev.parse_triplets_into(t, host, 12, _lib.MM_INTEGER, 5, 5, row, col, val, 3)
    assert all(v.tolist() == [-7] * 4 for v in (row, col, val))
    assert dev.parse_triplets_into(t, host, 12, _lib.MM_INTEGER, 5, 5, row, col, val, 1) == 2
    assert row.tolist() == [-7, 0, 1, -7] and col.tolist() == [-7, 0, 0, -7] and val.tolist() == [-7, 5, 6, -7]


# ---- CSC build ------------------------------------------------------------------------------------------------------------
def test_shuffled_entries_take_the_sort_route(dev, tmp_path):
    rng = np.random.default_rng(31)
    m = rng.integers(1, 50, size=(61, 33)) * (rng.random((61, 33)) < 0.4)
    m[:, [0, 14, 15, 16, 32]] = 0                       # columns 0, a middle run of three and C - 1 are empty
    a, b = str(tmp_path / "sorted.mtx"), str(tmp_path / "shuffled.mtx")
    scr.write_mtx(a, m)
    scr.write_mtx(b, m, order="shuffle", seed=5)
    ca, sa = read_both(dev, a)
    cb, sb = read_both(dev, b)
    assert (sa["sorted_on_device"], sb["sorted_on_device"]) == (0, 1)
    for x, y in zip(arrays(ca), arrays(cb)):
        assert np.array_equal(x, y)
    colptr = arrays(ca)[0]
    assert colptr[1] == 0 and colptr[14] == colptr[17] and colptr[32] == colptr[33] == ca.nnz


def test_one_full_column_one_column_and_no_entry(dev, tmp_path):
    full = np.zeros((1500, 3), dtype=np.int64)
    full[:, 1] = np.arange(1, 1501)                     # one column holds all G entries, more than a workgroup
    path = str(tmp_path / "full.mtx")
    scr.write_mtx(path, full)
    counts, _ = read_both(dev, path)
    assert arrays(counts)[0].tolist() == [0, 0, 1500, 1500]
    scr.write_mtx(path, np.arange(1, 8).reshape(7, 1))  # C = 1
    read_both(dev, path)
    scr.write_mtx(path, np.zeros((4, 6), dtype=np.int64))
    counts, stats = read_both(dev, path)                # nnz = 0
    assert counts.nnz == 0 and arrays(counts)[0].tolist() == [0] * 7 and stats["entries"] == 0
    assert counts.to_scipy().shape == (4, 6) and counts.to_dense().abs().sum().item() == 0


def test_duplicate_pair_is_refused_with_its_row_and_column(dev, tmp_path):
    for name, body in (("adjacent", b"1 1 5\n3 2 6\n3 2 7\n4 4 1\n"), ("apart", b"3 2 6\n1 1 5\n4 4 1\n3 2 7\n")):
        path = str(tmp_path / (name + ".mtx"))
        with open(path, "wb") as fh:
            fh.write(BANNER + b"4 4 4\n" + body)
        with pytest.raises(ValueError, match="duplicate entry for row 3, column 2"):
            dev.read_mtx(path)
        with pytest.raises(ValueError, match="duplicate entry for row 3, column 2"):
            scr.read_mtx(path)


def test_build_reports_the_first_violation(dev):
    row = torch.tensor([0, 2, 1, 1, 0], dtype=torch.int32, device="cuda")
    col = torch.tensor([0, 0, 1, 1, 0], dtype=torch.int32, device="cuda")
    assert dev.csc_from_sorted_triplets(row, col, 3, 2)[1:] == (3, _lib.CSC_DUPLICATE)
    assert dev.csc_from_sorted_triplets(row[[0, 1, 2, 4]].contiguous(), col[[0, 1, 2, 4]].contiguous(), 3, 2)[1:] == (3, _lib.CSC_DESCENT)
    colptr, first, kind = dev.csc_from_sorted_triplets(row[:3].contiguous(), col[:3].contiguous(), 3, 4)
    assert (first, kind) == (-1, _lib.CSC_SORTED) and colptr.tolist() == [0, 2, 3, 3, 3]
    with pytest.raises(_lib.IcnvError, match="entry 1 lies outside the matrix"):
        dev.csc_from_sorted_triplets(row[:3].contiguous(), col[:3].contiguous(), 2, 4)


# ---- selection ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_counts(dev, big):
    counts, _ = dev.read_mtx(big["path"])
    dense = torch.from_numpy(np.ascontiguousarray(big["dense"].T.astype(np.float64))).cuda()
    return counts, dense


def drop_column_5(big):
    _, _, colptr, rowidx, _, _ = big["csc"]
    gone = set(rowidx[colptr[5]:colptr[6]].tolist())
    return [g for g in range(700) if g not in gone]


SELECTIONS = {
    "genes reversed": lambda big: (list(range(699, -1, -1)), list(range(400))),
    "every third gene": lambda big: (list(range(0, 700, 3)), list(range(400))),
    "a column loses every entry": lambda big: (drop_column_5(big), list(range(400))),
    "cells descending": lambda big: (list(range(700)), list(range(399, -1, -1))),
    "a repeated cell": lambda big: (list(range(1, 700, 2)), [7, 3, 7, 399, 0, 7]),
    "identity": lambda big: (list(range(700)), list(range(400))),
}


@pytest.mark.parametrize("case", list(SELECTIONS))
def test_selection_equals_the_restatement(dev, big, big_counts, case):
    counts, dense = big_counts
    genes, cells = SELECTIONS[case](big)
    G, C, colptr, rowidx, vals, _ = big["csc"]
    want = scr.select(colptr, rowidx, vals, G, genes, cells)
    got = dev.csc_select(counts, genes, cells)
    same_csc(got, len(genes), len(cells), *want)
    if case == "a column loses every entry":
        assert want[0][5] == want[0][6] and colptr[5] < colptr[6]
    assert torch.equal(got.to_dense(), dev.gather_matrix(dense, genes=genes, cells=cells))


def test_selection_refuses_bad_maps(dev, big_counts):
    counts, _ = big_counts
    L = _lib.load()
    import ctypes as ct
    gm = torch.full((700,), -1, dtype=torch.int32, device="cuda")
    cells = torch.tensor([1, 400, 2], dtype=torch.int32, device="cuda")
    colptr = torch.full((4,), -5, dtype=torch.int64, device="cuda")
    nnz = ct.c_int64(-9)

    def call(n_genes_out):
        return L.icnv_csc_select_dev(ct.byref(counts.c), 700, 400, ct.c_void_p(gm.data_ptr()), n_genes_out, ct.c_void_p(cells.data_ptr()), 3,
                                     ct.c_void_p(colptr.data_ptr()), None, None, 0, ct.byref(nnz), None)
    assert call(5) == _lib.ERR_ARG and b"entry 1 of the cell list" in L.icnv_last_error()
    cells[1] = 3
    gm[9] = 5
    assert call(5) == _lib.ERR_ARG and b"entry 9 of the gene map" in L.icnv_last_error()
    assert colptr.tolist() == [-5] * 4 and nnz.value == -9
    with pytest.raises(ValueError, match="CSC form"):
        dev.csc_select(dev.DeviceCounts(2, 2, dense=torch.zeros((2, 2), dtype=torch.int32, device="cuda")), [0], [0])


def test_scipy_round_trip(dev, big):
    sp = pytest.importorskip("scipy.sparse")
    m = sp.csr_matrix(big["dense"])
    counts = dev.DeviceCounts.from_scipy(m)
    same_csc(counts, *big["csc"][:5])
    back = counts.to_scipy()
    assert back.dtype == np.float64 and (back != m.tocsc()).nnz == 0
    with pytest.raises(ValueError, match="sparse=False"):
        dev.DeviceCounts.from_scipy(m * 0.5)


# ---- end to end -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def example(golden_dir, tmp_path_factory):
    d = os.path.join(golden_dir, "create_object_example")
    genes, cells, x_bits = cor.read_table(os.path.join(d, "counts_every_8th_gene.matrix.gz"))
    x = np.rint(cor.as_double(x_bits))                  # a count table: the example's own values are not integers
    out = tmp_path_factory.mktemp("sparse_example")
    mtx, gz = str(out / "counts.mtx"), str(out / "counts.mtx.gz")
    scr.write_mtx(mtx, x.astype(np.int64))
    scr.write_mtx(gz, x.astype(np.int64))
    symbols = list(genes)
    symbols[11], symbols[500] = symbols[10], symbols[10]                 # a gene symbol three times
    tenx = out / "tenx"
    tenx.mkdir()
    scr.write_mtx(str(tenx / "matrix.mtx.gz"), x.astype(np.int64))
    with gzip.open(str(tenx / "features.tsv.gz"), "wt") as fh:
        fh.write("".join(f"ENSG{i:011d}\t{s}\tGene Expression\n" for i, s in enumerate(symbols)))
    with gzip.open(str(tenx / "barcodes.tsv.gz"), "wt") as fh:
        fh.write("".join(c + "\n" for c in cells))
    return {"mtx": mtx, "gz": gz, "tenx": str(tenx), "genes": genes, "cells": cells, "x": x, "symbols": symbols,
            "order": os.path.join(d, "gencode_downsampled.EXAMPLE_ONLY_DONT_REUSE.txt.gz"),
            "annot": os.path.join(d, "oligodendroglioma_annotations_downsampled.txt.gz")}


def same_objects(sparse_obj, dense_obj):
    """Every slot of the sparse route's object equals the dense route's, the matrices after toarray()."""
    a, b = sparse_obj, dense_obj
    assert a.count_data is a.expr_data and hasattr(a.expr_data, "tocsc") and a.expr_data.dtype == np.float64
    assert isinstance(b.expr_data, np.ndarray)
    assert np.array_equal(a.expr_data.toarray().view(np.int64), np.ascontiguousarray(b.expr_data).view(np.int64))
    assert list(a.gene_names) == list(b.gene_names) and list(a.cell_names) == list(b.cell_names)
    for slot in ("chr", "start", "stop"):
        assert list(getattr(a.gene_order, slot)) == list(getattr(b.gene_order, slot))
    for da, db in ((a.reference_grouped_cell_indices, b.reference_grouped_cell_indices),
                   (a.observation_grouped_cell_indices, b.observation_grouped_cell_indices)):
        assert list(da) == list(db) and all(np.array_equal(da[k], db[k]) and da[k].dtype == db[k].dtype for k in da)
    assert a.options == b.options and a.validate()


@pytest.mark.parametrize("kw", [dict(), dict(max_cells_per_group=20, min_max_counts_per_cell=(8000, 12000), chr_exclude=("chr1", "chrY"), seed=3)])
def test_mtx_routes_equal_the_dense_route_and_the_restatement(dev, example, kw):
    e = example
    dense = infercnv_amd.CreateInfercnvObject(e["x"], e["order"], e["annot"], REFS, gene_names=e["genes"], cell_names=e["cells"], **kw)
    want = cor.create_object(e["genes"], e["cells"], np.ascontiguousarray(e["x"]).view(np.int64), e["order"], e["annot"], REFS, **kw)
    cor.compare(dense, want)
    for path in (e["mtx"], e["gz"]):
        obj = infercnv_amd.CreateInfercnvObject(path, e["order"], e["annot"], REFS, gene_names=e["genes"], cell_names=e["cells"], **kw)
        same_objects(obj, dense)
        scr.compare(cor, obj, want)
    assert len(want["gene_names"]) > 1000 and len(want["cell_names"]) > 20


def test_tenx_directory_with_a_repeated_symbol(dev, example):
    e = example
    names = scr.make_unique(e["symbols"])
    assert names[11] == e["symbols"][10] + ".1" and names[500] == e["symbols"][10] + ".2"
    dense = infercnv_amd.CreateInfercnvObject(e["x"], e["order"], e["annot"], REFS, gene_names=names, cell_names=e["cells"])
    obj = infercnv_amd.CreateInfercnvObject(e["tenx"], e["order"], e["annot"], REFS)
    same_objects(obj, dense)
    assert not {names[11], names[500]} & set(obj.gene_names)             # the position table does not know the made names
    by_id = infercnv_amd.CreateInfercnvObject(e["tenx"], [(f"ENSG{i:011d}", "chr1", 10 * i + 1, 10 * i + 5) for i in range(0, 600, 2)],
                                              e["annot"], REFS, gene_column=1, min_max_counts_per_cell=None)
    assert list(by_id.gene_names) == [f"ENSG{i:011d}" for i in range(0, 600, 2)]


def test_names_from_tsv_files(dev, example, tmp_path):
    e = example
    g, c = tmp_path / "genes.tsv", tmp_path / "cells.tsv.gz"
    g.write_text("".join(f"id{i}\t{s}\n" for i, s in enumerate(e["genes"])))
    with gzip.open(str(c), "wt") as fh:
        fh.write("".join(x + "\n" for x in e["cells"]))
    a = infercnv_amd.CreateInfercnvObject(e["mtx"], e["order"], e["annot"], REFS, gene_names=str(g), cell_names=str(c))
    b = infercnv_amd.CreateInfercnvObject(e["mtx"], e["order"], e["annot"], REFS, gene_names=e["genes"], cell_names=e["cells"])
    assert list(a.gene_names) == list(b.gene_names) and (a.expr_data != b.expr_data).nnz == 0
    with pytest.raises(ValueError, match="gene_names and cell_names"):
        infercnv_amd.CreateInfercnvObject(e["mtx"], e["order"], e["annot"], REFS)
    with pytest.raises(ValueError, match="1293 x 184, but there are 1292 gene names"):
        infercnv_amd.CreateInfercnvObject(e["mtx"], e["order"], e["annot"], REFS, gene_names=e["genes"][1:], cell_names=e["cells"])


def test_device_counts_feed_the_ingest_bit_for_bit(dev, example):
    e = example
    obj, counts = infercnv_amd.CreateInfercnvObject(e["mtx"], e["order"], e["annot"], REFS, gene_names=e["genes"], cell_names=e["cells"],
                                                    return_device=True)
    assert isinstance(counts, dev.DeviceCounts) and (counts.G, counts.C) == obj.expr_data.shape and counts.nnz == obj.expr_data.nnz
    m = obj.expr_data.toarray()
    dense = dev.DeviceCounts(counts.G, counts.C, dense=torch.from_numpy(np.ascontiguousarray(m.T.astype(np.int32))).cuda())
    for kw in (dict(), dict(min_mean_expr_cutoff=0.1, min_cells_per_gene=3)):
        xs, keep_s, f_s = dev.ingest_counts(counts, **kw)
        xd, keep_d, f_d = dev.ingest_counts(dense, **kw)
        assert torch.equal(xs.view(torch.int64), xd.view(torch.int64)) and np.array_equal(keep_s, keep_d) and f_s == f_d
    from infercnv_amd import ops
    new, _ = ops.ingest_counts(obj)
    assert np.array_equal(np.ascontiguousarray(new.expr_data.T).view(np.int64), dev.ingest_counts(counts)[0].cpu().numpy().view(np.int64))


def test_sparse_false_and_scipy_input(dev, example):
    sp = pytest.importorskip("scipy.sparse")
    e = example
    kw = dict(gene_names=e["genes"], cell_names=e["cells"])
    dense = infercnv_amd.CreateInfercnvObject(e["x"], e["order"], e["annot"], REFS, **kw)
    off, x = infercnv_amd.CreateInfercnvObject(e["mtx"], e["order"], e["annot"], REFS, sparse=False, return_device=True, **kw)
    assert isinstance(off.expr_data, np.ndarray) and isinstance(x, torch.Tensor)
    cor.compare(off, cor.create_object(e["genes"], e["cells"], np.ascontiguousarray(e["x"]).view(np.int64), e["order"], e["annot"], REFS))
    assert np.array_equal(off.expr_data, dense.expr_data) and np.array_equal(x.cpu().numpy().T, dense.expr_data)
    m = sp.coo_matrix(e["x"])
    via_mtx = infercnv_amd.CreateInfercnvObject(e["mtx"], e["order"], e["annot"], REFS, **kw)
    kept = infercnv_amd.CreateInfercnvObject(m, e["order"], e["annot"], REFS, sparse=True, **kw)
    same_objects(kept, dense)
    assert (kept.expr_data != via_mtx.expr_data).nnz == 0
    assert np.array_equal(kept.expr_data.indices, via_mtx.expr_data.indices) and np.array_equal(kept.expr_data.indptr, via_mtx.expr_data.indptr)
    default = infercnv_amd.CreateInfercnvObject(m, e["order"], e["annot"], REFS, **kw)          # unchanged: densified by toarray()
    assert isinstance(default.expr_data, np.ndarray) and np.array_equal(default.expr_data, dense.expr_data)
    with pytest.raises(ValueError, match="sparse=False"):
        infercnv_amd.CreateInfercnvObject(m * 0.5, e["order"], e["annot"], REFS, sparse=True, **kw)
    with pytest.raises(ValueError, match="sparse=True wants"):
        infercnv_amd.CreateInfercnvObject(e["x"], e["order"], e["annot"], REFS, sparse=True, **kw)
