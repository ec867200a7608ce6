"""The host side of K22 (DESIGN K22) without a GPU: the restatement of tests/sparse_counts_restate.py against scipy's
MatrixMarket reader, every refusal with its text, make.unique, and the restated sparse route of CreateInfercnvObject against the
dense restatement on the example's inputs.  The library's own host pieces (the header reader, make_unique) are held to the
restatement here as well; its kernels are in tests/test_gpu_sparse_counts.py."""
import gzip
import io
import os

import numpy as np
import pytest

import create_object_restate as cor
import sparse_counts_restate as scr

REFS = ["Microglia/Macrophage", "Oligodendrocytes (non-malignant)"]


def small_table(seed=3, G=23, C=17, density=0.3):
    rng = np.random.default_rng(seed)
    m = rng.integers(1, 90, size=(G, C)) * (rng.random((G, C)) < density)
    m[:, [0, 5, 6, 7, C - 1]] = 0                      # empty columns at the start, in the middle and at the end
    return m


@pytest.mark.parametrize("field", ["integer", "real", "pattern"])
def test_reader_agrees_with_scipy_on_files_scipy_wrote(tmp_path, field):
    sio = pytest.importorskip("scipy.io")
    sp = pytest.importorskip("scipy.sparse")
    m = small_table()
    path = str(tmp_path / "m.mtx")
    sio.mmwrite(path, sp.csc_matrix(m.astype(np.float64 if field == "real" else np.int64)), field=field)
    G, C, colptr, rowidx, vals, _ = scr.read_mtx(path)
    want = np.asarray(sio.mmread(path).toarray())
    assert np.array_equal(scr.to_dense(colptr, rowidx, vals, G), want.astype(np.int64))
    assert np.array_equal(want != 0, m != 0) and (field == "pattern" or np.array_equal(want, m))


@pytest.mark.parametrize("kw", [dict(), dict(order="row"), dict(order="shuffle", seed=4), dict(field="real", spell=lambda k, v: b"%.15e" % v),
                                dict(field="pattern"), dict(eol=b"\r\n"), dict(eol=lambda k: b"\r\n" if k % 3 else b"\n", blank_every=5,
                                                                               final_newline=False, gaps=(b" ", b"\t", b"  "), edge_blanks=True)])
def test_reader_agrees_with_scipy_on_files_the_writer_wrote(tmp_path, kw):
    sio = pytest.importorskip("scipy.io")
    m = small_table(seed=8)
    path = str(tmp_path / "m.mtx")
    entries = scr.write_mtx(path, m, **kw)
    G, C, colptr, rowidx, vals, sorted_already = scr.read_mtx(path)
    assert sorted_already == (kw.get("order", "column") == "column")
    want = np.asarray(sio.mmread(path).toarray()).astype(np.int64)
    assert np.array_equal(scr.to_dense(colptr, rowidx, vals, G), want)
    assert np.array_equal(want, (m != 0).astype(np.int64) if kw.get("field") == "pattern" else m)
    assert colptr[1] == 0 and colptr[C] == colptr[C - 1] == len(entries) and colptr[5] == colptr[8]


BODY_REFUSALS = [
    (b"1 1 3\n0 2 4\n", "integer", "line 2, field 1: not an index in 1 .. 5: '0'"),
    (b"1 1 3\n\n6 2 4\n", "integer", "line 3, field 1: not an index in 1 .. 5: '6'"),
    (b"1 8 3\n", "integer", "line 1, field 2: not an index in 1 .. 7: '8'"),
    (b"+1 1 3\n", "integer", "line 1, field 1: not an index in 1 .. 5: '+1'"),
    (b"00000000001 1 3\n", "integer", "line 1, field 1: not an index in 1 .. 5: '00000000001'"),
    (b"1 1 -1\n", "integer", "line 1, field 3: not an integer count in 0 .. 2147483647: '-1'"),
    (b"1 1 0.5\r\n", "real", "line 1, field 3: not an integer count in 0 .. 2147483647: '0.5'"),
    (b"1 1 2147483648", "integer", "line 1, field 3: not an integer count in 0 .. 2147483647: '2147483648'"),
    (b"1 1 NA\n", "real", "line 1, field 3: not an integer count in 0 .. 2147483647: 'NA'"),
    (b"1 1 NaN\n", "real", "line 1, field 3: not an integer count in 0 .. 2147483647: 'NaN'"),
    (b"1 1 Inf\n", "real", "line 1, field 3: not an integer count in 0 .. 2147483647: 'Inf'"),
    (b"1 1 -0\n", "real", "line 1, field 3: not an integer count in 0 .. 2147483647: '-0'"),
    (b"1 1 12345678901234567890e-19\n", "real", "line 1, field 3: not an integer count in 0 .. 2147483647: '12345678901234567890e-19'"),
    (b"1 1 " + b"0" * 40 + b"3\n", "real", "line 1, field 3: not an integer count in 0 .. 2147483647: '" + "0" * 40 + "3'"),
    (b"1 1 3\n 2 2\n", "integer", "line 2, field 2: 2 fields where 3 are expected: ' 2 2'"),
    (b"1 1 3 4\n", "integer", "line 1, field 4: 4 fields where 3 are expected: '1 1 3 4'"),
    (b"1 1 3\n", "pattern", "line 1, field 3: 3 fields where 2 are expected: '1 1 3'"),
    (b"1 1 3\n% no\n", "integer", "line 2, field 1: a comment line inside the body: '% no'"),
]


@pytest.mark.parametrize("body,field,text", BODY_REFUSALS)
def test_body_refusals_have_the_stated_text(body, field, text):
    with pytest.raises(scr.Refusal) as exc:
        scr.parse_body(body, field, 5, 7)
    assert str(exc.value) == text


def test_accepted_spellings_and_blank_lines():
    body = b"1 1 3\n2 1 +3\r\n\r\n3 1 3.0\n  \t\n4\t1  3e0 \n 5 1 3.000000000000000e+00\n1 2 0\n2 2 2147483647\r"
    assert scr.parse_body(body, "real", 5, 7) == [(0, 0, 3), (1, 0, 3), (2, 0, 3), (3, 0, 3), (4, 0, 3), (0, 1, 0), (1, 1, 2147483647)]
    assert scr.parse_body(b"1 1\n2 2", "pattern", 5, 7) == [(0, 0, 1), (1, 1, 1)]
    # a 16-digit significand above 2^53 (what "%.15e" gives for 96), 19 digits, and a field that rounds to an integer
    spelled = [b"9.600000000000000e+01", b"3.000000000000000000", b"2147483646.999999999", b"96000e-3", b"1e9", b"0.0e5"]
    body = b"".join(b"1 %d %s\n" % (k + 1, s) for k, s in enumerate(spelled))
    assert [e[2] for e in scr.parse_body(body, "real", 5, 7)] == [96, 3, 2147483647, 96, 1000000000, 0]
    for s in spelled + [b"3", b"+3", b"3.0", b"3e0", b"0", b"2147483647", b"0.9999999999999999999"]:      # the last one's double is 1
        assert scr.value_field(s) == int(float(s)) and float(s) == int(float(s))
    for s in (b"1e-400", b"1e10", b"2147483647.5", b"0.99999999999999999999", b"0.999999999999", b"96000e-4", b"1e400"):
        assert scr.value_field(s) is None


HEADER_REFUSALS = [
    (b"%MatrixMarket matrix coordinate integer general\n1 1 0\n", "the banner line must start with %%MatrixMarket"),
    (b"%%MatrixMarket matrix coordinate integer\n1 1 0\n", "the banner has 4 fields, 5 are expected"),
    (b"%%MatrixMarket vector coordinate integer general\n1 1 0\n", "banner object 'vector': only 'matrix' is read"),
    (b"%%MatrixMarket matrix array integer general\n1 1\n", "banner format 'array': only 'coordinate' is read"),
    (b"%%MatrixMarket matrix coordinate complex general\n1 1 0\n", "banner field 'complex': only 'integer', 'real' and 'pattern' are read"),
    (b"%%MatrixMarket matrix coordinate integer symmetric\n1 1 0\n", "banner symmetry 'symmetric': only 'general' is read"),
    (b"%%MatrixMarket matrix coordinate integer skew-symmetric\n1 1 0\n", "banner symmetry 'skew-symmetric': only 'general' is read"),
    (b"%%MatrixMarket matrix coordinate complex hermitian\n1 1 0\n", "banner field 'complex'"),
    (b"%%MatrixMarket matrix coordinate integer general\n% only comments\n", "the size line is missing"),
    (b"%%MatrixMarket matrix coordinate integer general\n3 4\n", "size line '3 4': three integers G C nnz are expected"),
    (b"%%MatrixMarket matrix coordinate integer general\n0 4 0\n", "size line: G and C must be 1 .. 2147483647"),
    (b"%%MatrixMarket matrix coordinate integer general\n4 2147483648 0\n", "size line: G and C must be 1 .. 2147483647"),
    (b"%%MatrixMarket matrix coordinate integer general\n2 2 5\n", "size line: 5 entries do not fit a 2 x 2 matrix"),
]


@pytest.mark.parametrize("data,text", HEADER_REFUSALS)
def test_header_refusals_in_the_restatement_and_in_the_library(data, text):
    with pytest.raises(ValueError) as exc:
        scr.header(data)
    assert text in str(exc.value) and str(exc.value).startswith("read_mtx: ")
    device = pytest.importorskip("infercnv_amd.device")
    with pytest.raises(ValueError) as lib:
        device._mtx_header(io.BytesIO(data))
    assert str(lib.value) == str(exc.value)


def test_header_is_read_alike_by_the_restatement_and_the_library():
    device = pytest.importorskip("infercnv_amd.device")
    data = b"%%matrixmarket MATRIX Coordinate Real General\r\n% a comment\n%\n\n 37 29\t12 \r\n1 1 3\n"
    field, G, C, nnz, lines, used = scr.header(data)
    assert (field, G, C, nnz, lines) == ("real", 37, 29, 12, 5) and data[used:] == b"1 1 3\n"
    assert device._mtx_header(io.BytesIO(data)) == (1, 37, 29, 12, 5, used)


def test_entry_count_and_duplicates(tmp_path):
    path = str(tmp_path / "m.mtx")
    for said, there in ((3, 2), (1, 2)):
        with open(path, "wb") as fh:
            fh.write(b"%%MatrixMarket matrix coordinate integer general\n4 4 " + str(said).encode() + b"\n1 1 5\n2 1 6\n")
        with pytest.raises(ValueError, match=f"the size line says {said} entries, the body has {there}"):
            scr.read_mtx(path)
    with open(path, "wb") as fh:
        fh.write(b"%%MatrixMarket matrix coordinate integer general\n4 4 3\n3 2 5\n1 1 6\n3 2 7\n")
    with pytest.raises(ValueError, match="duplicate entry for row 3, column 2"):
        scr.read_mtx(path)


def test_make_unique():
    cases = [(["X", "X", "X"], ["X", "X.1", "X.2"]), (["a", "a", "a.2", "a"], ["a", "a.1", "a.2", "a.3"]),
             (["a", "a", "a.1"], ["a", "a.2", "a.1"]), (["b", "a", "b", "a", "c"], ["b", "a", "b.1", "a.1", "c"]), ([], [])]
    co = pytest.importorskip("infercnv_amd.create_object")
    for names, want in cases:
        assert scr.make_unique(names) == want
        assert co.make_unique(names) == want


def test_select_keeps_source_order():
    m = small_table(seed=11)
    G, C = m.shape
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        scr.write_mtx(os.path.join(d, "m.mtx"), m)
        _, _, colptr, rowidx, vals, _ = scr.read_mtx(os.path.join(d, "m.mtx"))
    genes, cells = list(range(G - 1, -1, -2)), [3, 1, 3, C - 2]
    p, r, v = scr.select(colptr, rowidx, vals, G, genes, cells)
    assert np.array_equal(scr.to_dense(p, r, v, len(genes)), m[genes][:, cells])
    for j in range(len(cells)):                         # reversed genes: the rows of a column descend, as the source ascends
        assert np.all(np.diff(r[p[j]:p[j + 1]]) < 0)


def test_restated_sparse_route_equals_the_dense_restatement_on_the_example(golden_dir, tmp_path):
    d = os.path.join(golden_dir, "create_object_example")
    genes, cells, x_bits = cor.read_table(os.path.join(d, "counts_every_8th_gene.matrix.gz"))
    x = np.rint(cor.as_double(x_bits))               # the example's values are not integers (17.86, ...): rounded, a count table
    x_bits = np.ascontiguousarray(x).view(np.int64)
    assert x.min() >= 0 and x.max() > 100
    order, annot = os.path.join(d, "gencode_downsampled.EXAMPLE_ONLY_DONT_REUSE.txt.gz"), os.path.join(d, "oligodendroglioma_annotations_downsampled.txt.gz")
    path = str(tmp_path / "example.mtx.gz")
    scr.write_mtx(path, x.astype(np.int64))
    for kw in (dict(), dict(max_cells_per_group=20, min_max_counts_per_cell=(8000, 12000), chr_exclude=("chr1", "chrY"), seed=3)):
        want = cor.create_object(genes, cells, x_bits, order, annot, REFS, **kw)
        got = scr.sparse_create_object(cor, path, genes, cells, order, annot, REFS, **kw)
        assert set(got) == set(want)
        for slot in want:
            assert np.array_equal(got[slot], want[slot]) if slot == "expr_bits" else got[slot] == want[slot], slot
