"""The table reader on the GPU (icnv_parse_table_dev, device.read_table, DESIGN K21) against the restatement of
tests/create_object_restate.py: str.split and float() per field.  Every comparison is equality of int64 bit patterns."""
import numpy as np
import pytest

import create_object_restate as cor
import table_parse_cases as cases

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from infercnv_amd import IcnvError   # noqa: E402


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infercnv_amd import device
    torch.cuda.set_device(0)
    device.init(0)
    return device


def read_both(dev, path, sep="\t", chunk_bytes=None):
    """read_table of the library and of the restatement; asserts they agree and returns the library's result."""
    rows, cols, x, stats = dev.read_table(str(path), sep=sep, chunk_bytes=chunk_bytes)
    r_rows, r_cols, r_bits = cor.read_table(str(path), sep)
    assert rows == r_rows and cols == r_cols
    assert tuple(x.shape) == (len(r_cols), len(r_rows)) and x.is_contiguous()
    got = x.cpu().numpy().view(np.int64)
    assert np.array_equal(got, r_bits.T)
    assert stats["rows"] == len(r_rows) and stats["fields"] == r_bits.size
    return rows, cols, got, stats


def write(tmp_path, name, text):
    path = tmp_path / name
    path.write_bytes(text.encode() if isinstance(text, str) else text)
    return path


# ---------------------------------------------------------------- 1. the number grammar
def test_plain_numbers_never_reach_the_host(dev, tmp_path):
    text, names, cols, _ = cases.table_text(cases.PLAIN, 7)
    rows, _, _, stats = read_both(dev, write(tmp_path, "plain.tsv", text))
    assert rows == names and stats["host_parsed"] == 0 and stats["fields"] >= 3000


def test_adversarial_numbers_and_na(dev, tmp_path):
    fields = cases.ADVERSARIAL + cases.PLAIN[:500]
    text, _, _, rows = cases.table_text(fields, 7)
    _, _, got, stats = read_both(dev, write(tmp_path, "hard.tsv", text))
    assert stats["host_parsed"] >= len(cases.TIES)                     # every exact tie is the host's
    flat = [f for r in rows for f in r]
    by_text = {f: got.T.ravel()[i] for i, f in enumerate(flat)}
    assert by_text["NA"] == by_text[""] == cor.signed(0x7FF00000000007A2)       # NA_real_, not the quiet NaN
    assert by_text["NaN"] == cor.signed(0x7FF8000000000000) and by_text["NA"] != by_text["NaN"]
    assert by_text["-0"] == cor.signed(1 << 63) and by_text["1e400"] == cor.signed(0x7FF0000000000000)
    assert by_text["4.9e-324"] == 1 and by_text["1e-400"] == 0


def test_more_uncertified_fields_than_one_round_lists(dev, tmp_path):
    """70 000 exact ties in one chunk: the list holds 65 536, a collection round finds the rest."""
    text, _, _, _ = cases.table_text(["9007199254740993"] * 70000, 7)
    _, _, _, stats = read_both(dev, write(tmp_path, "many_ties.tsv", text))
    assert stats["chunks"] == 1 and stats["host_parsed"] == 70000 and stats["collect_rounds"] == 1


def test_ties_alone_count_on_the_host(dev, tmp_path):
    text, _, _, _ = cases.table_text(cases.TIES + ["9007199254740993"], 3)
    _, _, _, stats = read_both(dev, write(tmp_path, "ties.tsv", text))
    assert stats["host_parsed"] >= len(cases.TIES) + 1 > 0


# ---------------------------------------------------------------- 2. structure
def small(n_rows, n_cols, seed):
    rng = np.random.default_rng(seed)
    return ["%.6g" % v for v in rng.gamma(0.7, 30.0, size=n_rows * n_cols)]


@pytest.mark.parametrize("n_rows,n_cols", [(1, 1), (1, 300), (300, 1), (37, 53)])
def test_shapes(dev, tmp_path, n_rows, n_cols):
    text, _, _, _ = cases.table_text(small(n_rows, n_cols, n_rows + n_cols), n_cols)
    read_both(dev, write(tmp_path, "t.tsv", text))


@pytest.mark.parametrize("chunk_bytes", [64, 333, 4096, 4097, 10000])
def test_rows_fields_and_crlf_straddle_chunks(dev, tmp_path, chunk_bytes):
    """37 x 53 with \\r\\n line ends: 16 KB, four 4096-byte segments per large chunk; the small chunks are shorter than one
    line (every buffer grows first) or cut the file at many different rows."""
    text, _, _, _ = cases.table_text(small(37, 53, 9), 53, eol="\r\n")
    _, _, _, stats = read_both(dev, write(tmp_path, "crlf.tsv", text), chunk_bytes=chunk_bytes)
    if chunk_bytes < 300:
        assert stats["grown"] > 0 and stats["chunks"] > 10


def test_crlf_pair_across_a_segment_boundary(dev, tmp_path):
    """Rows of exactly 64 bytes after a first row of 65: the \\r of row 64 is byte 4095 of the body and its \\n byte 4096."""
    def row(i, n):
        label = f"r{i}"
        return label + "\t" + "1" * (n - len(label) - 1 - 2 - 2) + "\t7"
    lines = ["a\tb", row(0, 65)] + [row(i, 64) for i in range(1, 130)]
    text = "\r\n".join(lines) + "\r\n"
    body = text.split("\r\n", 1)[1].encode()
    assert body[4095:4097] == b"\r\n" and body[8191:8193] == b"\r\n"
    read_both(dev, write(tmp_path, "seg.tsv", text))


def test_a_file_that_ends_where_a_buffer_ends(dev, tmp_path):
    """Every line, the header too, is exactly the 64 bytes of a chunk: the file ends with a full buffer, and the reader hands
    over an empty last chunk -- as a rule while the chunk before it is parsed, so the copy ahead takes it.  It is passed over
    like any empty chunk.  The reading runs on a thread that is joined with a time limit, so a loop that does not end fails."""
    import threading
    lines = ["a" * 31 + "\t" + "b" * 31] + [f"r{i}\t" + "1" * (63 - len(f"r{i}") - 3) + "\t7" for i in range(20)]
    assert all(len(l) == 63 for l in lines)
    path = write(tmp_path, "full.tsv", "\n".join(lines) + "\n")
    box = {}

    def run():
        try:
            dev.init(0)
            box["value"] = read_both(dev, path, chunk_bytes=64)
        except BaseException as exc:
            box["raised"] = exc
    worker = threading.Thread(target=run, daemon=True)
    worker.start()
    worker.join(60.0)
    assert not worker.is_alive(), "read_table did not return"
    if "raised" in box:
        raise box["raised"]
    rows, _, _, stats = box["value"]
    assert len(rows) == 20 and stats["chunks"] == 20 and stats["grown"] == 0


def test_one_line_longer_than_the_chunk(dev, tmp_path):
    fields = small(3, 400, 4)
    text, _, _, _ = cases.table_text(fields, 400)
    _, _, _, stats = read_both(dev, write(tmp_path, "wide.tsv", text), chunk_bytes=256)
    assert stats["grown"] > 0


def test_no_final_newline_blank_lines_and_trailing_empty_field(dev, tmp_path):
    text, _, _, _ = cases.table_text(small(5, 4, 1), 4, final_newline=False)
    read_both(dev, write(tmp_path, "nofinal.tsv", text))
    read_both(dev, write(tmp_path, "sep_last.tsv", "a\tb\ng1\t1\t\ng2\t\t"))            # empty fields are NA, also at the very end
    text, _, _, _ = cases.table_text(small(5, 4, 2), 4)
    lines = text.split("\n")
    blanky = "\n".join(lines[:2] + ["", ""] + lines[2:4] + ["\r"] + lines[4:]) + "\n\n\r\n\n"
    for chunk_bytes in (None, 64):
        rows, _, _, _ = read_both(dev, write(tmp_path, "blank.tsv", blanky), chunk_bytes=chunk_bytes)
        assert len(rows) == 5


def test_both_header_shapes_and_quoted_labels_with_a_space_separator(dev, tmp_path):
    fields = small(6, 5, 3)
    plain, names, cols, _ = cases.table_text(fields, 5)
    corner, _, _, _ = cases.table_text(fields, 5, header_corner=True)
    a = read_both(dev, write(tmp_path, "plain.tsv", plain))
    b = read_both(dev, write(tmp_path, "corner.tsv", corner))
    assert a[0] == b[0] == names and a[1] == b[1] == cols and np.array_equal(a[2], b[2])
    quoted, _, _, _ = cases.table_text(fields, 5, sep=" ", quote_labels=True)
    c = read_both(dev, write(tmp_path, "quoted.txt", quoted), sep=" ")
    assert c[0] == names and c[1] == cols and np.array_equal(a[2], c[2])


# ---------------------------------------------------------------- 3. round trip with the writer (K20)
def test_round_trip_with_write_matrix(dev, tmp_path):
    from infercnv_amd import heatmap as hm
    rng = np.random.default_rng(20)
    G, C = 64, 40
    x = rng.normal(1.0, 0.3, size=(G, C)) * 10.0 ** rng.integers(-3, 4, size=(G, C))
    x_dev = torch.from_numpy(np.ascontiguousarray(x.T)).cuda()
    genes, cells = [f"gene{i}" for i in range(G)], [f"cell{j}" for j in range(C)]
    path = tmp_path / "expr.dat"
    hm.write_matrix(str(path), x_dev, np.arange(C), "gene_rows", row_names=genes, col_names=cells, quote=True, sep=" ")
    rows, cols, got, _ = read_both(dev, path, sep=" ")                 # equals float() of every written field
    assert rows == genes and cols == cells
    back = got.view(np.float64).T                                      # genes x cells
    rounded = np.array([[float("%.15g" % v) for v in r] for r in x])
    assert np.array_equal(back.view(np.int64), rounded.view(np.int64))


# ---------------------------------------------------------------- 4. refusals
BAD = [("ragged", "a\tb\ng1\t1\t2\ng2\t3\ng3\t4\t5\n", r"line 3, field 2"),
       ("too_many", "a\tb\ng1\t1\t2\ng2\t3\t4\t5\n", r"line 3, field 4"),
       ("two_points", "a\tb\ng1\t1\t2\n\ng2\t3\t1.2.3\n", r"line 4, field 3.*'1\.2\.3'"),
       ("letters", "a\tb\ng1\tabc\t2\n", r"line 2, field 2.*'abc'"),
       ("quoted_number", 'a\tb\ng1\t1\t"2"\n', r"line 2, field 3"),
       ("quote_in_label", 'a\tb\ng1\t1\t2\ng"2\t1\t2\n', r"line 3, field 1"),
       ("hex", "a\tb\ng1\t0x10\t2\n", r"line 2, field 2"),
       ("blank_padded", "a\tb\ng1\t 1\t2\n", r"line 2, field 2"),
       ("long_bad", "a\tb\ng1\t1\t" + "1" * 50 + "x\n", r"line 2, field 3"),
       ("host_refusal_first", "a\tb\ng1\t1\t" + "1" * 50 + "x\ng2\tabc\t2\n", r"line 2, field 3"),
       ("many_short_lines", "a\tb\tc\td\te\ng1\t1\t2\t3\t4\t5\n" + "x\t1\n" * 100, r"line 3, field 2"),
       ("first_of_two", "a\tb\ng1\t1\t2\ng2\tzz\t2\ng3\t1\tyy\n", r"line 3, field 2.*'zz'")]


@pytest.mark.parametrize("name,text,match", BAD, ids=[b[0] for b in BAD])
def test_refusals_name_line_and_field_and_leave_the_output_alone(dev, tmp_path, name, text, match):
    with pytest.raises(IcnvError, match=match):
        dev.read_table(str(write(tmp_path, name + ".tsv", text)))
    with pytest.raises(IcnvError, match=match):
        dev.read_table(str(write(tmp_path, name + ".tsv", text)), chunk_bytes=64)
    body = text.split("\n", 1)[1].encode()
    host = np.frombuffer(body, dtype=np.uint8).copy()
    out = torch.full((2, 8), -7.25, dtype=torch.float64, device="cuda")
    with pytest.raises(IcnvError):
        dev.parse_table_into(torch.from_numpy(host).cuda(), host, host.size, "\t", out, 1, 6, line0=2)
    assert bool((out == -7.25).all())


def test_parse_table_into_places_rows_at_row0(dev):
    body = b"g1\t1\t2\ng2\t3\t4\n"
    host = np.frombuffer(body, dtype=np.uint8).copy()
    out = torch.full((2, 8), -7.25, dtype=torch.float64, device="cuda")
    n, ranges = dev.parse_table_into(torch.from_numpy(host).cuda(), host, host.size, "\t", out, 3, 5)
    assert n == 2 and ranges.tolist() == [[0, 2], [7, 9]]
    want = np.full((2, 8), -7.25)
    want[:, 3:5] = [[1, 3], [2, 4]]
    assert np.array_equal(out.cpu().numpy(), want)
    with pytest.raises(IcnvError, match="max_rows"):
        dev.parse_table_into(torch.from_numpy(host).cuda(), host, host.size, "\t", out, 0, 1)
    assert np.array_equal(out.cpu().numpy(), want)


def test_gather_matrix(dev):
    rng = np.random.default_rng(8)
    x = rng.normal(size=(9, 300))
    genes, cells = rng.permutation(300)[:257], np.array([8, 0, 3, 3])
    got = dev.gather_matrix(torch.from_numpy(x).cuda(), genes=genes, cells=cells).cpu().numpy()
    assert np.array_equal(got, x[cells][:, genes])
    assert np.array_equal(dev.gather_matrix(torch.from_numpy(x).cuda(), cells=cells).cpu().numpy(), x[cells])
    with pytest.raises(IcnvError):
        dev.gather_matrix(torch.from_numpy(x).cuda(), genes=[300])


def test_host_buffer_entry(dev):
    """icnv_parse_table: host bytes in, the host matrix written at row0 with its own ld, untouched on a refusal."""
    import ctypes as ct
    from infercnv_amd import _lib
    L = _lib.load()
    body = b'"g 1"\t1\t2.5\r\n\r\ng2\t4503599627370496.5\tNA'
    out = np.full((2, 5), -7.25)
    ranges, n = np.zeros((3, 2), dtype=np.int64), ct.c_int64(0)
    args = (len(body), b"\t", 2, 2, out.ctypes.data_as(ct.c_void_p), 5, 1, 3, ranges.ctypes.data_as(ct.POINTER(ct.c_int64)), ct.byref(n))
    _lib.check(L.icnv_parse_table(body, *args))
    assert n.value == 2 and [body[b:e] for b, e in ranges[:2].tolist()] == [b"g 1", b"g2"]
    want = np.full((2, 5), -7.25)
    want[0, 1:3], want[1, 1] = [1.0, float("4503599627370496.5")], 2.5
    want[1, 2] = np.array([0x7FF00000000007A2], dtype=np.uint64).view(np.float64)[0]
    assert np.array_equal(out.view(np.int64), want.view(np.int64))
    bad = body.replace(b"2.5", b"2,5")
    with pytest.raises(IcnvError, match="line 2, field 3"):
        _lib.check(L.icnv_parse_table(bad, *args))
    assert np.array_equal(out.view(np.int64), want.view(np.int64))
