"""K34 on the device: icnv_rds_columns_dev, icnv_rds_csc_check_dev / icnv_rds_csc_fill_dev, device.read_rds_counts, and
CreateInfercnvObject / ShardedCreate from .rds and .rda files.  Every comparison is bit for bit (view(int64)) against the
sequential restatement tests/rds_counts_restate.py, or against the object the same data gives when passed as an array."""
import gzip
import io
import os

import numpy as np
import pytest
import scipy.sparse as sp

import rds_counts_restate as rs
import read_select_restate as rsr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import infercnv_amd                                    # noqa: E402
from infercnv_amd import _lib, rds, sharded            # noqa: E402
from infercnv_amd.rds import RValue                    # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "infercnv_data_example.rda")
SENTINEL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infercnv_amd import device
    torch.cuda.set_device(0)
    device.init(0)
    return device


def embedded(stream, fill, lead=13, tail=40):
    """The bytes `stream` as a view of a larger CUDA tensor of `fill` bytes: it starts at an odd address and ends with its own
    last byte; whatever a kernel loads outside it is `fill`."""
    big = torch.full((lead + len(stream) + tail,), fill, dtype=torch.uint8, device="cuda")
    big[lead:lead + len(stream)] = torch.from_numpy(np.frombuffer(bytes(stream), dtype=np.uint8).copy()).cuda()
    return big[lead:lead + len(stream)]


def bits(t):
    return t.cpu().numpy().view(np.uint64) if t.dtype == torch.float64 else t.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- dense columns
def column_stream(rows, mode):
    """32 file columns of `rows` elements, each payload at another residue mod 16 (every residue, for both element sizes), with
    the special values rotated through the first elements; the stream ends with the last payload's last byte."""
    stream, off, kind = bytearray(b"\xA5" * 3), [], []
    for c in range(32):
        real = {"real": True, "int": False, "mixed": c % 3 != 0}[mode]
        while len(stream) % 16 != (c * 7 + (0 if c < 16 else 1)) % 16:      # 7 is odd: c = 0 .. 15 visits every residue, twice over
            stream.append(0xC3)
        off.append(len(stream))
        kind.append(rs.REAL if real else rs.INT)
        if real:
            stream += np.roll(rs.real_payload(rows + 11, 100 + c), -(c % 11))[:rows].astype(">u8").tobytes()
        else:
            stream += np.roll(rs.int_payload(rows + 7, 200 + c), -(c % 7))[:rows].astype(">i4").tobytes()
    return bytes(stream), np.array(off, dtype=np.int64), np.array(kind, dtype=np.int32)


@pytest.mark.parametrize("mode", ["real", "int", "mixed"])
@pytest.mark.parametrize("n_out", [1, 2, 70])
@pytest.mark.parametrize("rows", [1, 2, 3, 63, 64, 65, 257])
def test_columns_equal_the_restatement(dev, rows, n_out, mode):
    stream, off, kind = column_stream(rows, mode)
    assert {int(o) % 16 for o in off} == set(range(16))
    pick = np.random.default_rng(rows * 100 + n_out).permutation(32)
    pick = np.concatenate([pick, pick, pick])[:n_out]                      # out of order; 70: with repeats
    if n_out > 1:
        pick[-1] = pick[0]                                                  # a repeat
    want = rs.columns(stream, off[pick], kind[pick], rows)
    outs = []
    for fill in (0x00, 0xFF):
        view = embedded(stream, fill)
        full = torch.full((n_out, rows + 5), 0.0, dtype=torch.float64, device="cuda")
        full.view(torch.int64).fill_(SENTINEL)
        dev.rds_columns(view, off[pick], kind[pick], rows, out=full[:, :rows])          # ld = rows + 5
        got = full.cpu().numpy().view(np.uint64)
        assert np.array_equal(got[:, :rows], want)
        assert (got[:, rows:] == SENTINEL).all()                           # the padding is untouched
        outs.append(got)
    assert np.array_equal(outs[0], outs[1])                                # nothing outside the stream influences the result
    tight = dev.rds_columns(embedded(stream, 0xFF), off[pick], kind[pick], rows)         # ld == rows
    assert np.array_equal(bits(tight), want)


def test_special_values_survive(dev):
    """NA_real_, a NaN with another payload, both zeros, the infinities and denormals are moved bit for bit; NA_integer_ becomes
    NA_real_, INT_MIN + 1, INT_MAX and 0 convert exactly."""
    real = np.array(rs.REAL_SPECIALS, dtype=np.uint64)
    ints = np.array(rs.INT_SPECIALS, dtype=np.int32)
    stream = b"\x00" + real.astype(">u8").tobytes() + b"\x00\x00" + ints.astype(">i4").tobytes()
    r = dev.rds_columns(embedded(stream, 0xFF), [1], [rs.REAL], real.size)
    assert np.array_equal(bits(r)[0], real)
    i = dev.rds_columns(embedded(stream, 0xFF), [3 + 8 * real.size], [rs.INT], ints.size)
    want = ints.astype(np.float64).view(np.uint64).copy()
    want[0] = rs.NA_REAL_BITS
    assert np.array_equal(bits(i)[0], want) and rs.NA_REAL_BITS == 0x7FF00000000007A2


def test_columns_refusals_leave_the_output_alone(dev):
    stream, off, kind = column_stream(5, "mixed")
    view = embedded(stream, 0x00)
    out = torch.zeros((2, 5), dtype=torch.float64, device="cuda")
    out.view(torch.int64).fill_(SENTINEL)
    last = len(stream) - 5 * (8 if kind[31] == rs.REAL else 4)
    for o, k, r in (([off[0], last + 1], [kind[0], kind[31]], 5),          # one byte past the end
                    ([off[0], -1], [kind[0], kind[1]], 5),
                    ([off[0], off[1]], [kind[0], 10], 5),                  # LGLSXP is no kind
                    ([off[0], len(stream)], [kind[0], kind[1]], 5)):
        with pytest.raises(_lib.IcnvError) as e:
            dev.rds_columns(view, o, k, r, out=out)
        assert e.value.code == _lib.ERR_ARG
    assert (out.cpu().numpy().view(np.uint64) == SENTINEL).all()
    assert np.array_equal(bits(dev.rds_columns(view, [last], [kind[31]], 5))[0], rs.column_bits(stream, last, int(kind[31]), 5))


# ---------------------------------------------------------------------------------------------------------------- CSC check and fill
def csc_stream(i, p, x_bits, pads=(5, 2, 11)):
    """[pad | i | pad | p | pad | x] with the three payloads at different residues mod 16; ends with x's last byte."""
    s = bytearray(b"\x77" * pads[0])
    i_off = len(s)
    s += np.asarray(i, dtype=np.int64).astype(np.int32).astype(">i4").tobytes() + b"\x77" * pads[1]
    p_off = len(s)
    s += np.asarray(p, dtype=np.int64).astype(np.int32).astype(">i4").tobytes() + b"\x77" * pads[2]
    x_off = len(s)
    s += np.asarray(x_bits, dtype=np.uint64).astype(">u8").tobytes()
    return bytes(s), i_off, p_off, x_off


def random_csc(G, C, seed, empty=True):
    """A valid CSC: empty columns at the front, in the middle and at the end, one full column (where C allows)."""
    rng = np.random.default_rng(seed)
    cols = []
    for c in range(C):
        n = int(rng.integers(0, G + 1))
        if empty and C >= 4 and c in (0, C // 2, C - 1):
            n = 0
        if C >= 4 and c == 1:
            n = G
        cols.append(np.sort(rng.choice(G, size=n, replace=False)))
    p = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
    i = np.concatenate(cols).astype(np.int64) if p[-1] else np.zeros(0, dtype=np.int64)
    x = rng.integers(0, 5000, size=int(p[-1])).astype(np.float64)
    if x.size >= 2:
        x[0], x[1] = 2.0 ** 31 - 1, 0.0                                    # both stored explicitly: valid
    return i, p, x.view(np.uint64)


def selections(C, seed):
    rng = np.random.default_rng(seed)
    out = [None, rng.permutation(C)]
    if C > 1:
        out.append(rng.permutation(C)[:max(1, C // 2)])
    return out


def run_check_and_fill(dev, stream, offs, G, C, nnz, cells):
    st, colptr, out_nnz = dev.rds_csc_check(stream, *offs, G, C, nnz, cells)
    if st[0] != rs.OK:
        return st, None
    rowidx, vals = dev.rds_csc_fill(stream, *offs, G, C, nnz, colptr, out_nnz, cells)
    return st, (colptr.cpu().numpy(), rowidx.cpu().numpy(), vals.cpu().numpy())


@pytest.mark.parametrize("C", [1, 2, 65, 130])
@pytest.mark.parametrize("G", [1, 5, 300])
def test_csc_equals_the_restatement(dev, G, C):
    i, p, xb = random_csc(G, C, 1000 * G + C)
    s, *offs = csc_stream(i, p, xb)
    assert len({o % 16 for o in offs}) == 3
    for cells in selections(C, G + C):
        want = rs.csc_fill(i.tolist(), p.tolist(), xb, C, None if cells is None else cells.tolist())
        for fill in (0x00, 0xFF):
            st, got = run_check_and_fill(dev, embedded(s, fill), offs, G, C, int(p[-1]), cells)
            assert st == (rs.OK, -1, -1)
            assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got, want))
    # the DeviceCounts of it is what csc_select gives of the full one
    full = run_check_and_fill(dev, embedded(s, 0), offs, G, C, int(p[-1]), None)[1]
    assert np.array_equal(full[0], p) and np.array_equal(full[1], i)


@pytest.mark.parametrize("G, C", [(1, 1), (5, 2), (300, 65)])
def test_csc_without_entries(dev, G, C):
    s, *offs = csc_stream([], np.zeros(C + 1), [])
    for cells in selections(C, 3):
        st, got = run_check_and_fill(dev, embedded(s, 0xFF), offs, G, C, 0, cells)
        n_out = C if cells is None else len(cells)
        assert st == (rs.OK, -1, -1) and np.array_equal(got[0], np.zeros(n_out + 1)) and got[1].size == got[2].size == 0


G_V, C_V, SKIPPED, TESTED = 300, 65, 3, 40


def violation_base():
    """300 x 65, every column with at least four entries: violations are planted in column 3 (skipped by the subset) and in
    column 40."""
    rng = np.random.default_rng(77)
    cols = [np.sort(rng.choice(G_V, size=int(rng.integers(4, 30)), replace=False)) for _ in range(C_V)]
    p = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
    i = np.concatenate(cols).astype(np.int64)
    x = rng.integers(1, 900, size=i.size).astype(np.float64)
    return i, p, x.view(np.uint64).copy()


def dbits(v):
    return int(np.array([v], dtype=np.float64).view(np.uint64)[0])


ENTRY_VIOLATIONS = {
    "i = G": ("i", lambda i, e: G_V, rs.ROW_RANGE),
    "i = -1": ("i", lambda i, e: -1, rs.ROW_RANGE),
    "equal i": ("i", lambda i, e: i[e - 1], rs.ROW_ORDER),
    "descending i": ("i", lambda i, e: i[e - 1] - 1 if i[e - 1] > 0 else None, rs.ROW_ORDER),
    "x = 0.5": ("x", dbits(0.5), rs.VALUE),
    "x = -1": ("x", dbits(-1.0), rs.VALUE),
    "x = 2^31": ("x", dbits(2.0 ** 31), rs.VALUE),
    "x = NaN": ("x", 0x7FF8000000000000, rs.VALUE),
    "x = NA_real_": ("x", rs.NA_REAL_BITS, rs.VALUE),
    "x = Inf": ("x", 0x7FF0000000000000, rs.VALUE),
}


def plant(i, xb, e, what):
    slot, v, code = ENTRY_VIOLATIONS[what]
    if slot == "i":
        new = v(i, e)
        if new is None:                                                     # (the previous row is 0: descend from the next entry on)
            i[e - 1], new = 5, 4
        i[e] = new
    else:
        xb[e] = v
    return code


@pytest.mark.parametrize("what", list(ENTRY_VIOLATIONS))
def test_entry_violations_and_the_skipped_column(dev, what):
    """The violation under test sits in column 40; an EARLIER stream position, in column 3, holds a DIFFERENT violation.
    Without `cells` the earlier one is reported; with a subset that skips column 3 the later one is."""
    i, p, xb = violation_base()
    e_late, e_early = int(p[TESTED]) + 2, int(p[SKIPPED]) + 1
    code_late = plant(i, xb, e_late, what)
    code_early = plant(i, xb, e_early, "x = 0.5" if code_late != rs.VALUE else "i = G")
    assert code_early != code_late
    s, *offs = csc_stream(i, p, xb, pads=(1, 3, 6))
    subset = np.array([c for c in np.random.default_rng(5).permutation(C_V) if c != SKIPPED])
    for fill in (0x00, 0xFF):
        view = embedded(s, fill)
        colptr = torch.full((C_V + 1,), 123456789, dtype=torch.int64, device="cuda")
        st, _, out_nnz = dev.rds_csc_check(view, *offs, G_V, C_V, i.size, None, colptr=colptr)
        assert st == (code_early, SKIPPED, e_early) == rs.csc_check(i.tolist(), p.tolist(), xb, G_V, C_V, i.size) and out_nnz is None
        assert (colptr == 123456789).all()                                  # a refused call leaves the output alone
        colptr = torch.full((C_V,), 123456789, dtype=torch.int64, device="cuda")
        st, _, _ = dev.rds_csc_check(view, *offs, G_V, C_V, i.size, subset, colptr=colptr)
        assert st == (code_late, TESTED, e_late) == rs.csc_check(i.tolist(), p.tolist(), xb, G_V, C_V, i.size, subset.tolist())
        assert (colptr == 123456789).all()
    # with only column 3 skipped AND column 40 skipped, the rest is valid
    clean = np.array([c for c in range(C_V) if c not in (SKIPPED, TESTED)])
    st, got = run_check_and_fill(dev, embedded(s, 0xFF), offs, G_V, C_V, i.size, clean)
    assert st == (rs.OK, -1, -1)
    assert all(np.array_equal(a, b) for a, b in zip(got, rs.csc_fill(i.tolist(), p.tolist(), xb, C_V, clean.tolist())))


@pytest.mark.parametrize("what", ["p[0] = 1", "a decreasing p", "p[C] != nnz"])
def test_p_violations_come_first_and_need_no_selection(dev, what):
    """p is validated whole: an entry violation at an earlier stream position, in a skipped or a selected column, does not hide
    it, and a subset does not either."""
    i, p, xb = violation_base()
    plant(i, xb, int(p[SKIPPED]) + 1, "x = 0.5")
    nnz = i.size
    if what == "p[0] = 1":
        p[0], want = 1, (rs.P_FIRST, 0, 0)
    elif what == "a decreasing p":
        p[50], want = p[51] + 1, (rs.P_DESCENT, 51, 51)
    else:
        p[C_V], want = nnz + 1, (rs.P_LAST, C_V - 1, C_V)
    s, *offs = csc_stream(i, p, xb)
    subset = np.array([c for c in range(C_V) if c != SKIPPED])
    for cells in (None, subset):
        colptr = torch.full((C_V + 1 if cells is None else subset.size + 1,), 42, dtype=torch.int64, device="cuda")
        st, _, _ = dev.rds_csc_check(embedded(s, 0xFF), *offs, G_V, C_V, nnz, cells, colptr=colptr)
        assert st == want == rs.csc_check(i.tolist(), p.tolist(), xb, G_V, C_V, nnz, None if cells is None else cells.tolist())
        assert (colptr == 42).all()


def test_two_violations_in_selected_columns_report_the_smaller_index(dev):
    i, p, xb = violation_base()
    e1, e2 = int(p[10]) + 3, int(p[50]) + 1
    plant(i, xb, e2, "i = -1")
    plant(i, xb, e1, "x = Inf")
    s, *offs = csc_stream(i, p, xb)
    for cells in (None, np.array([50, 10, 0]), np.arange(C_V)[::-1].copy()):
        st, _, _ = dev.rds_csc_check(embedded(s, 0x00), *offs, G_V, C_V, i.size, cells)
        assert st == (rs.VALUE, 10, e1)
    xb[e1] = dbits(7.0)
    i[e1] = i[e1 - 1]                                                       # two rules at one entry: the smaller code
    xb[e1] = dbits(0.5)
    s, *offs = csc_stream(i, p, xb)
    assert dev.rds_csc_check(embedded(s, 0x00), *offs, G_V, C_V, i.size, None)[0] == (rs.ROW_ORDER, 10, e1)


def test_equal_rows_across_a_column_boundary_are_valid(dev):
    i = np.array([0, 4, 4, 2, 2], dtype=np.int64)                           # columns {0, 4}, {4}, {2}, {2}
    p = np.array([0, 2, 3, 4, 5], dtype=np.int64)
    xb = np.array([dbits(v) for v in (1.0, 2.0 ** 31 - 1, 0.0, 3.0, 4.0)], dtype=np.uint64)
    s, *offs = csc_stream(i, p, xb)
    st, got = run_check_and_fill(dev, embedded(s, 0xFF), offs, 5, 4, 5, None)
    assert st == (rs.OK, -1, -1) and got[2].tolist() == [1, 2 ** 31 - 1, 0, 3, 4] and got[1].tolist() == i.tolist()


def test_csc_refusals_before_any_launch(dev):
    i, p, xb = violation_base()
    s, i_off, p_off, x_off = csc_stream(i, p, xb)
    view = embedded(s, 0)
    bad = [dict(x_off=x_off + 1), dict(i_off=-4), dict(p_off=len(s)), dict(G=0), dict(C=0), dict(nnz=i.size + 1), dict(cells=[0, C_V]), dict(cells=[-1])]
    for kw in bad:
        a = dict(i_off=i_off, p_off=p_off, x_off=x_off, G=G_V, C=C_V, nnz=i.size, cells=None)
        a.update(kw)
        n_out = a["C"] if a["cells"] is None else len(a["cells"])
        out = torch.full((n_out + 1,), 7, dtype=torch.int64, device="cuda")
        with pytest.raises(_lib.IcnvError) as e:
            dev.rds_csc_check(view, a["i_off"], a["p_off"], a["x_off"], a["G"], a["C"], a["nnz"], a["cells"], colptr=out)
        assert e.value.code == _lib.ERR_ARG and (out == 7).all(), kw


# ---------------------------------------------------------------------------------------------------------------- read_rds_counts
G_E, C_E = 1500, 60
GENES = np.array([f"gene{k}" for k in range(G_E)], dtype=object)
CELLS = np.array([f"cell{k}" for k in range(C_E)], dtype=object)
REFS = ["normal"]


def order_and_annotations(genes, cells, is_ref):
    """A gene order (three chromosomes, positions descending within the second so that .order_reduce reorders) and annotations
    built from the names."""
    n = len(genes)
    order = [(g, f"chr{1 + 3 * k // n}", (n - k if 3 * k // n == 1 else k) * 100 + 1, (n - k if 3 * k // n == 1 else k) * 100 + 50)
             for k, g in enumerate(genes)]
    return order[::2] + order[1::2], [(c, "normal" if is_ref(c) else "tumor") for c in cells]


@pytest.fixture(scope="module")
def written():
    rng = np.random.default_rng(34)
    ints = rng.integers(0, 3000, size=(G_E, C_E)).astype(np.int32)
    reals = ints * rng.random((G_E, C_E))
    sparse = sp.csc_matrix(ints * (rng.random((G_E, C_E)) < 0.5))
    sparse.sort_indices()
    names = {"dimnames": [GENES, CELLS]}
    order, annot = order_and_annotations(GENES, CELLS, lambda c: int(c[4:]) % 3 == 0)
    return {"values": {"matrix_int": RValue(ints, names), "matrix_real": RValue(reals, names), "dgCMatrix": rds._matrix_value(sparse, GENES, CELLS)},
            "arrays": {"matrix_int": ints, "matrix_real": reals, "dgCMatrix": sparse}, "order": order, "annot": annot}


def write_file(tmp_path, value, how):
    """uncompressed; compress=True through our writer (flush points: K29); GzipFile (none: K30)."""
    plain = io.BytesIO()
    rds.write_rds(value, plain, device=False)
    path = tmp_path / f"counts_{how}.rds"
    if how == "plain":
        path.write_bytes(plain.getvalue())
    elif how == "k29":
        rds.write_rds(value, path, compress=True)
    else:
        with gzip.GzipFile(path, "wb") as f:
            f.write(plain.getvalue())
    return path


EXPECT_INFLATE = {"plain": "none", "k29": "device_k29", "k30": "device_k30"}


@pytest.fixture
def routes(dev, monkeypatch):
    from infercnv_amd import gunzip
    monkeypatch.setattr(rds, "DEVICE_THRESHOLD", 20_000)                     # the payloads through the device, both ways
    monkeypatch.setattr(gunzip, "GUNZIP_MIN_BYTES", 0)
    monkeypatch.delenv("ICNV_GUNZIP", raising=False)
    monkeypatch.delenv("ICNV_INFLATE", raising=False)
    return gunzip


@pytest.mark.parametrize("how", ["plain", "k29", "k30"])
@pytest.mark.parametrize("kind", ["matrix_int", "matrix_real", "dgCMatrix"])
def test_create_object_from_written_files(dev, routes, written, tmp_path, kind, how):
    path = write_file(tmp_path, written["values"][kind], how)
    genes, cells, got, stats = dev.read_rds_counts(path)
    assert stats["inflate"] == EXPECT_INFLATE[how], (stats, rds.inflate_stats(), routes.gunzip_stats())    # no silent host fallback
    assert stats["kind"] == kind and genes == list(GENES) and cells == list(CELLS)
    assert (stats["uploaded_bytes"] == 0) == (how != "plain")                # an inflated stream is consumed device to device
    arr = written["arrays"][kind]
    named = dict(gene_names=GENES, cell_names=CELLS)
    for sparse in (None, False):
        obj, x = infercnv_amd.CreateInfercnvObject(str(path), written["order"], written["annot"], REFS, sparse=sparse, return_device=True,
                                                   chunk_bytes=100_000)
        as_sparse = kind == "dgCMatrix" and sparse is None
        want, want_x = infercnv_amd.CreateInfercnvObject(arr if kind != "dgCMatrix" or as_sparse else arr.toarray(), written["order"],
                                                         written["annot"], REFS, sparse=True if as_sparse else None, return_device=True, **named)
        rsr.same_object(obj, want)
        assert obj.count_data is obj.expr_data and type(obj.expr_data) is type(want.expr_data) and hasattr(obj.expr_data, "tocsc") == as_sparse
        if as_sparse:
            assert all(torch.equal(a, b) for a, b in zip(x.t[1:], want_x.t[1:]))
        else:
            assert torch.equal(x.view(torch.int64), want_x.view(torch.int64))
    if kind != "dgCMatrix":
        with pytest.raises(ValueError, match="sparse=True wants"):
            infercnv_amd.CreateInfercnvObject(str(path), written["order"], written["annot"], REFS, sparse=True)


def test_create_object_from_the_r_written_data_frame(dev):
    full = rds.read_rds(GOLDEN)["infercnv_data_example"]
    genes, cells = list(full.attrs["row.names"]), list(full.value)
    arr = np.stack([full.value[c] for c in cells], axis=1)
    assert arr.shape == (8252, 20) and arr.dtype == np.int32 and (int(arr.sum()), arr.min(), arr.max()) == (2817798, 0, 6927)
    assert genes[0] == "KIF1B" and cells[0] == "normal_9"
    order, annot = order_and_annotations(genes, cells, lambda c: c.startswith("normal"))
    g2, c2, x, stats = dev.read_rds_counts(GOLDEN)
    assert (g2, c2) == (genes, cells) and stats["kind"] == "data_frame" and stats["inflate"] in ("host", "device_k30")
    assert np.array_equal(bits(x), np.ascontiguousarray(arr.T).astype(np.float64).view(np.uint64))
    obj = infercnv_amd.CreateInfercnvObject(GOLDEN, order, annot, REFS)
    want = infercnv_amd.CreateInfercnvObject(arr, order, annot, REFS, gene_names=genes, cell_names=cells)
    rsr.same_object(obj, want)
    assert obj.expr_data.shape == (8252, 20) and set(obj.reference_grouped_cell_indices) == {"normal"}


def test_host_chunks_and_selected_columns(dev, written, tmp_path, monkeypatch):
    """A host-side stream goes up in chunks of whole requested columns; cells= picks columns in any order."""
    monkeypatch.setattr(rds, "DEVICE_THRESHOLD", 20_000)
    sel = np.array([7, 3, 59, 0, 30, 31, 32])
    for kind in ("matrix_int", "matrix_real"):
        path = write_file(tmp_path, written["values"][kind], "plain")
        full = dev.read_rds_counts(path)[2]
        for chunk in (64, G_E * 8 * 3 + 5, None):
            _, cells, x, stats = dev.read_rds_counts(path, cells=sel, chunk_bytes=chunk)
            assert cells == list(CELLS) and torch.equal(x.view(torch.int64), full[sel].view(torch.int64))
            assert stats["uploaded_bytes"] == sel.size * G_E * (4 if kind == "matrix_int" else 8)      # only the requested columns
        assert np.array_equal(bits(full), np.ascontiguousarray(written["arrays"][kind].T).astype(np.float64).view(np.uint64))
    with pytest.raises(ValueError, match="cells entry 60 is not a column"):
        dev.read_rds_counts(path, cells=[60])


def test_an_invalid_dgcmatrix_is_refused_with_its_rule(dev, written, tmp_path):
    good = written["values"]["dgCMatrix"]
    cases = [("x", 5, 0.5, "the sparse route wants integer counts"), ("i", 1, None, "do not strictly increase"), ("p", 3, None, "p decreases")]
    for slot, at, v, text in cases:
        slots = {k: (np.array(s, copy=True) if isinstance(s, np.ndarray) else s) for k, s in good.slots.items()}
        if slot == "x":
            slots["x"][at] = v
        elif slot == "i":
            slots["i"][at] = slots["i"][at - 1]
        else:
            slots["p"][at] = slots["p"][at + 1] + 1
        path = write_file(tmp_path, rds.RS4("dgCMatrix", "Matrix", slots), "plain")
        with pytest.raises(ValueError, match=text):
            infercnv_amd.CreateInfercnvObject(str(path), written["order"], written["annot"], REFS)
        if slot == "p":                                                     # p is validated whole, whatever is selected
            with pytest.raises(ValueError, match=text):
                dev.read_rds_counts(path, cells=[50, 20])
        else:                                                               # the planted entry lies in column 0: skipped, not examined
            assert dev.read_rds_counts(path, cells=[50, 20])[2].C == 2


# ---------------------------------------------------------------------------------------------------------------- ShardedCreate
@pytest.mark.parametrize("kind", ["matrix_int", "dgCMatrix"])
def test_sharded_create_from_an_rds_file(dev, written, tmp_path, monkeypatch, kind):
    monkeypatch.setattr(rds, "DEVICE_THRESHOLD", 20_000)
    path = str(write_file(tmp_path, written["values"][kind], "plain"))
    single, x_single = infercnv_amd.CreateInfercnvObject(path, written["order"], written["annot"], REFS, return_device=True)
    obj, x, shard = sharded.ShardedCreate(path, written["order"], written["annot"], REFS, rank=0, world=1).run()
    rsr.same_object(obj, single)
    assert shard["global_index"].tolist() == list(range(len(single.cell_names)))
    full = dev.read_rds_counts(path)[2]
    for how in ("cyclic", "block"):                                         # rank 1 of 3: the gather of the full read
        sc = sharded.ShardedCreate(path, written["order"], written["annot"], REFS, rank=1, world=3, deal=how)
        mine = sc.dealt(C_E)
        _, cells, part, st = dev.read_rds_counts(path, cells=mine, chunk_bytes=50_000)
        assert cells == list(CELLS)
        if kind == "dgCMatrix":
            assert st["uploaded_bytes"] == 4 * (C_E + 1) + 12 * part.nnz < st["payload_bytes"] / 2     # p, and this rank's entries only
            want = dev.csc_select(full, np.arange(G_E), mine)
            assert all(torch.equal(a, b) for a, b in zip(part.t[1:], want.t[1:]))
        else:
            assert torch.equal(part.view(torch.int64), full[mine].view(torch.int64))
        ranks = [sharded.ShardedCreate(path, written["order"], written["annot"], REFS, rank=r, world=3, deal=how) for r in range(3)]
        sums = ranks[0].place([r.read() for r in ranks])
        shards = [r.finish(sums) for r in ranks]
        rsr.check_shards(single, shards, C_E, 3, how)
