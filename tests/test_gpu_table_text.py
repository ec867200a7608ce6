"""plot_cnv's matrix files written on the GPU (icnv_format_table_dev, heatmap.write_matrix, DESIGN K20) against the restatement
of tests/table_text_restate.py and against heatmap.write_table.  Every comparison is equality of bytes."""
import ctypes as ct
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import table_text_restate as ttr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from infercnv_amd import IcnvError, _lib   # noqa: E402
from infercnv_amd import heatmap as hm     # noqa: E402


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infercnv_amd import device
    torch.cuda.set_device(0)
    device.init(0)
    return device


def on_dev(x_gc, ld=None):
    """x_gc[g, c] on the host -> the (C, G) CUDA view the library takes, rows `ld` apart with NaN in the padding."""
    x_cg = np.ascontiguousarray(np.asarray(x_gc, dtype=np.float64).T)
    C, G = x_cg.shape
    if ld is None or ld == G:
        return torch.from_numpy(x_cg).cuda()
    full = torch.full((C, ld), float("nan"), dtype=torch.float64, device="cuda")
    view = full[:, :G]
    view.copy_(torch.from_numpy(x_cg))
    return view


# ---------------------------------------------------------------- 1. the field rule
TIES = [100000000000000.5, 123456789012345.5, 123456789012346.5, 999999999999999.5]      # the last one also carries into a new digit
PLAIN = [0.0, -0.0, 1.0, 0.1, 0.3, 2.0 / 3.0, 0.30000000000000004, 1e5, 100000.0, 1e-4, 0.0001234, 1234567.125, 2.0 ** -20, 1e15, 1e22,
         5e-324, 2.2250738585072014e-308, 1.7976931348623157e308, float("nan"), float("inf"), float("-inf"),
         -1.0, -0.1, -2.0 / 3.0, -1e5, -1e-4, -0.0001234, -1234567.125, -1e15, -1e22, -5e-324, -1.7976931348623157e308]
PLANTED = TIES + [-TIES[1], -TIES[3]]


def rule_fixture():
    rng = np.random.default_rng(2020)
    G, C = 70, 5
    x = rng.normal(1.0, 0.1, size=(G, C))
    vals = PLAIN + PLANTED
    where = rng.permutation(G * C)[:len(vals)]
    x.ravel()[where] = vals
    return x


def outside_certified_domain(x):
    """Is x outside the domain in which DESIGN K20 certifies the digits pass?  With s = |x| 10^(14 - E) in [10^14, 10^15): the
    fraction of s lies within 2^-62 of 1/2, or s lies within 2^-62 of 10^14 or of 10^15 (|x| next to a power of ten: the digits pass
    could not tell on which side, and although both readings print the same text it leaves the element to the host)."""
    if x != x or math.isinf(x) or x == 0.0:
        return False
    v = Fraction(abs(x))
    e = math.floor(math.log10(abs(x))) if abs(x) > 1e-300 else -330
    while Fraction(10) ** (e + 1) <= v:
        e += 1
    while Fraction(10) ** e > v:
        e -= 1
    s = v * Fraction(10) ** (14 - e)
    eps = Fraction(1, 2 ** 62)
    return abs(s - math.floor(s) - Fraction(1, 2)) < eps or 10 ** 15 - s < eps or s - 10 ** 14 < eps


@pytest.mark.parametrize("orientation", ["gene_rows", "cell_rows"])
def test_field_rule(dev, orientation):
    x = rule_fixture()
    flat = x.ravel().tolist()
    assert sorted(v for v in flat if ttr.is_exact_tie(v)) == sorted(PLANTED)
    G, C = x.shape
    xd = on_dev(x, ld=80)
    cells = [3, 0, 4, 1, 2]
    n_rows = G if orientation == "gene_rows" else C
    labels = [f'"row {i}"'.encode() for i in range(n_rows)]
    dev.table_text_stats(reset=True)
    got, done = dev.format_table(xd, rows=(0, n_rows), cells=cells, orientation=orientation, labels=labels, sep=" ")
    st = dev.table_text_stats()
    assert done == n_rows
    assert got == b"".join(ttr.rows(x, orientation, cells, 0, n_rows, labels, " "))
    # 4. the fallback is a fallback: every planted tie went to the host, and nothing that the certificate covers
    assert len(PLANTED) <= st["host_formatted"] <= sum(outside_certified_domain(v) for v in flat)
    assert st["calls"] == 1 and st["elements"] == G * C and st["rows"] == n_rows and st["bytes"] == len(got)


def test_field_rule_host_entry(dev):
    """icnv_format_table: host matrix, host output, row offsets."""
    x = rule_fixture()
    G, C = x.shape
    L = _lib.load()
    host = np.ascontiguousarray(x.T)
    cells = np.arange(C, dtype=np.int32)
    out = np.zeros(G * C * 23, dtype=np.uint8)
    offs = np.zeros(G + 1, dtype=np.int64)
    done, nbytes = ct.c_int64(-1), ct.c_int64(-1)
    rc = L.icnv_format_table(host.ctypes.data, G, C, _lib.TABLE_GENE_ROWS, 0, G, cells.ctypes.data_as(ct.POINTER(ct.c_int32)), C, None, None,
                             b"\t", out.ctypes.data, out.size, offs.ctypes.data_as(ct.POINTER(ct.c_int64)), ct.byref(done), ct.byref(nbytes))
    assert rc == _lib.OK, L.icnv_last_error()
    want = ttr.rows(x, "gene_rows", list(range(C)), 0, G, None, "\t")
    assert done.value == G and out[:nbytes.value].tobytes() == b"".join(want)
    assert offs.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()


# ---------------------------------------------------------------- 2. shapes
def heat_values(rng, shape):
    """What a clamped heatmap holds: N(1, 0.1) and 2^U(-0.3, 0.3) half and half, 1 % of it the clamp bound (it prints short)."""
    x = np.where(rng.random(shape) < 0.5, rng.normal(1.0, 0.1, size=shape), 2.0 ** rng.uniform(-0.3, 0.3, size=shape))
    x[rng.random(shape) < 0.01] = 1.25
    return x


CELL_LISTS = {"one": lambda C: [C // 2], "two": lambda C: [C - 1, 0], "all64": lambda C: list(range(64)), "all70": lambda C: list(range(70)),
              "perm": lambda C: np.random.default_rng(3).permutation(C).tolist(), "repeat": lambda C: [5, 2, 5, 69, 2]}
LABELS = {"absent": lambda n: None, "empty": lambda n: [b""] * n, "quoted": lambda n: [('"g%s"' % ("x" * (i % 7))).encode() for i in range(n)],
          "bare": lambda n: [("gene-%d" % (i * i)).encode() for i in range(n)]}
SHAPE_CASES = [  # G, cell list, padded, g0, labels, sep, orientation
    (1, "all70", False, 0, "quoted", " ", "gene_rows"), (2, "perm", True, 1, "bare", "\t", "gene_rows"),
    (63, "two", False, 0, "absent", " ", "gene_rows"), (64, "all64", True, 0, "empty", " ", "gene_rows"),
    (65, "all70", False, 7, "quoted", "\t", "gene_rows"), (257, "perm", True, 100, "bare", " ", "gene_rows"),
    (257, "one", False, 0, "quoted", " ", "gene_rows"), (65, "repeat", True, 0, "absent", "\t", "gene_rows"),
    (1, "repeat", False, 0, "bare", " ", "cell_rows"), (64, "two", True, 1, "quoted", "\t", "cell_rows"),
    (257, "all70", False, 3, "empty", " ", "cell_rows"), (257, "perm", True, 0, "absent", " ", "cell_rows"),
    (63, "one", True, 0, "quoted", " ", "cell_rows"), (65, "all64", False, 60, "bare", "\t", "cell_rows"),
]


@pytest.mark.parametrize("case", range(len(SHAPE_CASES)))
def test_shapes(dev, case):
    G, cl, padded, r0, lab, sep, orientation = SHAPE_CASES[case]
    C = 70
    rng = np.random.default_rng(100 + case)
    x = heat_values(rng, (G, C))
    assert not any(ttr.is_exact_tie(v) for v in x.ravel().tolist())
    cells = CELL_LISTS[cl](C)
    total = G if orientation == "gene_rows" else len(cells)
    r0 = min(r0, total - 1)
    n = total - r0
    labels = LABELS[lab](n)
    xd = on_dev(x, ld=(G + 15) // 16 * 16 if padded else G)
    dev.table_text_stats(reset=True)
    got, done = dev.format_table(xd, rows=(r0, n), cells=cells, orientation=orientation, labels=labels, sep=sep)
    assert done == n
    assert got == b"".join(ttr.rows(x, orientation, cells, r0, n, labels, sep))
    assert dev.table_text_stats()["host_formatted"] == 0          # 4. tie-free data never reaches the host


# ---------------------------------------------------------------- 3. chunking
def chunk_case():
    rng = np.random.default_rng(33)
    G, C = 257, 70
    x = heat_values(rng, (G, C))
    genes, cells = [f"G{i}" for i in range(G)], [f"cell-{i:02d}" for i in range(C)]
    perm = rng.permutation(C)
    obs, ref = perm[:50].tolist(), perm[50:].tolist()
    layouts = {   # orientation, cells, row names, column names, quote, sep
        "expr_dat": ("gene_rows", list(range(C)), genes, cells, False, "\t"),
        "observations": ("gene_rows", obs, genes, [cells[c] for c in obs], True, " "),
        "references": ("gene_rows", ref, genes, [cells[c] for c in ref], True, " "),
        "members": ("cell_rows", obs[:9], [cells[c] for c in obs[:9]], genes, True, " "),
        "one_member": ("gene_rows", [obs[3]], genes, ["V1"], True, " "),
    }
    return x, layouts


def table_rows(x, orientation, cells):
    return [x[g, cells].tolist() for g in range(x.shape[0])] if orientation == "gene_rows" else [x[:, c].tolist() for c in cells]


@pytest.mark.parametrize("layout", ["expr_dat", "observations", "references", "members", "one_member"])
def test_chunking(dev, tmp_path, monkeypatch, layout):
    x, layouts = chunk_case()
    orientation, cells, row_names, col_names, quote, sep = layouts[layout]
    want_path, got_path = str(tmp_path / "want.txt"), str(tmp_path / "got.txt")
    hm.write_table(want_path, table_rows(x, orientation, cells), row_names, col_names, quote=quote, sep=sep)
    want = open(want_path, "rb").read()
    assert want == ttr.file_bytes(x, orientation, cells, row_names, col_names, quote, sep)
    body = want.split(b"\n")[1:-1]
    n_fields = len(cells) if orientation == "gene_rows" else x.shape[0]
    worst_row = max(len(b.split(sep.encode(), 1)[0]) for b in body) + 1 + 23 * n_fields
    xd = on_dev(x, ld=272)
    for chunk, rows_per_chunk in ((3 * worst_row, 3), (max(len(b) for b in body) + 1, 1)):
        monkeypatch.setenv("ICNV_TABLE_TEXT_CHUNK", str(chunk))
        st = hm.write_matrix(got_path, xd, cells, orientation, row_names, col_names, quote=quote, sep=sep)
        assert open(got_path, "rb").read() == want
        assert st["chunks"] == -(-len(body) // rows_per_chunk) and st["bytes"] == sum(len(b) + 1 for b in body)
    for chunk in (len(body[0]), 8):            # below the first row: found by the lengths pass / before any launch
        monkeypatch.setenv("ICNV_TABLE_TEXT_CHUNK", str(chunk))
        with pytest.raises(IcnvError) as err:
            hm.write_matrix(got_path, xd, cells, orientation, row_names, col_names, quote=quote, sep=sep)
        assert err.value.code == _lib.ERR_ARG


# ---------------------------------------------------------------- 5. plot_cnv
def plot_objects():
    from test_gpu_heatmap import synthetic_object, with_subclusters
    lone = synthetic_object()
    expr = np.array(lone.expr_data)
    expr[:, int(np.asarray(lone.observation_grouped_cell_indices["a_single_cell_group"])[0])] += 3.0   # cutree(k = 2) leaves it alone
    lone.expr_data = expr
    return {"by_groups": (with_subclusters(synthetic_object(), True), dict(cluster_by_groups=True, x_range=(0.9, 1.1))),
            "all_observations": (with_subclusters(synthetic_object(), False), dict(cluster_by_groups=False, k_obs_groups=3, x_range=(0.9, 1.1))),
            "single_member": (lone, dict(cluster_by_groups=False, k_obs_groups=2, x_range=None))}


@pytest.mark.parametrize("which", ["by_groups", "all_observations", "single_member"])
def test_plot_cnv_files(dev, tmp_path, which):
    import heatmap_restate as hmr
    obj, kw = plot_objects()[which]
    kw = dict(kw, write_expr_matrix=True, x_center=1.0, png_res=40, output_filename="run")
    got_dir, want_dir = str(tmp_path / "got"), str(tmp_path / "want")
    dev.table_text_stats(reset=True)
    hm.plot_cnv(obj, got_dir, **kw)
    assert dev.table_text_stats()["calls"] >= 3
    hmr.plot_cnv(obj, want_dir, **kw)
    names = sorted(os.listdir(want_dir))
    assert {"expr.run.dat", "run.observations.txt", "run.references.txt"} <= set(names)
    for n in names:
        assert open(os.path.join(got_dir, n), "rb").read() == open(os.path.join(want_dir, n), "rb").read(), n
    # the matrix files again, from the field rule's restatement: names and order are read from the files' own labels
    expr = np.asarray(obj.expr_data, dtype=np.float64)
    clamped = expr if kw["x_range"] is None else np.clip(expr, *kw["x_range"])
    genes, cells = [str(g) for g in obj.genes()], [str(c) for c in obj.cells()]
    index = {c: i for i, c in enumerate(cells)}
    got = lambda n: open(os.path.join(got_dir, n), "rb").read()
    assert got("expr.run.dat") == ttr.file_bytes(expr, "gene_rows", list(range(len(cells))), genes, cells, quoted=False, sep="\t")
    members = [n for n in names if n.startswith("General_HCL_")]
    assert bool(members) == (not kw["cluster_by_groups"])
    single = 0
    for n in ["run.observations.txt", "run.references.txt"] + members:
        text = got(n)
        header = [h.strip('"') for h in text.split(b"\n", 1)[0].decode().split(" ")]
        if n.startswith("General_HCL_") and header != ["V1"]:
            order = [index[line.split(b" ", 1)[0].decode().strip('"')] for line in text.split(b"\n")[1:-1]]
            assert header == genes
            assert text == ttr.file_bytes(clamped, "cell_rows", order, [cells[c] for c in order], genes)
        elif header == ["V1"]:
            single += 1
            lone = [c for c in range(len(cells)) if text == ttr.file_bytes(clamped, "gene_rows", [c], genes, ["V1"])]
            assert len(lone) == 1
        else:
            order = [index[h] for h in header]
            assert text == ttr.file_bytes(clamped, "gene_rows", order, genes, header)
    assert single == (1 if which == "single_member" else 0)


# ---------------------------------------------------------------- 6. bad arguments
def test_bad_arguments(dev):
    L = _lib.load()
    G, C, ld = 10, 4, 16
    x = torch.ones((C, ld), dtype=torch.float64, device="cuda")
    out = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    i32p, i64p = ct.POINTER(ct.c_int32), ct.POINTER(ct.c_int64)
    cells = np.array([0, 1, 2, 3], dtype=np.int32)
    off = np.arange(G + 1, dtype=np.int64)
    lab = np.frombuffer(b"abcdefghij", dtype=np.uint8)
    done, nbytes = ct.c_int64(-7), ct.c_int64(-7)

    def call(xp=x.data_ptr(), ld=ld, G=G, C=C, orientation=0, row0=0, n_rows=G, cells=cells, n_cells=4, lab=lab.ctypes.data, off=off,
             sep=b" ", outp=out.data_ptr(), cap=4096):
        return L.icnv_format_table_dev(xp, ld, G, C, orientation, row0, n_rows, cells.ctypes.data_as(i32p), n_cells, lab,
                                       None if off is None else off.ctypes.data_as(i64p), sep, outp, cap, None, ct.byref(done),
                                       ct.byref(nbytes), None)

    dev.table_text_stats(reset=True)
    bad_off, down_off = off.copy(), off.copy()
    bad_off[0] = 1
    down_off[5] = 3
    refused = [dict(cells=np.array([0, 1, 4, 3], dtype=np.int32)), dict(cells=np.array([0, -1, 2, 3], dtype=np.int32)), dict(ld=G - 1),
               dict(xp=None), dict(n_rows=0), dict(row0=G, n_rows=1), dict(row0=5, n_rows=6), dict(row0=-1), dict(off=bad_off),
               dict(off=down_off), dict(off=None), dict(lab=None), dict(sep=b", "), dict(sep=b""), dict(cap=8), dict(outp=None),
               dict(orientation=2), dict(orientation=1, n_rows=5), dict(n_cells=0), dict(G=0)]
    for kw in refused:
        assert call(**kw) == _lib.ERR_ARG, kw
        assert L.icnv_last_error().startswith(b"format_table")
    assert (done.value, nbytes.value) == (-7, -7)
    assert dev.table_text_stats()["calls"] == 0 and not out.any().item()
    assert call() == _lib.OK and done.value == G and dev.table_text_stats()["calls"] == 1
    want = b"".join(bytes([97 + g]) + b" 1 1 1 1\n" for g in range(G))
    assert out[:nbytes.value].cpu().numpy().tobytes() == want
