"""rds.locate_counts on the host (no GPU, no library): where the count matrix of a serialised stream lies (DESIGN K34).  The
R-written data/infercnv_data_example.rda of the reference (tests/golden/infercnv_data_example.rda: a data.frame of 20 integer
columns x 8 252 genes) and files written here of all four kinds, formats 2 and 3, uncompressed / gzip / bzip2 / xz: kinds, names,
offsets and lengths agree with a full read_rds of the same file, the bytes at the recorded offsets decode to the same arrays
(tests/rds_counts_restate.py), and every refusal names its offender."""
import bz2
import gzip
import io
import lzma
import os
import struct

import numpy as np
import pytest
import scipy.sparse as sp

import rds_counts_restate as rs
from infercnv_amd import rds
from infercnv_amd.rds import RFactor, RS4, RValue

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "infercnv_data_example.rda")
G, C = 37, 5
GENES = np.array([f"g{k}" for k in range(G)], dtype=object)
CELLS = np.array([f"c{k}" for k in range(C)], dtype=object)


def dump(v):
    b = io.BytesIO()
    rds.write_rds(v, b, device=False)
    return b.getvalue()


def as_v2(b):
    """The same value as a format-2 stream: the header loses its encoding, the items are the same."""
    assert b[:6] == b"X\n" + struct.pack(">i", 3)
    return b"X\n" + struct.pack(">iII", 2, rds.WRITER_VERSION, 0x00020300) + b[23:]


def as_rda(variables):
    """An .rda container of {name: value}: values whose streams hold no symbol reference (every attribute name once)."""
    out = b"RDX3\n" + dump(None)[:23]
    for name, v in variables.items():
        b = name.encode()
        out += struct.pack(">I", 0x402) + struct.pack(">I", 1) + struct.pack(">Ii", 0x00040009, len(b)) + b + dump(v)[23:]
    return out + struct.pack(">I", 254)


def dense(seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 50, size=(G, C)).astype(np.float64)


def values():
    m = dense()
    m[3, 1] = 0.5
    s = sp.random(G, C, density=0.3, random_state=1, format="csc")
    s.data = np.ceil(s.data * 9)
    return {"matrix_real": RValue(m, {"dimnames": [GENES, CELLS]}),
            "matrix_int": RValue(dense(1).astype(np.int32), {"dimnames": [GENES, CELLS]}),
            "data_frame": RValue({str(c): (dense(2)[:, k].astype(np.int32) if k % 2 else dense(2)[:, k]) for k, c in enumerate(CELLS)},
                                 {"row.names": GENES, "class": "data.frame"}),
            "dgCMatrix": rds._matrix_value(s, GENES, CELLS)}


def payload_array(buf, p):
    return np.frombuffer(buf, dtype=">f8" if p.sexp == rds.REALSXP else ">i4", count=p.length, offset=p.offset)


def check_against_full_read(buf, loc, full):
    """loc (locate_counts of buf) against `full` (read_rds' value of the same stream)."""
    if loc.kind in ("matrix_real", "matrix_int"):
        m = full.value
        assert (loc.G, loc.C) == m.shape and loc.payloads[0].length == m.size
        assert loc.payloads[0].sexp == (rds.REALSXP if m.dtype.kind == "f" else rds.INTSXP)
        assert np.array_equal(payload_array(buf, loc.payloads[0]).reshape(loc.C, loc.G).T, m)
        assert loc.genes == list(full.attrs["dimnames"][0]) and loc.cells == list(full.attrs["dimnames"][1])
        off = [loc.payloads[0].offset + j * loc.G * loc.payloads[0].elem_size for j in range(loc.C)]
        kinds = [loc.payloads[0].sexp] * loc.C
        want = np.ascontiguousarray(m.T.astype(np.float64))
    elif loc.kind == "data_frame":
        cols = full.value
        assert loc.cells == list(cols) and loc.genes == list(full.attrs["row.names"]) and loc.C == len(cols)
        for p, col in zip(loc.payloads, cols.values()):
            assert p.length == loc.G == col.size and p.sexp == (rds.REALSXP if col.dtype.kind == "f" else rds.INTSXP)
            assert np.array_equal(payload_array(buf, p), col)
        off, kinds = [p.offset for p in loc.payloads], [p.sexp for p in loc.payloads]
        want = np.stack([np.asarray(col, dtype=np.float64) for col in cols.values()])
    else:
        sl = full.slots
        assert (loc.G, loc.C) == tuple(sl["Dim"]) and loc.nnz == sl["x"].size
        for p, name in zip(loc.payloads, ("i", "p", "x")):
            assert p.length == sl[name].size and np.array_equal(payload_array(buf, p), sl[name])
        assert loc.genes == list(sl["Dimnames"][0]) and loc.cells == list(sl["Dimnames"][1])
        i, p, x = loc.payloads
        bits = rs.column_bits(buf, x.offset, rs.REAL, x.length) if x.length else []
        ints = lambda q: [int(v) for v in payload_array(buf, q)]
        assert rs.csc_check(ints(i), ints(p), bits, loc.G, loc.C, loc.nnz) == (rs.OK, -1, -1)
        return
    # the restatement decodes the recorded offsets to what read_rds returns, bit for bit
    assert np.array_equal(rs.columns(buf, off, kinds, loc.G), want.view(np.uint64))


def test_r_written_data_frame():
    buf, route, _ = rds.open_counts(GOLDEN, device=False)
    assert route == "host"                                               # an R-written, gzip-compressed container
    loc = rds.locate_counts(buf)
    assert (rs.INT, rs.REAL) == (rds.INTSXP, rds.REALSXP)               # the restatement's kinds are the SEXP types
    assert (loc.kind, loc.G, loc.C, loc.container, loc.variable) == ("data_frame", 8252, 20, "rda", "infercnv_data_example")
    assert loc.genes[0] == "KIF1B" and loc.cells[0] == "normal_9" and len(set(loc.genes)) == 8252
    assert all(p.sexp == rds.INTSXP and p.length == 8252 and p.elem_size == 4 for p in loc.payloads)
    full = rds.read_rds(GOLDEN)["infercnv_data_example"]
    check_against_full_read(buf, loc, full)
    m = rs.columns(buf, [p.offset for p in loc.payloads], [p.sexp for p in loc.payloads], loc.G).view(np.float64)
    assert (m.sum(), m.min(), m.max()) == (2817798, 0, 6927)


@pytest.mark.parametrize("threshold", [rds.DEVICE_THRESHOLD, 16])
@pytest.mark.parametrize("compression", ["none", "gzip", "bzip2", "xz"])
@pytest.mark.parametrize("version", [3, 2])
@pytest.mark.parametrize("kind", ["matrix_real", "matrix_int", "data_frame", "dgCMatrix"])
def test_written_files(tmp_path, monkeypatch, kind, version, compression, threshold):
    monkeypatch.setattr(rds, "DEVICE_THRESHOLD", threshold)             # 16: no payload is decoded by the walk
    b = dump(values()[kind])
    b = b if version == 3 else as_v2(b)
    path = tmp_path / "counts.rds"
    path.write_bytes({"none": bytes, "gzip": gzip.compress, "bzip2": bz2.compress, "xz": lzma.compress}[compression](b))
    buf, route, _ = rds.open_counts(path, device=False)
    assert route == ("none" if compression == "none" else "host") and bytes(buf) == b
    loc = rds.locate_counts(buf)
    assert loc.kind == kind and loc.container is None
    decoded = [p.value is not None for p in loc.payloads]
    assert all(decoded) if threshold > 16 else not any(d for d, p in zip(decoded, loc.payloads) if p.nbytes >= 16)
    for p in loc.payloads:
        if p.value is not None:
            assert np.array_equal(p.value, payload_array(buf, p))
    check_against_full_read(buf, loc, rds.read_rds(path))
    rds.close_counts(buf)                                                # no view of the mapping is left behind by the walk
    assert compression != "none" or buf.closed


def test_offsets_are_byte_offsets_of_any_residue(tmp_path):
    """A version-3 header is 23 bytes, an .rda adds 5, and names of varying length precede a dgCMatrix's x."""
    seen = set()
    for n in range(16):
        genes = np.array([f"gene{'x' * n}{k}" for k in range(G)], dtype=object)
        v = values()["dgCMatrix"]
        v.slots["Dimnames"] = [genes, CELLS]
        buf = dump(v)
        loc = rds.locate_counts(buf)
        seen |= {p.offset % 16 for p in loc.payloads}
        (tmp_path / f"n{n}.rds").write_bytes(buf)
        check_against_full_read(buf, loc, rds.read_rds(tmp_path / f"n{n}.rds"))
    assert len(seen) >= 8


def test_rda_container_with_one_variable(tmp_path):
    v = values()["matrix_int"]
    b = as_rda({"counts": v})
    path = tmp_path / "counts.rda"
    path.write_bytes(b)
    loc = rds.locate_counts(b)
    assert (loc.kind, loc.container, loc.variable) == ("matrix_int", "rda", "counts")
    assert loc.payloads[0].offset == rds.locate_counts(dump(v)).payloads[0].offset + 5 + 4 + 4 + 8 + len("counts")
    check_against_full_read(b, loc, rds.read_rds(path)["counts"])


def test_rda_container_with_two_variables_is_refused():
    with pytest.raises(ValueError, match=r"2 variables \(a, b\)"):
        rds.locate_counts(as_rda({"a": values()["matrix_int"], "b": values()["matrix_real"]}))


def refused(v, match, **kw):
    with pytest.raises(ValueError, match=match):
        rds.locate_counts(dump(v), **kw)


def test_other_s4_classes_are_refused():
    v = values()["dgCMatrix"]
    for cls in ("dgTMatrix", "lgCMatrix", "ngCMatrix", "dgRMatrix"):
        refused(RS4(cls, "Matrix", v.slots), f"class '{cls}'")
    refused(RS4("infercnv", "infercnv", {"expr.data": values()["matrix_real"]}), "class 'infercnv'")


@pytest.mark.parametrize("column, what", [(RFactor(np.zeros(G, dtype=np.int64), ["a"]), "a factor"),
                                          (np.array(["a"] * G, dtype=object), "a character vector"),
                                          (np.zeros(G, dtype=bool), "a logical vector")])
def test_data_frame_columns_that_are_not_numbers_are_refused_by_name(column, what):
    refused(RValue({"c0": dense()[:, 0], "bad one": column}, {"row.names": GENES, "class": "data.frame"}), f"column 'bad one' of the data.frame is {what}")


def test_data_frame_columns_of_unequal_length_are_refused():
    refused(RValue({"c0": dense()[:, 0], "c1": dense()[:5, 0]}, {"row.names": GENES, "class": "data.frame"}), "column 'c1' of the data.frame has 5 rows, the first column has 37")


def test_matrix_with_further_attributes_is_refused():
    refused(RValue(dense(), {"dimnames": [GENES, CELLS], "tsp": np.array([1.0, 2.0, 3.0])}), "attributes tsp beyond dim and dimnames")
    refused(RValue(dense(), {"dimnames": [GENES, CELLS], "class": "table"}), "attributes class beyond dim and dimnames")
    refused(dense()[:, 0], "a numeric vector")
    refused({"a": 1}, "a list")


def test_missing_names_need_the_arguments():
    compact = RValue({"c0": dense()[:, 0], "c1": dense()[:, 1]}, {"row.names": np.array([-2 ** 31, -G], dtype=np.int32), "class": "data.frame"})
    refused(compact, "compact row.names")
    loc = rds.locate_counts(dump(compact), gene_names=list(GENES))
    assert loc.genes == list(GENES) and loc.cells == ["c0", "c1"]
    refused(compact, "36 names were passed, the matrix has 37", gene_names=list(GENES[:-1]))
    refused(dense(), "no row names: pass gene_names")
    refused(dense(), "no column names: pass cell_names", gene_names=list(GENES))
    loc = rds.locate_counts(dump(dense()), gene_names=list(GENES), cell_names=list(CELLS))
    assert (loc.genes, loc.cells) == (list(GENES), list(CELLS))
    refused(RValue(dense(), {"dimnames": [GENES, None]}), "no column names")
    v = values()["dgCMatrix"]
    v.slots["Dimnames"] = [None, None]
    refused(v, "no row names in Dimnames: pass gene_names")
    refused(v, "no column names in Dimnames: pass cell_names", gene_names=list(GENES))
    refused(v, "4 names were passed, the matrix has 5", gene_names=list(GENES), cell_names=list(CELLS[:-1]))
    assert rds.locate_counts(dump(v), gene_names=list(GENES), cell_names=list(CELLS)).cells == list(CELLS)
    passed = rds.locate_counts(dump(values()["matrix_int"]), gene_names=[f"x{k}" for k in range(G)])        # the arguments win
    assert passed.genes[0] == "x0" and passed.cells == list(CELLS)


def test_dgcmatrix_whose_slots_disagree_is_refused():
    v = values()["dgCMatrix"]
    v.slots["Dim"] = np.array([G, C + 1], dtype=np.int32)
    refused(v, "Dim says 6 columns, p has 6 entries")
    v = values()["dgCMatrix"]
    v.slots["x"] = v.slots["x"][:-1]
    refused(v, f"i has {v.slots['i'].size} entries, x has {v.slots['i'].size - 1}")
    v = values()["dgCMatrix"]
    v.slots["x"] = v.slots["x"].astype(np.int32)
    refused(v, "slot x of the dgCMatrix is an integer vector")


def test_truncated_stream_is_refused():
    b = dump(values()["matrix_real"])
    with pytest.raises(ValueError, match="truncated"):
        rds.locate_counts(b[:200])


@pytest.mark.parametrize("kind", ["matrix_int", "data_frame", "dgCMatrix"])
def test_sharded_create_takes_the_column_count_from_the_file(tmp_path, kind):
    """ShardedCreate's host logic on an .rds path, with a NumPy / SciPy reader in place of the device: C_file comes from
    locate_counts, and the ranks' objects are the single rank's, column for column."""
    import read_select_restate as rsr
    from infercnv_amd import sharded
    path = str(tmp_path / "counts.rds")
    v = values()[kind]
    if kind != "dgCMatrix":                                              # counts large enough to pass the cell filter
        v = RValue(v.value * 40 if kind == "matrix_int" else {k: c * 40 for k, c in v.value.items()}, v.attrs)
    else:
        v.slots["x"] = v.slots["x"] * 40
    with open(path, "wb") as f:
        f.write(dump(v))

    def reader(p, cells):
        full = rds.read_rds(p)
        if kind == "dgCMatrix":
            sl = full.slots
            m = sp.csc_matrix((sl["x"], sl["i"], sl["p"]), shape=tuple(sl["Dim"]))
            return list(sl["Dimnames"][0]), list(sl["Dimnames"][1]), m[:, list(cells)]
        if kind == "data_frame":
            m = np.stack([np.asarray(c, dtype=np.float64) for c in full.value.values()], axis=1)
            return list(full.attrs["row.names"]), list(full.value), np.ascontiguousarray(m[:, list(cells)].T)
        return list(full.attrs["dimnames"][0]), list(full.attrs["dimnames"][1]), np.ascontiguousarray(full.value[:, list(cells)].T.astype(np.float64))

    order = [(g, "chr1" if k < 20 else "chr2", 100 * k + 1, 100 * k + 50) for k, g in enumerate(GENES)]
    annot = [(c, "normal" if k % 2 == 0 else "tumor") for k, c in enumerate(CELLS)]
    make = lambda rank, world, deal="cyclic": sharded.ShardedCreate(path, order, annot, ["normal"], rank=rank, world=world, deal=deal, reader=reader)
    single, _, _ = make(0, 1).run()
    assert list(single.cell_names) == list(CELLS) and hasattr(single.expr_data, "tocsc") == (kind == "dgCMatrix")
    for how in ("cyclic", "block"):
        ranks = [make(r, 2, how) for r in range(2)]
        sums = ranks[0].place([r.read() for r in ranks])
        assert sums.size == C
        rsr.check_shards(single, [r.finish(sums) for r in ranks], C, 2, how)
    with pytest.raises(ValueError, match="world is 6, but the file has only 5 columns"):
        make(0, 6).read()


# ---- ALTREP, from bytes laid out by hand after R's serialize.c (as tests/test_rds_host.py does): what R >= 3.5 writes in format 3 ----
HEADER = bytes.fromhex("580A" "00000003" "00040000" "00030500" "00000005") + b"UTF-8"


def h(*words):
    return b"".join(bytes.fromhex(w) if isinstance(w, str) else w for w in words)


def char(s):
    return h("00040009") + struct.pack(">i", len(s)) + s.encode()


def sym(s):                                                              # every symbol in full: the streams hold no reference
    return h("00000001") + char(s)


def strs(*values):
    return h("00000010") + struct.pack(">i", len(values)) + b"".join(char(v) for v in values)


def ints(*values, flags="0000000D"):
    return h(flags) + struct.pack(">i", len(values)) + np.array(values, dtype=">i4").tobytes()


def reals(values, flags="0000000E"):
    return h(flags) + struct.pack(">i", len(values)) + np.array(values, dtype=">f8").tobytes()


def attributes(**named):
    return b"".join(h("00000402") + sym(k.replace("_", ".")) + v for k, v in named.items()) + h("000000FE")


def altrep(cls, sexptype, state, attr=None):
    """0xEE, info = pairlist(class symbol, package symbol, type), the state, the attributes."""
    info = h("00000002") + sym(cls) + h("00000002") + sym("base") + h("00000002") + ints(sexptype) + h("000000FE")
    return h("000000EE") + info + state + (attr if attr is not None else h("000000FE"))


def compact_intseq(n, start=1):
    return altrep("compact_intseq", 13, reals([n, start, 1]))


def deferred_string(arg):
    return altrep("deferred_string", 16, h("00000002") + arg + ints(0))  # CONS(arg, scalar)


VALS = [1.5, 2.0, 3.0, 4.0, 5.0, 6.25]


def located_matrix(stream, cells):
    loc = rds.locate_counts(stream)
    assert (loc.kind, loc.G, loc.C, loc.genes, loc.cells) == ("matrix_real", 2, 3, ["a", "b"], cells)
    assert len(loc.payloads) == 1 and loc.payloads[0].length == 6
    assert payload_array(stream, loc.payloads[0]).tolist() == VALS
    return loc


def test_altrep_deferred_string_dimnames(tmp_path):
    """colnames(m) <- 1:n leaves a deferred_string behind, over an expanded vector or over a compact_intseq."""
    for arg in (ints(1, 2, 3), compact_intseq(3)):
        dimnames = h("00000013", "00000002") + strs("a", "b") + deferred_string(arg)
        stream = HEADER + reals(VALS, "0000020E") + attributes(dim=ints(2, 3), dimnames=dimnames)
        located_matrix(stream, ["1", "2", "3"])
        (tmp_path / "m.rds").write_bytes(stream)
        full = rds.read_rds(tmp_path / "m.rds")                         # the host route reads the same
        assert list(full.attrs["dimnames"][1]) == ["1", "2", "3"] and full.value[:, 0].tolist() == VALS[:2]


def test_altrep_wrap_real_matrix():
    """The wrapped vector is a payload like any other, whether the attributes hang on the wrapper or on the vector."""
    names = h("00000013", "00000002") + strs("a", "b") + strs("x", "y", "z")
    outer = HEADER + altrep("wrap_real", 14, h("00000013", "00000002") + reals(VALS) + ints(0, 0), attributes(dim=ints(2, 3), dimnames=names))
    inner = HEADER + altrep("wrap_real", 14, h("00000013", "00000002") + reals(VALS, "0000020E") + attributes(dim=ints(2, 3), dimnames=names) + ints(0, 0))
    for stream in (outer, inner):
        loc = located_matrix(stream, ["x", "y", "z"])
        assert stream[loc.payloads[0].offset - 8:loc.payloads[0].offset - 4] in (h("0000000E"), h("0000020E"))


def test_altrep_compact_sequences_have_no_payload_and_are_refused_by_name():
    frame = lambda second, row_names: HEADER + h("00000313", "00000002") + reals(VALS[:3]) + second + attributes(
        names=strs("c0", "seq"), row_names=row_names, **{"class": strs("data.frame")})
    with pytest.raises(ValueError, match="column 'seq' of the data.frame is an ALTREP compact_intseq"):
        rds.locate_counts(frame(compact_intseq(3), strs("g0", "g1", "g2")))
    with pytest.raises(ValueError, match="ALTREP compact_intseq .* with the attributes dim"):      # matrix(1:6, 2)
        rds.locate_counts(HEADER + altrep("compact_intseq", 13, reals([6, 1, 1]), attributes(dim=ints(2, 3))))
    with pytest.raises(ValueError, match="ALTREP compact_realseq"):
        rds.locate_counts(HEADER + altrep("compact_realseq", 14, reals([6, 1, 1])))
    v = values()["dgCMatrix"]                                              # a slot: p = 0:C
    body = dump(rds.RS4("dgCMatrix", "Matrix", {k: s for k, s in v.slots.items() if k != "p"}))
    cut = body.rindex(h("00000402") + sym("class"))                       # the class attribute is written last: p goes in front of it
    with pytest.raises(ValueError, match="slot p of the dgCMatrix is an ALTREP compact_intseq"):
        rds.locate_counts(body[:cut] + h("00000402") + sym("p") + compact_intseq(C + 1, 0) + body[cut:])
    # row.names = 1:n as a compact sequence: no gene names, unless they are passed
    seq_rows = frame(reals(VALS[3:]), compact_intseq(3))
    with pytest.raises(ValueError, match="compact row.names"):
        rds.locate_counts(seq_rows)
    loc = rds.locate_counts(seq_rows, gene_names=["g0", "g1", "g2"])
    assert (loc.kind, loc.G, loc.C, loc.cells) == ("data_frame", 3, 2, ["c0", "seq"])
    assert [payload_array(seq_rows, p).tolist() for p in loc.payloads] == [VALS[:3], VALS[3:]]


def test_attributes_are_plain_arrays_in_a_refused_object():
    """A character matrix and a factor inside a list: their dim and levels are read as always, and the refusal names the list."""
    chars = h("00000210", "00000002") + char("u") + char("v") + attributes(dim=ints(1, 2))
    factor = ints(1, 1, flags="0000030D") + attributes(levels=strs("lvl"), **{"class": strs("factor")})
    with pytest.raises(ValueError, match="the file holds a list; a numeric matrix, a data.frame or a dgCMatrix is read"):
        rds.locate_counts(HEADER + h("00000013", "00000002") + chars + factor)
    with pytest.raises(ValueError, match="the file holds a character matrix; a numeric matrix, a data.frame or a dgCMatrix is read"):
        rds.locate_counts(HEADER + chars)
