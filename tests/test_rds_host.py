"""infercnv_amd.rds on the host route (no GPU): literal bytes derived by hand from R's serialisation format, round trips over
the value model and over infercnv objects, the structure of an R-written infercnv object as a skeleton our file must
reproduce, R's own file read back, the refusals, and R's file names of rds_checkpoints."""
import gzip
import io
import json
import os
import struct
import sys

import numpy as np
import pytest

from infercnv_amd import GeneOrder, InfercnvObject, load_infercnv_obj, rds, save_infercnv_obj
from infercnv_amd.pipeline import checkpoint_file_names, rds_checkpoints
from infercnv_amd.rds import RFactor, RS4, RValue
from infercnv_amd.tumor_subclusters import HClust

REFERENCE = os.environ.get("INFERCNV_REFERENCE", "/root/reference")
HEADER = bytes.fromhex("580A" "00000003" "00040000" "00030500" "00000005") + b"UTF-8"
NA_REAL = np.array([0x7FF00000000007A2], dtype=np.uint64).view(np.float64)[0]
OTHER_NAN = np.array([0xFFF8000000000123], dtype=np.uint64).view(np.float64)[0]


def dump(v, **kw):
    b = io.BytesIO()
    rds.write_rds(v, b, device=False, **kw)
    return b.getvalue()


def h(*words):
    return b"".join(bytes.fromhex(w) if isinstance(w, str) else w for w in words)


def char(s):
    b = s.encode("utf-8")
    return h("00040009" if b.isascii() else "00008009") + struct.pack(">i", len(b)) + b


def sym(s):
    return h("00000001") + char(s)


# ---- literal bytes ---------------------------------------------------------------------------------------------------------
LITERALS = {
    "NULL": (None, h("000000FE")),
    "c(1L, NA)": (np.array([1, -2 ** 31], dtype=np.int32), h("0000000D", "00000002", "00000001", "80000000")),
    "c(1.5, NA_real_, -0, Inf)": (np.array([1.5, NA_REAL, -0.0, np.inf]),
                                  h("0000000E", "00000004", "3FF8000000000000", "7FF00000000007A2", "8000000000000000", "7FF0000000000000")),
    '"a"': ("a", h("00000010", "00000001") + char("a")),
    "non-ASCII": ("é", h("00000010", "00000001", "00008009", "00000002", "C3A9")),
    "NA_character_": (np.array([None], dtype=object), h("00000010", "00000001", "00000009", "FFFFFFFF")),
    "list(a = 1L)": ({"a": 1}, h("00000213", "00000001", "0000000D", "00000001", "00000001",
                                "00000402") + sym("names") + h("00000010", "00000001") + char("a") + h("000000FE")),
    "matrix": (RValue(np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]),
                      {"dimnames": [np.array(["r1", "r2"]), np.array(["c1", "c2", "c3"])]}),
               h("0000020E", "00000006") + np.array([1, 4, 2, 5, 3, 6], dtype=">f8").tobytes()
               + h("00000402") + sym("dim") + h("0000000D", "00000002", "00000002", "00000003")
               + h("00000402") + sym("dimnames") + h("00000013", "00000002", "00000010", "00000002") + char("r1") + char("r2")
               + h("00000010", "00000003") + char("c1") + char("c2") + char("c3") + h("000000FE")),
    "factor": (RFactor(np.array([0, 1, 0]), ["b", "a"]),
               h("0000030D", "00000003", "00000001", "00000002", "00000001", "00000402") + sym("levels")
               + h("00000010", "00000002") + char("b") + char("a") + h("00000402") + sym("class") + h("00000010", "00000001")
               + char("factor") + h("000000FE")),
    "S4": (RS4("k", "p", {"s": 1}),
           h("00010319", "00000402") + sym("s") + h("0000000D", "00000001", "00000001") + h("00000402") + sym("class")
           + h("00000210", "00000001") + char("k") + h("00000402") + sym("package") + h("00000010", "00000001") + char("p")
           + h("000000FE", "000000FE")),
}


@pytest.mark.parametrize("name", list(LITERALS))
def test_literal_bytes(name):
    value, body = LITERALS[name]
    assert dump(value) == HEADER + body


def test_docstring_example_and_symbol_reference():
    assert dump(np.array([1, -2 ** 31], dtype=np.int32)).hex() == (
        "580a" "00000003" "00040000" "00030500" "00000005" + b"UTF-8".hex() + "0000000d" "00000002" "00000001" "80000000")
    # the second `names` is a reference to symbol 1: (1 << 8) | 255
    got = dump([{"a": 1}, {"a": 1}])
    one = LITERALS["list(a = 1L)"][1]
    again = one.replace(sym("names"), h("000001FF"))
    assert got == HEADER + h("00000013", "00000002") + one + again


def test_many_strings():
    """Long pure-ASCII string vectors are assembled at once: the same bytes as string by string."""
    vals = [f"g{i}" * (i % 5) for i in range(1000)]
    for k in range(2):
        assert dump(np.array(vals, dtype=object)) == HEADER + h("00000010") + struct.pack(">i", 1000) + b"".join(char(s) for s in vals)
        vals[7] = "é"                                       # one non-ASCII string: the vector goes string by string


def test_long_vector_length_words():
    assert rds.length_words(0) == h("00000000")
    assert rds.length_words(2 ** 31 - 1) == h("7FFFFFFF")
    assert rds.length_words(2 ** 31) == h("FFFFFFFF", "00000000", "80000000")
    assert rds.length_words(10_000 * 250_000) == h("FFFFFFFF", "00000000") + struct.pack(">I", 2_500_000_000)
    assert rds.length_words(2 ** 32 + 5) == h("FFFFFFFF", "00000001", "00000005")
    rd = rds._Reader(rds.length_words(2 ** 40 + 7))
    assert rd.length() == 2 ** 40 + 7


# ---- round trips -----------------------------------------------------------------------------------------------------------
def same(a, b):
    """Deep equality over the value model: floats by bits, a scalar equal to the vector of length one it is written as."""
    if isinstance(a, RValue) or isinstance(b, RValue):
        return (isinstance(a, RValue) and isinstance(b, RValue) and same(a.value, b.value) and list(a.attrs) == list(b.attrs)
                and all(same(a.attrs[k], b.attrs[k]) for k in a.attrs))
    if isinstance(a, RS4) or isinstance(b, RS4):
        return (isinstance(a, RS4) and isinstance(b, RS4) and (a.cls, a.package) == (b.cls, b.package)
                and list(a.slots) == list(b.slots) and all(same(a.slots[k], b.slots[k]) for k in a.slots))
    if isinstance(a, RFactor) or isinstance(b, RFactor):
        return (isinstance(a, RFactor) and isinstance(b, RFactor) and np.array_equal(a.codes, b.codes)
                and list(a.levels) == list(b.levels) and same(a.attrs, b.attrs))
    if isinstance(a, dict) or isinstance(b, dict):
        return isinstance(a, dict) and isinstance(b, dict) and list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)) or isinstance(b, (list, tuple)):
        return (isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)) and len(a) == len(b)
                and all(same(x, y) for x, y in zip(a, b)))
    if a is None or b is None:
        return a is None and b is None
    a, b = np.atleast_1d(np.asarray(a)), np.atleast_1d(np.asarray(b))
    if a.shape != b.shape:
        return False
    if a.dtype.kind == "f" or b.dtype.kind == "f":
        return a.dtype.kind == b.dtype.kind and a.astype(np.float64).tobytes() == b.astype(np.float64).tobytes()
    if a.dtype.kind in "USO" or b.dtype.kind in "USO":
        return a.tolist() == b.tolist()
    return a.dtype.kind == b.dtype.kind and np.array_equal(a, b)


VALUES = {
    "null": None,
    "scalars": [True, 3, 2.5, "x", "é中"],
    "vectors": [np.array([True, False]), np.array([1, -2 ** 31, 7], dtype=np.int32), np.array([1.5, NA_REAL, OTHER_NAN, -0.0, 5e-324]),
                np.array(["a", None, ""], dtype=object), np.zeros(0), np.zeros(0, dtype=np.int32), np.array([], dtype=str)],
    "named": {"a": 1, "b": {"c": np.array([1.0, 2.0]), "d": None}, "e": []},
    "matrix": RValue(np.arange(12, dtype=np.float64).reshape(3, 4), {"dimnames": [None, np.array(list("wxyz"))]}),
    "int matrix": np.arange(6, dtype=np.int32).reshape(3, 2),
    "named vector": RValue(np.array([3, 1], dtype=np.int32), {"names": np.array(["p", "q"])}),
    "factor": RFactor(np.array([1, -1, 0]), ["u", "v"]),
    "data.frame": RValue({"x": np.array([1, 2], dtype=np.int32), "f": RFactor(np.array([0, 0]), ["k"])},
                         {"row.names": np.array(["g1", "g2"]), "class": np.array(["data.frame"])}),
    "S4": RS4("outer", "pkg", {"m": np.eye(2), "n": None, "inner": RS4("inner", "pkg", {"v": np.array(["s"])})}),
}


@pytest.mark.parametrize("name", list(VALUES))
@pytest.mark.parametrize("compress", [False, True])
def test_value_round_trip(tmp_path, name, compress):
    path = tmp_path / "v.rds"
    rds.write_rds(VALUES[name], path, compress=compress, device=False)
    raw = path.read_bytes()
    assert (raw[:2] == b"\x1f\x8b") == compress and (compress or raw[:2] == b"X\n")
    assert same(rds.read_rds(path), VALUES[name])
    assert not same(rds.read_rds(path), "something else")


def tree(n, labels, method="ward.D2"):
    merge = np.stack([-np.arange(1, n), np.arange(0, n - 1)], axis=1).astype(np.int32)
    merge[0, 1] = -n
    return HClust(merge, np.arange(1, n, dtype=np.float64) / 3, np.arange(n, 0, -1).astype(np.int32), np.asarray(labels), method)


def small_object(sparse_counts=False, with_hspike=True, seed=1):
    rng = np.random.default_rng(seed)
    G, C = 7, 6
    x = rng.normal(size=(G, C))
    x[0, 0], x[1, 2], x[2, 3], x[3, 4], x[4, 5] = NA_REAL, OTHER_NAN, -0.0, np.inf, 5e-324
    counts = rng.poisson(0.7, size=(G, C)).astype(np.float64)
    if sparse_counts:
        import scipy.sparse as sp
        counts = sp.csc_matrix(counts)
    cells = np.array([f"cellé_{i}" if i == 2 else f"c{i}" for i in range(C)])
    return InfercnvObject(
        expr_data=x, count_data=counts,
        gene_order=GeneOrder(np.array(["chr2", "chr2", "chr1", "chr1", "chr1", "chrX", "chrX"]), np.array([1, 5, 2.5, 9, 11, 3, 8]),
                             np.array([4, 7, 8, 10, 20, 6, 12])),
        reference_grouped_cell_indices={"ref": np.array([0, 4])}, observation_grouped_cell_indices={"obs": np.array([1, 2, 3, 5])},
        tumor_subclusters={"hc": {"obs": tree(4, cells[[1, 2, 3, 5]]), "ref": [tree(2, cells[[0, 4]]), None]},
                           "subclusters": {"obs": {"obs_s1": np.array([3, 1]), "obs_s2": np.array([5, 2])},
                                           "ref": {"ref_s1": np.array([0, 4]), "ref_s2": np.zeros(0, dtype=np.int64)}}},
        options={"out_dir": "o", "HMM": True, "k_nn": 20, "cutoff": 0.1, "noise_filter": None, "chr_exclude": ["chrX", "chrY"],
                 "final_scale_limits": [0.5, 1.5], "mixed": [1, "a", None], "nested": {"a": 1}},
        hspike=small_object(with_hspike=False, seed=2) if with_hspike else None,
        gene_names=np.array([f"g{i}" for i in range(G)]), cell_names=cells)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_option(a, b):
    """Options come back in Python's terms: scalars as scalars of the same type, vectors and lists as lists."""
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same_option(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, list) and len(a) == len(b) and all(same_option(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and (a == b or (a != a and b != b))


def assert_same_object(a, b):
    assert np.array_equal(bits(a.expr_data), bits(b.expr_data))
    if hasattr(a.count_data, "tocsc"):
        assert hasattr(b.count_data, "tocsc") and b.count_data.format == "csc"
        ac = a.count_data.tocsc()
        assert np.array_equal(ac.indptr, b.count_data.indptr) and np.array_equal(ac.indices, b.count_data.indices)
        assert np.array_equal(bits(ac.data), bits(b.count_data.data)) and ac.shape == b.count_data.shape
    elif a.count_data is None:
        assert b.count_data is None
    else:
        assert np.array_equal(np.asarray(a.count_data), np.asarray(b.count_data))
    assert [str(c) for c in a.gene_order.chr] == [str(c) for c in b.gene_order.chr]
    for k in ("start", "stop"):
        assert np.array_equal(np.asarray(getattr(a.gene_order, k), dtype=np.float64), np.asarray(getattr(b.gene_order, k), dtype=np.float64))
    for k in ("reference_grouped_cell_indices", "observation_grouped_cell_indices"):
        ga, gb = getattr(a, k), getattr(b, k)
        assert list(ga) == list(gb) and all(np.array_equal(ga[g], gb[g]) for g in ga)
    if a.tumor_subclusters is None:
        assert b.tumor_subclusters is None
    else:
        ta, tb = a.tumor_subclusters, b.tumor_subclusters
        assert list(ta["subclusters"]) == list(tb["subclusters"])
        for g in ta["subclusters"]:
            assert list(ta["subclusters"][g]) == list(tb["subclusters"][g])
            for s in ta["subclusters"][g]:
                assert np.array_equal(ta["subclusters"][g][s], tb["subclusters"][g][s])      # 0-based on both sides
        assert list(ta["hc"]) == list(tb["hc"])
        for g in ta["hc"]:
            la, lb = ta["hc"][g], tb["hc"][g]
            assert isinstance(la, list) == isinstance(lb, list)
            for x, y in zip(la if isinstance(la, list) else [la], lb if isinstance(lb, list) else [lb]):
                if x is None:
                    assert y is None
                    continue
                assert np.array_equal(x.merge, y.merge) and y.merge.shape == x.merge.shape
                assert np.array_equal(bits(x.height), bits(y.height)) and np.array_equal(x.order, y.order)
                assert list(x.labels) == list(y.labels) and (x.method, x.dist_method) == (y.method, y.dist_method)
    assert same_option(a.options, b.options), (a.options, b.options)
    assert list(a.genes()) == list(b.genes()) and list(a.cells()) == list(b.cells())
    assert (a.hspike is None) == (b.hspike is None)
    if a.hspike is not None:
        assert_same_object(a.hspike, b.hspike)


@pytest.mark.parametrize("sparse_counts", [False, True])
def test_object_round_trip(tmp_path, sparse_counts):
    obj = small_object(sparse_counts)
    path = tmp_path / "o.rds"
    save_infercnv_obj(obj, path, device=False)
    back = load_infercnv_obj(path)
    assert_same_object(obj, back)
    assert back.gene_order.start.dtype.kind == "f" and back.gene_order.stop.dtype.kind == "i"    # 2.5 keeps `start` double
    # in the file: 1-based indices, named by the cells
    raw = rds.read_rds(path)
    sub = raw.slots["tumor_subclusters"]["subclusters"]["obs"]["obs_s2"]
    assert sub.value.tolist() == [6, 3] and sub.attrs["names"].tolist() == [obj.cell_names[5], obj.cell_names[2]]
    assert raw.slots["reference_grouped_cell_indices"]["ref"].tolist() == [1, 5]
    assert raw.slots["tumor_subclusters"]["hc"]["ref"][1] is None
    assert raw.slots["tumor_subclusters"]["hc"]["obs"].value["call"] is None
    assert list(raw.slots) == list(rds.SLOTS)
    if sparse_counts:
        assert raw.slots["count.data"].cls == "dgCMatrix" and list(raw.slots["count.data"].slots) == ["i", "p", "Dim", "Dimnames", "x", "factors"]
    gz = tmp_path / "o.gz.rds"
    save_infercnv_obj(obj, gz, compress=True, device=False)
    assert gzip.decompress(gz.read_bytes()) == path.read_bytes()
    assert_same_object(obj, load_infercnv_obj(gz))


def test_slot_the_mirror_cannot_hold(tmp_path):
    v = rds.to_r(small_object())
    for slot, bad in (("expr.data", np.array(["a"])), ("count.data", RS4("lgCMatrix", "Matrix", {})),
                      ("tumor_subclusters", {"hc": {"g": 3.0}, "subclusters": {}}), ("options", np.array([1.0]))):
        w = RS4(v.cls, v.package, {**v.slots, slot: bad})
        rds.write_rds(w, tmp_path / "bad.rds", device=False)
        with pytest.raises(ValueError, match=slot.replace(".", r"\.")):
            load_infercnv_obj(tmp_path / "bad.rds")
    rds.write_rds(RS4(v.cls, v.package, {**v.slots, "extra": 1}), tmp_path / "bad.rds", device=False)
    with pytest.raises(ValueError, match="extra"):
        load_infercnv_obj(tmp_path / "bad.rds")


# ---- against R's own bytes -------------------------------------------------------------------------------------------------
def example_object(golden_dir):
    d = np.load(os.path.join(golden_dir, "infercnv_object_example.npz"))
    G, C = d["expr_data"].shape
    cells = np.array([f"cell_{i + 1}" for i in range(C)])
    chr_names = d["chr_levels"][d["chr_codes"] - d["chr_codes"].min()]
    ref, obs = d["ref_normal"], d["obs_tumor"]
    return d, InfercnvObject(
        expr_data=d["expr_data"], count_data=d["count_data"].astype(np.int32), gene_order=GeneOrder(chr_names, d["gene_start"], d["gene_stop"]),
        reference_grouped_cell_indices={"normal": ref}, observation_grouped_cell_indices={"tumor": obs},
        tumor_subclusters={"hc": {"tumor": tree(obs.size, cells[obs]), "normal": tree(ref.size, cells[ref])},
                           "subclusters": {"tumor": {"tumor_s1": obs}, "normal": {"normal_s1": ref}}},
        options={"chr_exclude": ["chrX", "chrY", "chrM"], "max_cells_per_group": None, "min_max_counts_per_cell": None,
                 "counts_md5": "0" * 32, "cutoff": 1.0, "out_dir": "out", "cluster_by_groups": True, "HMM": False, "denoise": True,
                 "num_threads": 2.0, "no_plot": True})


def test_skeleton_of_the_r_written_object(tmp_path, golden_dir):
    """Our file of the example object, decoded by the reader that decoded R's file, has the structure of R's file."""
    sys.path.insert(0, golden_dir)
    import make_rds_skeleton as mk
    with open(os.path.join(golden_dir, "rds_skeleton_infercnv_object_example.json")) as fh:
        want = json.load(fh)
    _, obj = example_object(golden_dir)
    save_infercnv_obj(obj, tmp_path / "example.rds", device=False)
    got = json.loads(json.dumps(mk.skeleton(mk.decode(str(tmp_path / "example.rds")))))
    assert got["attributes"] == want["attributes"] == list(rds.SLOTS) + ["class"]
    assert got == want


@pytest.mark.skipif(not os.path.exists(os.path.join(REFERENCE, "data", "infercnv_object_example.rda")), reason="the reference is not here")
def test_r_written_file_read_back(golden_dir):
    d, _ = example_object(golden_dir)
    obj = load_infercnv_obj(os.path.join(REFERENCE, "data", "infercnv_object_example.rda"))
    assert np.array_equal(bits(obj.expr_data), bits(d["expr_data"])) and obj.expr_data.shape == d["expr_data"].shape
    assert np.array_equal(bits(obj.count_data), bits(d["count_data"]))
    assert np.array_equal(obj.reference_grouped_cell_indices["normal"], d["ref_normal"])
    assert np.array_equal(obj.observation_grouped_cell_indices["tumor"], d["obs_tumor"])
    assert list(obj.reference_grouped_cell_indices) == ["normal"] and list(obj.observation_grouped_cell_indices) == ["tumor"]
    assert list(obj.gene_order.chr) == list(d["chr_levels"][d["chr_codes"] - d["chr_codes"].min()])
    assert np.array_equal(obj.gene_order.start, d["gene_start"]) and np.array_equal(obj.gene_order.stop, d["gene_stop"])
    assert obj.hspike is None and obj.options["cutoff"] == 1.0 and obj.options["max_cells_per_group"] is None
    assert isinstance(obj.tumor_subclusters["hc"]["tumor"], HClust) and obj.tumor_subclusters["hc"]["tumor"].merge.shape == (9, 2)
    top = rds.read_rds(os.path.join(REFERENCE, "data", "infercnv_object_example.rda"))
    assert isinstance(top["infercnv_object_example"].slots["tumor_subclusters"]["hc"]["tumor"].value["call"], rds.RLang)


def test_altrep_reference_and_format_2(tmp_path):
    """What R emits and this library does not write, from bytes laid out by hand after R's serialize.c: the ALTREP item is
    0xEE, then info = pairlist(class symbol, package symbol, type), the state, the attributes."""
    def info(cls, sexptype):
        return (h("00000002") + sym(cls) + h("00000002") + sym("base") + h("00000002", "0000000D", "00000001")
                + struct.pack(">i", sexptype) + h("000000FE"))

    def info_again(sexptype):      # the class and package symbols a second time: references 1 and 2
        return h("00000002", "000001FF", "00000002", "000002FF", "00000002", "0000000D", "00000001") + struct.pack(">i", sexptype) + h("000000FE")

    path = tmp_path / "a.rds"
    intseq = h("000000EE") + info("compact_intseq", 13) + h("0000000E", "00000003") + np.array([4, 3, 1], dtype=">f8").tobytes() + h("000000FE")
    path.write_bytes(HEADER + h("00000013", "00000002") + intseq + h("000000EE") + info_again(13) + h("0000000E", "00000003")
                     + np.array([2, 9, -1], dtype=">f8").tobytes() + h("000000FE"))
    a, b = rds.read_rds(path)
    assert a.dtype == np.int32 and a.tolist() == [3, 4, 5, 6] and b.tolist() == [9, 8]
    wrapped = (h("000000EE") + info("wrap_real", 14) + h("00000013", "00000002", "0000000E", "00000002") + np.array([1.5, NA_REAL], dtype=">f8").tobytes()
               + h("0000000D", "00000002", "00000000", "00000000") + h("000000FE"))
    path.write_bytes(HEADER + wrapped)
    assert np.array_equal(rds.read_rds(path).view(np.uint64), np.array([1.5, NA_REAL]).view(np.uint64))
    deferred = (h("000000EE") + info("deferred_string", 16) + h("00000002", "0000000D", "00000003", "00000007", "80000000", "0000002A")
                + h("0000000D", "00000001", "00000000") + h("000000FE"))
    path.write_bytes(HEADER + deferred)
    assert rds.read_rds(path).tolist() == ["7", None, "42"]
    path.write_bytes(HEADER + h("000000EE") + info("mmap_real", 14) + h("000000FE", "000000FE"))
    with pytest.raises(ValueError, match=r"mmap_real.*type 238\) at byte 23"):
        rds.read_rds(path)
    # format 2 has no encoding in its header; a latin-1 string is marked by gp bit 4
    path.write_bytes(h("580A", "00000002", "00030404", "00020300", "00000010", "00000001", "00004009", "00000001", "E9"))
    assert rds.read_rds(path).tolist() == ["é"]
    path.write_bytes(h("580A", "00000004", "00030404", "00020300", "000000FE"))
    with pytest.raises(ValueError, match="version 4"):
        rds.read_rds(path)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_unknown_type_and_truncation(tmp_path):
    path = tmp_path / "x.rds"
    path.write_bytes(HEADER + h("00000013", "00000002", "000000FE", "00000004"))       # an ENVSXP at byte 35
    with pytest.raises(ValueError, match=r"type 4 at byte 35"):
        rds.read_rds(path)
    whole = dump(small_object().expr_data)
    for cut in (1, 10, len(HEADER) + 2, len(HEADER) + 6, len(whole) - 1, len(whole) - 30):
        path.write_bytes(whole[:cut])
        with pytest.raises(ValueError, match="truncated"):
            rds.read_rds(path)
    path.write_bytes(b"")
    with pytest.raises(ValueError):
        rds.read_rds(path)
    path.write_bytes(gzip.compress(whole)[:-20])
    with pytest.raises(ValueError):
        rds.read_rds(path)
    path.write_bytes(b"A\n" + whole[2:])
    with pytest.raises(ValueError, match="XDR"):
        rds.read_rds(path)


# ---- rds_checkpoints: R's file names (the sprintf patterns of R/inferCNV_ops.R:3316-3492) ------------------------------------
COMMON = {1: "01_incoming_data.infercnv_obj", 2: "02_reduced_by_cutoff.infercnv_obj"}
NAME_CASES = [
    (dict(denoise=True),
     {**COMMON, 3: "03_normalized_by_depth.infercnv_obj", 4: "04_logtransformed.infercnv_obj", 5: "05_scaled.infercnv_obj",
      8: "08_remove_ref_avg_from_obs_logFC.infercnv_obj", 9: "09_apply_max_centered_expr_threshold.infercnv_obj",
      10: "10_smoothed_by_chr.infercnv_obj", 11: "11_recentered_cells_by_chr.infercnv_obj",
      12: "12_remove_ref_avg_from_obs_adjust.infercnv_obj", 14: "14_invert_log_transform.infercnv_obj",
      15: "15_tumor_subclusters.leiden.infercnv_obj", 22: "22_denoise.leiden.NF_NA.SD_1.5.NL_FALSE.infercnv_obj"}),
    (dict(HMM=True, HMM_type="i6", tumor_subcluster_partition_method="random_trees", num_ref_groups=2, denoise=True, noise_filter=0.1,
          mask_nonDE_genes=True, prune_outliers=True, remove_genes_at_chr_ends=True),
     {**COMMON, 3: "03_normalized_by_depthHMMi6.infercnv_obj", 4: "04_logtransformedHMMi6.infercnv_obj", 5: "05_scaledHMMi6.infercnv_obj",
      6: "06_split_HMMi6f_refs2.infercnv_obj", 7: "07_tumor_subclustersHMMi6.rand_trees.random_trees.infercnv_obj",
      8: "08_remove_ref_avg_from_obs_logFCHMMi6.rand_trees.infercnv_obj",
      9: "09_apply_max_centered_expr_thresholdHMMi6.rand_trees.infercnv_obj", 10: "10_smoothed_by_chrHMMi6.rand_trees.infercnv_obj",
      11: "11_recentered_cells_by_chrHMMi6.rand_trees.infercnv_obj", 12: "12_remove_ref_avg_from_obs_adjustHMMi6.rand_trees.infercnv_obj",
      13: "13_remove_gene_at_chr_endsHMMi6.rand_trees.infercnv_obj", 14: "14_invert_log_transformHMMi6.rand_trees.infercnv_obj",
      16: "16_remove_outlierHMMi6.rand_trees.infercnv_obj", 17: "17_HMM_predHMMi6.rand_trees.hmm_mode-subclusters.infercnv_obj",
      18: "18_HMM_pred.Bayes_NetHMMi6.rand_trees.hmm_mode-subclusters.mcmc_obj",
      19: "19_HMM_pred.Bayes_NetHMMi6.rand_trees.hmm_mode-subclusters.Pnorm_0.5.infercnv_obj",
      20: "20_HMM_pred.repr_intensitiesHMMi6.rand_trees.hmm_mode-subclusters.Pnorm_0.5.infercnv_obj",
      21: "21_mask_nonDEHMMi6.rand_trees.infercnv_obj", 22: "22_denoiseHMMi6.rand_trees.NF_0.1.SD_1.5.NL_FALSE.infercnv_obj"}),
    (dict(HMM=True, HMM_type="i3", analysis_mode="samples", BayesMaxPNormal=0, max_centered_threshold=None, denoise=True,
          noise_logistic=True, sd_amplifier=2),
     {**COMMON, 3: "03_normalized_by_depthHMMi3.infercnv_obj", 4: "04_logtransformedHMMi3.infercnv_obj", 5: "05_scaledHMMi3.infercnv_obj",
      8: "08_remove_ref_avg_from_obs_logFCHMMi3.infercnv_obj", 10: "10_smoothed_by_chrHMMi3.infercnv_obj",
      11: "11_recentered_cells_by_chrHMMi3.infercnv_obj", 12: "12_remove_ref_avg_from_obs_adjustHMMi3.infercnv_obj",
      14: "14_invert_log_transformHMMi3.infercnv_obj", 15: "15_no_subclusteringHMMi3.infercnv_obj",
      17: "17_HMM_predHMMi3.hmm_mode-samples.infercnv_obj", 20: "20_HMM_pred.repr_intensitiesHMMi3.hmm_mode-samples.Pnorm_0.infercnv_obj",
      22: "22_denoiseHMMi3.NF_NA.SD_2.NL_TRUE.infercnv_obj"}),
]


@pytest.mark.parametrize("case", range(len(NAME_CASES)))
def test_rds_checkpoints_names(tmp_path, case, caplog):
    args, want = NAME_CASES[case]
    assert checkpoint_file_names(**args) == want
    saved = []

    def saver(obj, path):
        saved.append(obj)
        with open(path, "w") as fh:
            fh.write(obj)

    hook = rds_checkpoints(str(tmp_path), saver=saver, **args, out_dir_ignored=1, seed=3)
    ran = [s for s in range(1, 23) if s in want and s != 5]                 # scale_data is off: step 5 does not report
    with caplog.at_level("INFO", logger="infercnv_amd"):
        for s in ran:
            hook(s, "label", f"object of step {s}")
    written = {s: want[s] for s in ran if s != 18}
    assert sorted(os.listdir(tmp_path)) == sorted(list(written.values()) + ["preliminary.infercnv_obj", "run.final.infercnv_obj"])
    assert saved == [f"object of step {s}" for s in ran if s != 18]          # every object encoded once
    assert sum("MCMCInferCNV" in r.getMessage() for r in caplog.records) == (1 if 18 in ran else 0)
    read = lambda name: open(os.path.join(tmp_path, name)).read()
    assert all(read(name) == f"object of step {s}" for s, name in written.items())
    assert read("preliminary.infercnv_obj") == f"object of step {15 if 15 in ran else 14}"
    assert read("run.final.infercnv_obj") == f"object of step {max(s for s in ran if s not in (17, 18, 19, 20))}"

    final_dir = tmp_path / "final"
    final_dir.mkdir()
    saved.clear()
    hook = rds_checkpoints(str(final_dir), "final", saver=saver, **args)
    for s in ran:
        hook(s, "label", f"object of step {s}")
    assert sorted(os.listdir(final_dir)) == ["preliminary.infercnv_obj", "run.final.infercnv_obj"]
    read = lambda name: open(os.path.join(final_dir, name)).read()
    assert read("preliminary.infercnv_obj") == f"object of step {15 if 15 in ran else 14}"
    assert read("run.final.infercnv_obj") == f"object of step {max(s for s in ran if s not in (17, 18, 19, 20))}"
    assert saved == [f"object of step {s}" for s in ran if s in (14, 15, 16, 21, 22)]
