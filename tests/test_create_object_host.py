"""The host decisions of CreateInfercnvObject (infercnv_amd/create_object.py, DESIGN K21) against the restatement of
tests/create_object_restate.py, on hand-made tables: .order_reduce, the annotation quirks, the group ordering, each error
text and the seeded down-sampling.  No GPU: the column sums are exact sums taken here."""
import math

import numpy as np
import pytest

import create_object_restate as cor
from infercnv_amd import create_object as co

GENES = ["g5", "gX", "g2", "g9", "g1", "gZ", "g7", "g3"]
CELLS = [f"c{j}" for j in range(1, 11)]
GENE_ORDER = [("g1", "chr2", 50, 90), ("g2", "chr1", 300, 400), ("g3", "chr2", 50, 60), ("gX", "chrX", 1, 2), ("g5", "chr1", 300, 350),
              ("g7", "chr3", 0, 0), ("g9", "chr2", 10, 20), ("gQ", "chr7", 5, 6), ("gZ", "chrM", 9, 10)]
ANNOT = [("c1", "tumor B"), ("c2", "normal"), ("c3", "tumor A"), ("c4", "tumor B"), ("c5", "normal"), ("c6", "other"), ("c8", "tumor A"),
         ("c9", "tumor B"), ("c10", "normal")]                      # c7 is not annotated


def matrix():
    rng = np.random.default_rng(3)
    x = rng.integers(0, 60, size=(len(GENES), len(CELLS))).astype(np.float64)
    x[:, 3] = 0.0                                                   # c4: below every count filter
    x[:, 8] *= 40.0                                                 # c9: above an upper bound
    return x


def library(genes, cells, x, gene_order, annot, refs, **kw):
    """The library's host functions chained as CreateInfercnvObject chains them, with exact column sums."""
    chr_exclude = kw.pop("chr_exclude", co.CHR_EXCLUDE)
    delim = kw.pop("delim", "\t")
    pos = co.read_gene_order(gene_order, chr_exclude)
    ann = co.read_annotations(annot, delim)
    if co._first_duplicate(genes) is not None:
        raise ValueError(co.ERR_DUP_ROW_NAMES)
    co.check_annotated_cells(cells, ann)
    rows, chrs, start, stop = co.order_reduce(genes, pos)
    if rows is None:
        raise ValueError(co.ERR_NO_GENES)
    xr = x[rows]
    cs = [math.fsum(xr[:, j].tolist()) for j in range(xr.shape[1])]
    columns, classes, ref, obs = co.select_cells(cells, cs, ann, refs, **kw)
    return {"expr_bits": np.ascontiguousarray(xr[:, columns]).view(np.int64), "gene_names": [genes[r] for r in rows],
            "cell_names": [cells[j] for j in columns], "chr": chrs, "start": start, "stop": stop,
            "ref": {k: v.tolist() for k, v in ref.items()}, "obs": {k: v.tolist() for k, v in obs.items()},
            "ref_order": list(ref), "obs_order": list(obs)}


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k == "expr_bits":
            assert np.array_equal(a[k], b[k])
        else:
            assert a[k] == b[k], k


def both(refs, **kw):
    x = matrix()
    got = library(GENES, CELLS, x, GENE_ORDER, ANNOT, refs, **dict(kw))
    want = cor.create_object(GENES, CELLS, x.view(np.int64), GENE_ORDER, ANNOT, refs, **dict(kw))
    same(got, want)
    return got


def test_order_reduce_and_groups():
    got = both(["normal"], min_max_counts_per_cell=(1, float("inf")))
    # chr levels in order of first appearance after the drops: chr2, chr1; stable order(chr, start, stop); gX, gZ excluded, g7 at 0 + 0
    assert got["gene_names"] == ["g9", "g3", "g1", "g5", "g2"]
    assert got["chr"] == ["chr2", "chr2", "chr2", "chr1", "chr1"]
    assert got["cell_names"] == ["c1", "c2", "c3", "c5", "c6", "c8", "c9", "c10"]          # c4 has no counts, c7 no annotation
    assert got["ref_order"] == ["normal"] and got["obs_order"] == ["other", "tumor A", "tumor B"]
    assert got["ref"]["normal"] == [1, 3, 7]


def test_reference_groups_keep_the_callers_order():
    got = both(["tumor B", "normal"], min_max_counts_per_cell=None)
    assert got["ref_order"] == ["tumor B", "normal"] and got["obs_order"] == ["other", "tumor A"]


def test_count_filter_bounds():
    got = both(["normal"], min_max_counts_per_cell=(0, 2000))       # low becomes max(1, 0); c9 is above 2000
    assert "c9" not in got["cell_names"] and "c4" not in got["cell_names"]
    both([], min_max_counts_per_cell=(100, float("inf")))


def test_no_chr_exclude_and_obs_sorted_by_bytes():
    got = both(None, chr_exclude=None, min_max_counts_per_cell=None)
    assert "gX" in got["gene_names"] and "gZ" in got["gene_names"] and got["ref_order"] == []
    x = matrix()
    ann = [("c1", "b"), ("c2", "B"), ("c3", "a"), ("c5", "é")]
    got = library(GENES, CELLS, x, GENE_ORDER, ann, [], min_max_counts_per_cell=None)
    same(got, cor.create_object(GENES, CELLS, x.view(np.int64), GENE_ORDER, ann, [], min_max_counts_per_cell=None))
    assert got["obs_order"] == ["B", "a", "b", "é"]


def test_v1_first_row_is_dropped():
    x = matrix()
    ann = [("V1", "V2")] + ANNOT
    got = library(GENES, CELLS, x, GENE_ORDER, ann, ["normal"], min_max_counts_per_cell=None)
    same(got, cor.create_object(GENES, CELLS, x.view(np.int64), GENE_ORDER, ann, ["normal"], min_max_counts_per_cell=None))
    assert "V2" not in got["obs_order"]


@pytest.mark.parametrize("seed", [0, 7])
def test_seeded_down_sampling(seed):
    got = both(["normal"], min_max_counts_per_cell=None, max_cells_per_group=2, seed=seed)
    sizes = {k: len(v) for k, v in {**got["ref"], **got["obs"]}.items()}
    assert sizes == {"normal": 2, "other": 1, "tumor A": 2, "tumor B": 2}
    other = both(["normal"], min_max_counts_per_cell=None, max_cells_per_group=1, seed=seed)
    assert all(len(v) == 1 for v in {**other["ref"], **other["obs"]}.values())


def test_files_read_like_tables(tmp_path):
    go, an = tmp_path / "genes.txt", tmp_path / "annot.txt"
    go.write_text("".join(f"{n}\t{c}\t{a}\t{b}\n" for n, c, a, b in GENE_ORDER) + "\n")
    an.write_text("".join(f"{c}\t{k}\r\n" for c, k in ANNOT))
    x = matrix()
    got = library(GENES, CELLS, x, str(go), str(an), ["normal"], min_max_counts_per_cell=None)
    same(got, cor.create_object(GENES, CELLS, x.view(np.int64), str(go), str(an), ["normal"], min_max_counts_per_cell=None))
    same(got, both(["normal"], min_max_counts_per_cell=None))


def raises_same(text, genes, cells, gene_order, annot, refs):
    x = np.ones((len(genes), len(cells)))
    with pytest.raises(ValueError) as lib:
        library(genes, cells, x, gene_order, annot, refs, min_max_counts_per_cell=None)
    with pytest.raises(ValueError) as ref:
        cor.create_object(genes, cells, x.view(np.int64), gene_order, annot, refs, min_max_counts_per_cell=None)
    assert text in str(lib.value) and text in str(ref.value)
    return str(lib.value), str(ref.value)


def test_error_texts():
    lib, ref = raises_same("Please make sure that all the annotated cell  names match a sample in your data matrix.  Attention to:  zz,yy",
                           GENES, CELLS, GENE_ORDER, ANNOT + [("zz", "normal"), ("yy", "other")], ["normal"])
    assert lib == ref
    lib, ref = raises_same("None of the genes in the expression data matched the genes in the reference genomic position file. "
                           "Analysis Stopped.", ["a", "b"], CELLS, GENE_ORDER, ANNOT, ["normal"])
    assert lib == ref
    raises_same("duplicate 'row.names' are not allowed", GENES[:3] + ["g5"], CELLS, GENE_ORDER, ANNOT, ["normal"])
    raises_same("duplicate 'row.names' are not allowed", GENES, CELLS, GENE_ORDER + [("g1", "chr1", 1, 2)], ANNOT, ["normal"])
    raises_same("duplicate 'row.names' are not allowed", GENES, CELLS, GENE_ORDER, ANNOT + [("c1", "normal")], ["normal"])
    raises_same("duplicate cell name", GENES, CELLS[:-1] + ["c1"], GENE_ORDER, ANNOT[:-1], ["normal"])
    raises_same("eference group", GENES, CELLS, GENE_ORDER, ANNOT, ["normal", "absent"])


def test_host_decisions_at_fifty_thousand_cells():
    """The name checks are linear: 5 x 10^4 cells, one annotation each, in well under a second (a quadratic check takes minutes)."""
    import time
    cells = [f"cell_{j:06d}" for j in range(50000)]
    ann = (cells[::-1], ["normal" if j % 4 == 0 else f"tumor{j % 3}" for j in range(50000)])
    t0 = time.perf_counter()
    co.check_annotated_cells(cells, ann)
    with pytest.raises(ValueError, match="Attention to:  zz"):
        co.check_annotated_cells(cells, (ann[0] + ["zz"], ann[1] + ["normal"]))
    columns, classes, ref, obs = co.select_cells(cells, np.full(50000, 500.0), ann, ["normal"])
    assert time.perf_counter() - t0 < 20.0
    assert columns.size == 50000 and ref["normal"].size == 12500 and list(obs) == ["tumor0", "tumor1", "tumor2"]


def test_package_exports_the_entry():
    import infercnv_amd
    assert infercnv_amd.CreateInfercnvObject is co.CreateInfercnvObject
    with pytest.raises(NotImplementedError):
        from infercnv_amd import device
        device.read_table("counts.rds")
