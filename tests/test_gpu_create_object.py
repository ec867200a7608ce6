"""CreateInfercnvObject on the GPU (infercnv_amd/create_object.py, DESIGN K21) against the restatement of
tests/create_object_restate.py, end to end on the inputs of the reference's example/run.R (every eighth gene row of its
matrix: tests/golden/create_object_example/make_inputs.py).  Bit equality throughout."""
import gzip
import os

import numpy as np
import pytest

import create_object_restate as cor

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import infercnv_amd                                    # noqa: E402
from infercnv_amd import create_object as co           # noqa: E402

REFS = ["Microglia/Macrophage", "Oligodendrocytes (non-malignant)"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infercnv_amd import device
    torch.cuda.set_device(0)
    device.init(0)
    return device


@pytest.fixture(scope="module")
def example(golden_dir, tmp_path_factory):
    """The three input paths (the matrix as .gz and decompressed) and the restatement's reading of the matrix, made once."""
    d = os.path.join(golden_dir, "create_object_example")
    gz = os.path.join(d, "counts_every_8th_gene.matrix.gz")
    plain = str(tmp_path_factory.mktemp("example") / "counts.matrix")
    with gzip.open(gz, "rb") as src, open(plain, "wb") as dst:
        dst.write(src.read())
    genes, cells, x_bits = cor.read_table(plain)
    return {"gz": gz, "plain": plain, "genes": os.path.join(d, "gencode_downsampled.EXAMPLE_ONLY_DONT_REUSE.txt.gz"),
            "annot": os.path.join(d, "oligodendroglioma_annotations_downsampled.txt.gz"), "table": (genes, cells, x_bits)}


def test_example_equals_the_restatement_in_every_slot(dev, example):
    obj, x = infercnv_amd.CreateInfercnvObject(example["plain"], example["genes"], example["annot"], REFS, return_device=True)
    want = cor.create_object(*example["table"], example["genes"], example["annot"], REFS)
    cor.compare(obj, want)
    assert len(want["gene_names"]) > 1000 and len(want["cell_names"]) > 100 and len(want["obs_order"]) >= 2
    assert obj.options == {"chr_exclude": ["chrX", "chrY", "chrM"], "max_cells_per_group": None,
                           "min_max_counts_per_cell": [100, float("inf")], "counts_md5": None}
    assert tuple(x.shape) == obj.expr_data.T.shape and np.array_equal(x.cpu().numpy().view(np.int64), want["expr_bits"].T)
    assert obj.validate()


def test_gz_and_small_chunks_give_the_same_object(dev, example):
    want = cor.create_object(*example["table"], example["genes"], example["annot"], REFS)
    cor.compare(infercnv_amd.CreateInfercnvObject(example["gz"], example["genes"], example["annot"], REFS), want)
    cor.compare(infercnv_amd.CreateInfercnvObject(example["plain"], example["genes"], example["annot"], REFS, chunk_bytes=100000), want)


def test_options_change_the_object_as_in_the_restatement(dev, example):
    kw = dict(max_cells_per_group=20, min_max_counts_per_cell=(8000, 12000), chr_exclude=("chr1", "chrY"), seed=3)
    obj = infercnv_amd.CreateInfercnvObject(example["plain"], example["genes"], example["annot"], REFS[::-1], **kw)
    cor.compare(obj, cor.create_object(*example["table"], example["genes"], example["annot"], REFS[::-1], **kw))
    assert max(len(v) for v in obj.observation_grouped_cell_indices.values()) <= 20


def test_arrays_and_small_tables(dev):
    rng = np.random.default_rng(12)
    genes, cells = [f"g{i}" for i in range(40)], [f"c{j}" for j in range(30)]
    x = rng.integers(0, 50, size=(40, 30)).astype(np.float64)
    order = [(g, f"chr{1 + (i * 7) % 3}", 1000 - 13 * i, 1100 - 13 * i) for i, g in enumerate(genes) if i % 5]
    annot = [(c, "normal" if j % 3 == 0 else f"tumor{j % 2}") for j, c in enumerate(cells) if j != 4]
    obj = infercnv_amd.CreateInfercnvObject(x, order, annot, ["normal"], gene_names=genes, cell_names=cells)
    cor.compare(obj, cor.create_object(genes, cells, x.view(np.int64), order, annot, ["normal"]))

    class Sparse:                                       # what a scipy sparse matrix offers
        def toarray(self):
            return x
    cor.compare(infercnv_amd.CreateInfercnvObject(Sparse(), order, annot, ["normal"], gene_names=genes, cell_names=cells),
                cor.create_object(genes, cells, x.view(np.int64), order, annot, ["normal"]))


def test_duplicate_names_are_refused(dev, tmp_path):
    order, annot = [("g1", "chr1", 1, 2), ("g2", "chr1", 3, 4)], [("c1", "a"), ("c2", "b")]
    dup_gene = tmp_path / "dup_gene.tsv"
    dup_gene.write_text("c1\tc2\ng1\t1\t2\ng2\t3\t4\ng1\t5\t6\n")
    with pytest.raises(ValueError, match="duplicate 'row.names' are not allowed"):
        infercnv_amd.CreateInfercnvObject(str(dup_gene), order, annot, [], min_max_counts_per_cell=None)
    dup_cell = tmp_path / "dup_cell.tsv"
    dup_cell.write_text("c1\tc1\ng1\t1\t2\ng2\t3\t4\n")
    with pytest.raises(ValueError, match="duplicate cell name"):
        infercnv_amd.CreateInfercnvObject(str(dup_cell), order, [("c1", "a")], [], min_max_counts_per_cell=None)
    fine = tmp_path / "fine.tsv"
    fine.write_text("c1\tc2\ng1\t1\t2\ng2\t3\t4\n")
    with pytest.raises(ValueError, match="None of the genes"):
        infercnv_amd.CreateInfercnvObject(str(fine), [("zz", "chr1", 1, 2)], annot, [])
    obj = infercnv_amd.CreateInfercnvObject(str(fine), order, annot, [], min_max_counts_per_cell=None)
    assert obj.expr_data.tolist() == [[1.0, 2.0], [3.0, 4.0]] and list(obj.observation_grouped_cell_indices) == ["a", "b"]


def test_object_runs_through_the_first_steps(dev, example):
    """A smoke check, not a parity claim: steps 3 and 4 and the fused chain accept the object."""
    from infercnv_amd import ops
    obj = infercnv_amd.CreateInfercnvObject(example["plain"], example["genes"], example["annot"], REFS)
    obj = ops.log2xplus1(ops.normalize_counts_by_seq_depth(obj))
    out = ops.hip_smooth_chain(obj, window_length=21)
    assert out.expr_data.shape == obj.expr_data.shape and np.isfinite(out.expr_data).all()
