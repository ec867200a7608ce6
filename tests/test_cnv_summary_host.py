"""The restatement of add_to_seurat's feature table (tests/cnv_summary_restate.py) on the reference's HMM_states fixture and
on hand-made literals, and the pure-Python parts of infercnv_amd/seurat_interaction.py against it (no GPU, no library)."""
import os

import numpy as np
import pytest

import cnv_summary_restate as rs


def fixture_object(golden_dir):
    from infercnv_amd.infercnv_object import GeneOrder, InfercnvObject
    d = np.load(os.path.join(golden_dir, "infercnv_object_example.npz"))
    hs = np.load(os.path.join(golden_dir, "hmm_states_example.npz"))["HMM_states"]
    chr_names = d["chr_levels"][d["chr_codes"] - d["chr_codes"].min()]
    # the fixture's region counter starts at the tumour group: it comes first, the normal cells are a second group
    obj = InfercnvObject(expr_data=hs.astype(np.float64), gene_order=GeneOrder(chr_names, d["gene_start"], d["gene_stop"]),
                         reference_grouped_cell_indices={}, observation_grouped_cell_indices={"tumor": d["obs_tumor"], "normal": d["ref_normal"]},
                         tumor_subclusters={"subclusters": {"tumor": {"tumor_s1": d["obs_tumor"]}, "normal": {"normal_s1": d["ref_normal"]}}})
    return obj, hs, d


def genes_table(rows):
    """rows: (cell group, region name, state, chr, [(start, end)])."""
    t = {k: [] for k in ("cell_group_name", "gene_region_name", "state", "gene", "chr", "start", "end")}
    for grp, name, state, chrom, genes in rows:
        for k, (s, e) in enumerate(genes):
            for col, v in zip(t, (grp, name, state, f"{name}_g{k}", chrom, s, e)):
                t[col].append(v)
    return t


def span(first, n, step=500000):
    return [(first + k * step, first + k * step + 1000) for k in range(n)]


def top(t, sign_loss, s0=3, top_n=10, tol=2000000):
    a = rs._arrays(t)
    keep = a["state"] < s0 if sign_loss else a["state"] > s0
    return rs.get_top_n_regions(t, rs.sorted_regions(a["gene_region_name"][keep].tolist()), top_n, tol)


def test_fixture_nine_regions_one_loss(golden_dir):
    obj, hs, d = fixture_object(golden_dir)
    out = rs.run_on_object(obj, hs, "i6", by_cells=False)
    names = [str(n) for n in np.load(os.path.join(golden_dir, "mcmc_cell_gene.npz"))["names"]]
    assert out["tables"][0]["cnv_name"] == names
    assert [n for n, s in zip(out["tables"][0]["cnv_name"], out["tables"][0]["state"]) if s < 3] == ["chr4-region_8"]
    cells = out["cells"]
    tumour, normal = [cells[i] for i in d["obs_tumor"]], [cells[i] for i in d["ref_normal"]]
    assert len(out["top_loss"]) == 1 and len(out["top_dupli"]) == 8
    assert sorted(c for c, v in out["top_loss"][0].items() if v) == sorted(tumour) and len(tumour) == 10
    assert [lv for lv in out["levels"] if out["feats"]["has_loss"][lv][tumour[0]]] == ["chr4"]
    for f, per_level in out["feats"].items():
        for lv in out["levels"]:
            assert all(per_level[lv][c] == 0 for c in normal), (f, lv)
    genes4 = int((np.asarray(obj.gene_order.chr) == "chr4").sum())
    n_loss = out["tables"][1]["gene_region_name"].count("chr4-region_8")
    assert out["feats"]["proportion_loss"]["chr4"][tumour[0]] == n_loss / genes4
    assert out["top_losses.txt"][0] == f"top_loss_1;tumor.tumor_s1;{tumour[0]}" and len(out["top_losses.txt"]) == 10


def test_merge_within_tolerance_and_not_beyond():
    near = genes_table([("t.s1", "chr1-region_2", 2, "chr1", span(1, 30)), ("t.s2", "chr1-region_7", 1, "chr1", span(1 + 3 * 500000, 30))])
    t = top(near, True)
    assert len(t) == 1 and t[0]["regions_names"] == ["chr1-region_2", "chr1-region_7"] and t[0]["subclust_names"] == ["t.s1", "t.s2"]
    far = genes_table([("t.s1", "chr1-region_2", 2, "chr1", span(1, 30)), ("t.s2", "chr1-region_7", 1, "chr1", span(1 + 40 * 500000, 30))])
    t = top(far, True)
    assert [x["regions_names"] for x in t] == [["chr1-region_2"], ["chr1-region_7"]]
    # the window is taken on GENES: a longer region of another group joins when one of its genes starts inside the start window
    # and one of its genes ends inside the end window, whatever its own extent is
    inner = genes_table([("t.s1", "chr1-region_2", 2, "chr1", span(1 + 10 * 500000, 20)), ("t.s2", "chr1-region_7", 2, "chr1", span(1, 60))])
    t = top(inner, True, top_n=1)
    assert t[0]["regions_names"] == ["chr1-region_7"]                       # the largest seeds; its own window holds only itself
    other_chr = genes_table([("t.s1", "chr1-region_2", 2, "chr1", span(1, 30)), ("t.s2", "chr2-region_7", 2, "chr2", span(1, 30))])
    assert len(top(other_chr, True)) == 2


def test_gain_inside_the_window_joins_a_loss_seed():
    t = genes_table([("t.s1", "chr1-region_2", 2, "chr1", span(1, 30)), ("t.s2", "chr1-region_7", 5, "chr1", span(1 + 500000, 30)),
                     ("t.s3", "chr1-region_12", 4, "chr1", span(1 + 500000, 29))])
    loss = top(t, True)
    assert loss[0]["regions_names"] == ["chr1-region_2", "chr1-region_7", "chr1-region_12"]
    assert loss[0]["subclust_names"] == ["t.s1", "t.s2", "t.s3"]
    gain = top(t, False)                                                    # each call starts with nothing used
    assert len(gain) == 1 and gain[0]["regions_names"] == ["chr1-region_2", "chr1-region_7", "chr1-region_12"]


def test_fixed_point_needs_two_rounds():
    # B is within tolerance of A, C only of B: C joins in the second round, after the bounds were re-taken from {A, B}
    step = 3 * 500000
    t = genes_table([("t.s1", "chr1-region_2", 2, "chr1", span(1, 40)), ("t.s2", "chr1-region_7", 2, "chr1", span(1 + step, 39)),
                     ("t.s3", "chr1-region_12", 2, "chr1", span(1 + 2 * step, 38))])
    got = top(t, True)
    assert len(got) == 1 and got[0]["regions_names"] == ["chr1-region_2", "chr1-region_7", "chr1-region_12"]
    assert [x["regions_names"] for x in top(t, True, tol=step - 1)] == [["chr1-region_2"], ["chr1-region_7"], ["chr1-region_12"]]


def test_ties_in_size_are_taken_in_byte_order():
    assert [n for n, _ in rs.sorted_regions(["chr10-region_2"] * 3 + ["chr1-region_9"] * 3 + ["chr2-region_1"] * 4)] == \
        ["chr2-region_1", "chr1-region_9", "chr10-region_2"]
    t = genes_table([("t.s1", "chr10-region_2", 2, "chr10", span(1, 5)), ("t.s2", "chr1-region_9", 2, "chr1", span(1, 5))])
    assert [x["regions_names"] for x in top(t, True, top_n=1)] == [["chr1-region_9"]]


def three_cell_object():
    from infercnv_amd.infercnv_object import GeneOrder, InfercnvObject
    chrs = np.array(["chr1"] * 3 + ["chr2"] * 5000)
    pos = np.arange(5003) * 1000 + 1
    states = np.full((5003, 3), 3, dtype=np.int8)
    states[0:2, 0] = 1                                                      # 2 of 3 genes lost, two copies each
    states[3, 0] = 4                                                        # 1 of 5 000 genes gained
    obj = InfercnvObject(expr_data=states.astype(np.float64), gene_order=GeneOrder(chrs, pos, pos + 10),
                         reference_grouped_cell_indices={"n": np.array([2])}, observation_grouped_cell_indices={"t": np.array([0, 1])},
                         tumor_subclusters={"subclusters": {"n": {"n_s1": np.array([2])}, "t": {"t_s1": np.array([0])}}},
                         cell_names=np.array(["a", "b", "c"]))
    return obj, states


def test_file_format_on_a_three_cell_literal():
    obj, states = three_cell_object()
    out = rs.run_on_object(obj, states, "i6", by_cells=False)
    lines = out["lines"]
    head = lines[0].split("\t")
    assert head[:4] == ["subcluster", "has_cnv_chr1", "has_loss_chr1", "has_dupli_chr1"] and head[-2:] == ["top_loss_1", "top_dupli_1"]
    assert len(head) == 1 + 2 * 9 + 2 and all(len(ln.split("\t")) == len(head) + 1 for ln in lines[1:])
    a = lines[1].split("\t")
    assert a[:2] == ["a", "t_s1"]
    assert a[2:11] == ["1", "1", "0", "0.666666666666667", "0.666666666666667", "0", "0.666666666666667", "0.666666666666667", "0"]
    assert a[11:20] == ["1", "0", "1", "2e-04", "0", "2e-04", "1e-04", "0", "1e-04"] and a[20:] == ["1", "1"]
    assert lines[2].split("\t") == ["b", "NA"] + ["0"] * 20                  # in no subcluster: NA and zeros
    assert lines[3].split("\t")[:2] == ["c", "n_s1"]
    assert out["top_losses.txt"] == ["top_loss_1;t.t_s1;a"] and out["top_duplis.txt"] == ["top_dupli_1;t.t_s1;a"]
    i3 = rs.run_on_object(obj, np.where(states > 3, 3, np.where(states < 3, 1, 2)), "i3", by_cells=True)
    assert len(i3["lines"][0].split("\t")) == 1 + 2 * 6 + 2 and i3["top_losses.txt"] == ["top_loss_1;a;a"]


# ---- the pure-Python parts of the library against the restatement ---------------------------------------------------------
@pytest.mark.parametrize("mode", ["i6", "i3"])
def test_python_parts_against_the_restatement(mode):
    from infercnv_amd import seurat_interaction as si
    obj, states = rs.synthetic_object(120, 12, seed=5, mode=mode)
    want = rs.run_on_object(obj, states, mode, by_cells=True)
    s0 = si.CENTER_STATE[mode]
    _, chr_start = obj.chr_layout()
    order = np.concatenate([obj.reference_grouped_cell_indices["normal"], obj.observation_grouped_cell_indices["tumor"]])
    counts, rec = rs.counts_and_runs_np(states, chr_start, s0, order)
    feats = si.features_from_counts(counts, np.diff(chr_start), mode)
    levels = want["levels"]
    rec["name"] = [f"{levels[k]}-region_{o}" for k, o in zip(rec["chr"], rec["ordinal"])]
    assert rec["name"] == rs.uniq(want["tables"][1]["gene_region_name"])
    got = {"chr_names": np.array(levels), **feats}
    for sign, loss in (("loss", True), ("dupli", False)):
        tops = si.get_top_n_regions(rec, obj.gene_order.start, obj.gene_order.stop, s0, loss, 10, 2000000)
        vecs = []
        for _, owners in tops:
            v = np.zeros(len(want["cells"]), dtype=bool)
            v[order[owners]] = True
            vecs.append(v)
        got["top_" + sign] = vecs
    rs.assert_equal_to_library(want, got)
    assert len(want["top_loss"]) == 10 and len(want["top_dupli"]) == 10
    sub = si.subcluster_of_cells(obj)
    _, lines = si.format_table(obj.cells(), sub, got, mode)
    assert lines == want["lines"] and sub[obj.observation_grouped_cell_indices["tumor"][-1]] is None


def test_overlapping_subclusters_are_refused():
    from infercnv_amd import seurat_interaction as si
    obj, _ = rs.synthetic_object(40, 3, seed=1)
    obj.tumor_subclusters["subclusters"]["tumor"]["tumor_s2"] = np.append(obj.tumor_subclusters["subclusters"]["tumor"]["tumor_s2"],
                                                                        obj.tumor_subclusters["subclusters"]["tumor"]["tumor_s1"][0])
    with pytest.raises(ValueError):
        si._groups_and_map(obj, by_cells=False)
    with pytest.raises(ValueError):
        si.add_to_seurat(obj, None, "unused")
