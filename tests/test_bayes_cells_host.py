"""The host side of the table route of steps 18-19 (DESIGN K25): the vectorised region tokens against fnv1a64 of the names,
RegionTable's cell lists and group numbers against the dict route's loop on a mock of the run records, and the lazy
sequences.  No GPU."""
import numpy as np
import pytest

import bayes_restate as br


def test_tokens_equal_fnv1a64_of_the_name():
    from infercnv_amd import bayes_net
    chr_names = np.array(["chr1", "chrX", "MT", "1", "GL000219.1", "chr-é"])
    edges = [1, 2, 9, 10, 11, 99, 100, 101, 999, 1000, 9999, 10000, 99999, 100000, 999999, 1000000, 9999999, 10000000]
    chr_i, ordinal = (a.ravel() for a in np.meshgrid(np.arange(chr_names.size), np.array(edges), indexing="ij"))
    got = bayes_net.region_tokens(chr_names, chr_i, ordinal)
    assert got.dtype == np.uint64 and got.shape == ordinal.shape
    want = np.array([br.fnv1a64(f"{chr_names[c]}-region_{o}") for c, o in zip(chr_i, ordinal)], dtype=np.uint64)
    assert np.array_equal(got, want)
    assert len(set(want.tolist())) == want.size                                     # the fixture tells every name apart
    assert bayes_net.region_tokens(chr_names, [], []).shape == (0,)
    with pytest.raises(ValueError):
        bayes_net.region_tokens(chr_names, [0], [10 ** 10])


def mock_records():
    """Five cell groups (one empty, one unsorted, one without a region, one whose cells lie beyond the observations) and
    eight run records in report order; gene runs in a gathered order whose perm keeps every run contiguous."""
    groups = [("ref", np.array([0, 1], dtype=np.int32)), ("a.s1", np.array([7, 3, 5], dtype=np.int32)),
              ("a.s2", np.zeros(0, dtype=np.int32)), ("b.s1", np.array([4, 2], dtype=np.int32)), ("b.s2", np.array([6, 9, 8], dtype=np.int32))]
    chr_names = np.array(["chr2", "chr1"])
    perm = np.concatenate([np.arange(10, 20), np.arange(0, 10)])                    # chr2 first appeared at row 10
    rec = np.array([[0, 0, 2, 4, 5, 2], [1, 0, 0, 0, 255, 1], [1, 1, 10, 19, 2, 3], [2, 0, 5, 9, 4, 2],
                    [4, 0, 1, 1, 6, 2], [4, 0, 8, 9, 1, 4], [4, 1, 10, 10, 5, 5], [4, 1, 15, 18, 4, 7]], dtype=np.int64).T
    return groups, chr_names, perm, rec


def dict_route(groups, chr_names, perm, rec, n_obs):
    """inferCNVBayesNet's loop over groups and regions, on the records."""
    cell_gene, group_id, gid = [], np.full(n_obs, np.iinfo(np.int32).min, dtype=np.int64), 0
    for gi, (_, idx) in enumerate(groups):
        cols = np.sort(np.asarray(idx, dtype=np.int64))
        mine = [r for r in range(rec.shape[1]) if rec[0, r] == gi]
        if not mine:
            continue
        gid += 1
        group_id[cols[cols < n_obs]] = gid
        for r in mine:
            cell_gene.append({"cnv_regions": f"{chr_names[rec[1, r]]}-region_{rec[5, r]}", "Genes": perm[np.arange(rec[2, r], rec[3, r] + 1)],
                              "Cells": cols.copy(), "State": -1 if rec[4, r] == 255 else int(rec[4, r])})
    return cell_gene, group_id


def test_region_table_against_the_dict_route_on_mock_records():
    from infercnv_amd import bayes_net
    groups, chr_names, perm, rec = mock_records()
    assert any(len(g) == 0 for _, g in groups) and any(np.any(np.diff(g) < 0) for _, g in groups if len(g) > 1)
    assert set(range(len(groups))) - set(rec[0].tolist()) == {3} and (rec[4] == 255).any()
    n_obs = 9                                                                       # cell 9 lies beyond the observations
    want, want_gid = dict_route(groups, chr_names, perm, rec, n_obs)
    t = bayes_net.RegionTable.from_records(groups, chr_names, perm, rec)
    assert len(t) == len(want) == 8
    assert t.cell_off.dtype == np.int64 and t.cell_idx.dtype == np.int32 and t.token.dtype == np.uint64
    assert np.array_equal(t.cell_off, np.concatenate([[0], np.cumsum([len(w["Cells"]) for w in want])]))
    assert np.array_equal(t.cell_idx, np.concatenate([w["Cells"] for w in want]))
    assert np.array_equal(t.group_id(n_obs), want_gid) and (want_gid == np.iinfo(np.int32).min).any() and want_gid.max() == 4
    for r, w in enumerate(want):
        got = t.cell_gene(r)
        assert got.keys() == w.keys() and got["cnv_regions"] == w["cnv_regions"] == t.name(r) and got["State"] == w["State"]
        assert np.array_equal(got["Genes"], w["Genes"]) and got["Genes"].dtype == w["Genes"].dtype
        assert np.array_equal(got["Cells"], w["Cells"]) and got["Cells"].dtype == w["Cells"].dtype
        assert int(t.token[r]) == br.fnv1a64(w["cnv_regions"])
        assert np.array_equal(np.arange(t.row_first[r], t.row_first[r] + t.gene_count[r]), w["Genes"])
    # take(): the kept regions with new states, the table it came from remembered
    keep = np.array([True, False, True, True, False, True, False, True])
    state = np.arange(8) + 1
    sub = t.take(keep, state)
    assert len(sub) == 5 and sub.source is t and sub.take(np.array([0, 4])).source is t
    for j, r in enumerate(np.nonzero(keep)[0]):
        got = sub.cell_gene(j)
        assert got["cnv_regions"] == want[r]["cnv_regions"] and got["State"] == state[r] and sub.token[j] == t.token[r]
        assert np.array_equal(got["Genes"], want[r]["Genes"]) and np.array_equal(got["Cells"], want[r]["Cells"])
    # a run that the gather tears apart is refused, as the dict route's _gene_run refuses it
    torn = rec.copy()
    torn[2, 2], torn[3, 2] = 9, 10
    with pytest.raises(ValueError, match="contiguous"):
        bayes_net.RegionTable.from_records(groups, chr_names, perm, torn)


def test_lazy_sequences():
    from infercnv_amd import bayes_net
    groups, chr_names, perm, rec = mock_records()
    obj = bayes_net.MCMCInferCNV(infercnv_obj=None)
    bayes_net._attach_table(obj, bayes_net.RegionTable.from_records(groups, chr_names, perm, rec))
    names = [f"{chr_names[c]}-region_{o}" for c, o in zip(rec[1], rec[5])]
    assert len(obj.cnv_regions) == 8 and list(obj.cnv_regions) == names
    assert obj.cnv_regions[0] == names[0] and obj.cnv_regions[-1] == names[-1] and obj.cnv_regions[np.int64(3)] == names[3]
    assert obj.cnv_regions[2:7:2] == names[2:7:2] and obj.cnv_regions[::-1] == names[::-1] and obj.cnv_regions[8:] == []
    assert [cg["cnv_regions"] for cg in obj.cell_gene] == names and len(obj.cell_gene[1:3]) == 2
    for bad in (8, -9):
        with pytest.raises(IndexError):
            obj.cell_gene[bad]
    with pytest.raises(TypeError):
        obj.cnv_regions[0] = "x"                                                    # read-only
    calls = []
    seq = bayes_net._LazySeq(3, lambda i: calls.append(i) or i * i)
    assert calls == [] and seq[2] == 4 and calls == [2]                             # an element is built when it is asked for


def test_remove_cnv_keeps_the_same_regions_as_before(tmp_path):
    """The boolean mask that replaced the O(n^2) comprehension of _remove_cnv: the same kept list."""
    from infercnv_amd import bayes_net
    rng = np.random.default_rng(0)
    n = 300
    means = rng.dirichlet(np.ones(6), size=n).T
    means[:, 5] = np.nan
    obj = bayes_net.MCMCInferCNV(infercnv_obj=None)
    obj.cnv_regions = [f"chr1-region_{i}" for i in range(n)]
    obj.cell_gene = [{"cnv_regions": nm, "Genes": np.array([i]), "Cells": np.array([0]), "State": 4} for i, nm in enumerate(obj.cnv_regions)]
    obj.cnv_means, obj.cell_probabilities, obj.cnv_probabilities = means, [None] * n, [None] * n
    obj.args = {"HMM_type": "i6", "postMcmcMethod": "removeCNV", "reassignCNVs": False, "out_dir": None}
    f, st = bayes_net.filterHighPNormals(obj, np.full((n, 1), 4, dtype=np.int8), 0.2)
    remove = set(np.nonzero(means[2] > 0.2)[0].tolist())
    keep = [i for i in range(n) if i not in remove]
    assert 0 < len(keep) < n and 5 in keep
    assert f.cnv_regions == [obj.cnv_regions[i] for i in keep] and np.array_equal(f.cnv_means, means[:, keep], equal_nan=True)
    assert np.array_equal(st[:, 0], np.where(np.isin(np.arange(n), keep), 4, 3))
