"""The random-trees subclustering's driver and restatement (DESIGN K10), on the host: runmean's window rule, R's p-value
arithmetic, cutree numbering, naming and recursion limits, the .hspike argument slip, and the planted-clone end to end
(R/inferCNV_tumor_subclusters.random_smoothed_trees.R)."""
import numpy as np
import pytest

import random_trees_restate as rr
from infercnv_amd import tumor_subclusters as ts
from infercnv_amd.infercnv_object import GeneOrder, InfercnvObject


# ------------------------------------------------------------------ runmean
def direct_runmean(X, window):
    G = X.shape[0]
    k = min(window, G)
    out = np.empty_like(X)
    for c in range(X.shape[1]):
        for o in range(G):
            lo, hi = max(0, o - (k - 1 - k // 2)), min(G - 1, o + k // 2)
            s = 0.0
            for q in range(lo, hi + 1):
                s = s + X[q, c]
            out[o, c] = s / (hi - lo + 1) if k > 1 else X[o, c]
    return out


@pytest.mark.parametrize("G", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("window", [1, 2, 3, 4, 5, 7])
def test_runmean_clipped_window(G, window):
    X = np.random.default_rng(G * 10 + window).standard_normal((G, 3))
    got = rr.runmean(X, window)
    assert np.array_equal(got, direct_runmean(X, window))
    k = min(window, G)
    if k > 1:   # the plain mean of the clipped window (caTools' endrule = "mean")
        for o in range(G):
            lo, hi = max(0, o - (k - 1 - k // 2)), min(G - 1, o + k // 2)
            np.testing.assert_allclose(got[o], X[lo:hi + 1].mean(axis=0), rtol=1e-15, atol=1e-15)


def test_runmean_even_window_bias():
    X = np.arange(6, dtype=np.float64)[:, None]
    # k = 4, k2 = 2: output o averages [o - 1, o + 2]
    assert rr.runmean(X, 4)[:, 0].tolist() == [1.0, 1.5, 2.5, 3.5, 4.0, 4.5]


# ------------------------------------------------------------------ p-value
def test_pvalue_arithmetic():
    rand = np.arange(100, dtype=np.float64)
    assert ts.random_trees_pvalue(94.0, rand) == 1 - 95 / 100 == 0.050000000000000044
    assert not ts.random_trees_pvalue(94.0, rand) <= 0.05          # 95 of 100: no split at 0.05
    assert ts.random_trees_pvalue(89.0, rand) <= 0.1                # 90 of 100: split at 0.1
    assert ts.random_trees_pvalue(0.0, np.full(100, -1.0)) == 1.0   # a flat tree never splits
    assert ts.random_trees_pvalue(1e9, rand) == 0.0
    assert ts.random_trees_pvalue(-0.5, rand) == 1.0


# ------------------------------------------------------------------ cutree
def test_cutree_first_appearance_numbering():
    # ((3, 4), (1, (0, 2))): cells 1, 0, 2 together, 3, 4 together
    merge = np.array([[-1, -3], [-4, -5], [-2, 1], [2, 3]], dtype=np.int32)
    height = np.array([1.0, 2.0, 3.0, 10.0])
    assert ts.cutree_h(merge, height, 6.5).tolist() == [1, 1, 1, 2, 2]
    assert ts.cutree_h(merge, height, 2.5).tolist() == [1, 2, 1, 3, 3]
    assert ts.cutree_h(merge, height, 0.5).tolist() == [1, 2, 3, 4, 5]
    assert ts.cutree_h(merge, height, 10.0).tolist() == [1, 1, 1, 1, 1]


def fake_fn(trees, calls):
    """A scripted clade_fn: trees[name] = (merge, height, order, p) with p the fraction of random heights below the max."""
    def fn(clades):
        calls.append([(name, cells.tolist()) for name, cells in clades])
        out = []
        for name, cells in clades:
            merge, height, p = trees[name]
            mh = float(np.max(height))
            rand = np.where(np.arange(100) < round(p * 100), mh - 1.0, mh + 1.0)
            out.append(((np.asarray(merge), np.asarray(height, dtype=np.float64), None), rand))
        return out
    return fn


def chain_tree(n, heights):
    """A caterpillar tree over n cells: cell 0 with 1, then each next cell joins; the given n-1 heights."""
    merge = [[-1, -2]] + [[-(i + 1), i - 1] for i in range(2, n)]
    return np.array(merge, dtype=np.int32), np.asarray(heights, dtype=np.float64)


def test_top_two_tie_recurses_into_same_cells():
    m, h = chain_tree(4, [1.0, 5.0, 5.0])
    calls = []
    trees = {"g.1": (m, h, 1.0), "g.1.1": (m, h, 0.0)}
    hc, sub = ts.random_trees_partition({"g": np.array([7, 8, 9, 10])}, fake_fn(trees, calls), 0.05, 3, 2)
    assert calls[1] == [("g.1.1", [7, 8, 9, 10])]   # one group: the same cells, one level down
    assert list(sub["g"]) == ["g.1.1"]


def test_naming_sorted_split_and_depth_limit():
    # 12 cells: level 1 splits into {0..5}, {6..11}; level 2 splits the first again; depth 2 stops the recursion
    merge = []
    for a in range(0, 12, 2):
        merge.append([-(a + 1), -(a + 2)])                              # rows 1..6: pairs
    merge += [[1, 2], [7, 3], [4, 5], [9, 6], [8, 10]]                   # rows 7..11
    h = np.array([1, 1, 1, 1, 1, 1, 2, 3, 2, 3, 20], dtype=np.float64)
    m6, h6 = chain_tree(6, [1.0, 2.0, 3.0, 9.0, 10.0])
    trees = {"t.1": (np.array(merge), h, 1.0), "t.1.1": (m6, h6, 1.0), "t.1.2": (m6, h6, 0.0)}
    calls = []
    cells = np.arange(100, 112)
    hc, sub = ts.random_trees_partition({"t": cells}, fake_fn(trees, calls), 0.05, max_recursion_depth=2,
                                        min_cluster_size_recurse=3)
    assert len(calls) == 2 and [c[0] for c in calls[1]] == ["t.1.1", "t.1.2"]
    # t.1.1 splits at mean(10, 9): {0..4} and {5} -> t.1.1.1 and t.1.1.2; depth 3 is not evaluated
    assert list(sub["t"]) == ["t.1.1.1", "t.1.1.2", "t.1.2"]
    assert sub["t"]["t.1.1.1"].tolist() == [100, 101, 102, 103, 104]
    assert sub["t"]["t.1.2"].tolist() == list(range(106, 112))
    assert hc["t"][0] is trees["t.1"][0]


def test_all_groups_too_small_keeps_name():
    m, h = chain_tree(4, [1.0, 2.0, 9.0])
    calls = []
    hc, sub = ts.random_trees_partition({"a": np.array([3, 1, 2, 0])}, fake_fn({"a.1": (m, h, 1.0)}, calls), 0.05, 3, 10)
    assert list(sub["a"]) == ["a.1"] and sub["a"]["a.1"].tolist() == [3, 1, 2, 0]
    assert len(calls) == 1


def test_single_cell_group_raises():
    with pytest.raises(ValueError):
        ts.random_trees_partition({"a": np.array([4])}, lambda c: [], 0.05)


def test_hspike_argument_slip(monkeypatch):
    from infercnv_amd import ops
    calls = []
    orig = ts.define_signif_tumor_subclusters_via_random_smooothed_trees

    def spy(obj, *args, **kw):
        calls.append((args, kw))
        return orig(obj, *args, **kw) if len(calls) == 1 else "mirrored"

    monkeypatch.setattr(ts, "define_signif_tumor_subclusters_via_random_smooothed_trees", spy)
    monkeypatch.setattr(ops, "subtract_ref_expr_from_obs", lambda obj, inv_log=False: obj)
    monkeypatch.setattr(ts, "random_trees_partition", lambda *a, **k: ({}, {}))
    x = np.zeros((5, 4))
    hs = InfercnvObject(x, GeneOrder(np.array(["1"] * 5)), observation_grouped_cell_indices={"o": np.arange(4)})
    obj = InfercnvObject(x, GeneOrder(np.array(["1"] * 5)), observation_grouped_cell_indices={"o": np.arange(4)}, hspike=hs)
    out = ts.define_signif_tumor_subclusters_via_random_smooothed_trees(obj, 0.05, "ward.D2", False, 51, 2, 7, seed=5)
    assert out.hspike == "mirrored" and out.expr_data is obj.expr_data
    # the reference's call: (hspike, p_val, hclust_method, window_size, max_recursion_depth, min_cluster_size_recurse)
    assert calls[1] == ((0.05, "ward.D2", 51, 2, 7), {"seed": 6})


def test_fnv1a64():
    assert ts.fnv1a64("") == 0xCBF29CE484222325
    assert ts.fnv1a64("a") == 0xAF63DC4C8601EC8C


# ------------------------------------------------------------------ end to end on the restatement
def test_planted_clones_split():
    x, clone = rr.planted_clones()
    hc, sub = rr.partition(x, {"tumor": np.arange(x.shape[1])}, 0.05, max_recursion_depth=1)
    assert list(sub["tumor"]) == ["tumor.1.1", "tumor.1.2"]
    got = [set(v.tolist()) for v in sub["tumor"].values()]
    want = [set(np.flatnonzero(clone == c).tolist()) for c in (0, 1)]
    assert sorted(map(sorted, got)) == sorted(map(sorted, want))
    merge, height, order = hc["tumor"]
    assert merge.shape == (x.shape[1] - 1, 2) and np.all(np.diff(height) >= 0)


def test_homogeneous_does_not_split():
    x, _ = rr.planted_clones(homogeneous=True)
    _, sub = rr.partition(x, {"tumor": np.arange(x.shape[1])}, 0.05, max_recursion_depth=1)
    assert list(sub["tumor"]) == ["tumor.1"]
