"""The hclust restatement (tests/hclust_restate.py) that the GPU tests hold icnv_hclust_dev to (DESIGN K9), checked on the
host: against the reference's own stored hclust objects, against SciPy, and its R-format conversion."""
import os

import numpy as np
import pytest

import hclust_restate as hr
import oracle_np as onp


@pytest.fixture(scope="module")
def golden(golden_dir):
    d = np.load(os.path.join(golden_dir, "infercnv_object_example.npz"))
    g = np.load(os.path.join(golden_dir, "hclust_example.npz"))
    log = onp.log2xplus1(onp.normalize_counts_by_seq_depth(d["count_data"]))
    pre = onp.run_chain(log, d["chr_codes"], [d["ref_normal"]], denoise=False)      # step 14, before step 22
    return pre, {"tumor": d["obs_tumor"], "normal": d["ref_normal"]}, g


@pytest.mark.parametrize("grp", ["tumor", "normal"])
def test_restatement_reproduces_reference_hclust(golden, grp):
    """@tumor_subclusters$hc$<grp> of data/infercnv_object_example.rda: hclust(dist(t(x)), "ward.D2") of the step-14
    matrix restricted to the group's cells."""
    pre, groups, g = golden
    assert str(g[f"{grp}_method"]) == "ward.D2" and str(g[f"{grp}_dist_method"]) == "euclidean"
    merge, height, order = hr.hclust(hr.seq_dist(pre[:, groups[grp]].T), "ward.D2")
    assert np.array_equal(merge, g[f"{grp}_merge"])
    assert np.array_equal(order, g[f"{grp}_order"])
    assert np.max(np.abs(height - g[f"{grp}_height"]) / g[f"{grp}_height"]) <= 1e-14


def scipy_r_merge(Z, n):
    """SciPy's linkage matrix in R's labelling: ids < n are singletons -(id+1), the others the 1-based step; per row the
    smaller id first (a singleton before a cluster, singletons by index, clusters by creation)."""
    ab = np.sort(Z[:, :2].astype(np.int64), axis=1)
    return np.where(ab < n, -(ab + 1), ab - n + 1).astype(np.int32)


@pytest.mark.parametrize("method,scipy_method", [("single", "single"), ("complete", "complete"), ("average", "average"),
                                                 ("mcquitty", "weighted"), ("ward.D2", "ward")])
def test_restatement_matches_scipy_on_tie_free_data(method, scipy_method):
    from scipy.cluster.hierarchy import linkage
    from scipy.spatial.distance import pdist, squareform
    rng = np.random.default_rng(11)
    X = rng.standard_normal((150, 9))
    d = pdist(X)
    merge, height, order = hr.hclust(squareform(d), method)
    Z = linkage(d, scipy_method)
    assert np.array_equal(merge, scipy_r_merge(Z, 150))
    np.testing.assert_allclose(height, Z[:, 2], rtol=1e-12, atol=0)
    assert sorted(order.tolist()) == list(range(1, 151))


def test_r_format_two_objects():
    merge, height, order = hr.r_format(2, np.array([0]), np.array([1]), np.array([4.0]), sqrt_heights=True)
    assert merge.tolist() == [[-1, -2]]
    assert height.tolist() == [2.0]
    assert order.tolist() == [1, 2]


def test_r_format_chained_merges():
    # each merge takes the previous cluster (which lives on at the larger index): a singleton comes first in R's rows
    merge, height, order = hr.r_format(4, np.array([0, 1, 2]), np.array([1, 2, 3]), np.array([1.0, 2.0, 3.0]))
    assert merge.tolist() == [[-1, -2], [-3, 1], [-4, 2]]
    assert order.tolist() == [4, 3, 1, 2]
    assert height.tolist() == [1.0, 2.0, 3.0]


def test_r_format_sorts_chain_order_by_height_and_labels_clusters_by_creation():
    # chain order (2,3) @1.0, (0,1) @0.5, (1,3) @2.0 -> sorted: (0,1), (2,3), then the two clusters
    merge, height, order = hr.r_format(4, np.array([2, 0, 1]), np.array([3, 1, 3]), np.array([1.0, 0.5, 2.0]))
    assert merge.tolist() == [[-1, -2], [-3, -4], [1, 2]]
    assert height.tolist() == [0.5, 1.0, 2.0]
    assert order.tolist() == [1, 2, 3, 4]


def test_restatement_rejects_what_the_library_rejects():
    with pytest.raises(ValueError):
        hr.hclust(np.zeros((1, 1)), "ward.D2")
    for m in ("centroid", "median"):
        with pytest.raises(ValueError):
            hr.hclust(np.zeros((3, 3)), m)


def assert_valid_r_dendrogram(merge, height, order, n):
    assert merge.shape == (n - 1, 2) and height.shape == (n - 1,) and order.shape == (n,)
    assert np.all(np.diff(height) >= 0)
    assert sorted(order.tolist()) == list(range(1, n + 1))
    assert sorted((-merge[merge < 0]).tolist()) == list(range(1, n + 1))
    for i, row in enumerate(merge):
        assert np.all(row[row > 0] <= i)   # a cluster is used only after the step that made it
        if row[0] < 0 and row[1] < 0:
            assert row[0] > row[1]          # two singletons: the smaller index first
        elif row[0] > 0 and row[1] > 0:
            assert row[0] < row[1]          # two clusters: the older first
        else:
            assert row[0] < 0               # a singleton before a cluster


@pytest.mark.parametrize("method", ["ward.D2", "ward.D", "single", "complete", "average", "mcquitty"])
def test_restatement_on_duplicated_rows(method):
    """The GPU's distances are held to seq_dist; on duplicated rows seq_dist is exactly 0 and the restatement merges
    them at height exactly 0, ties by index, as R does."""
    rng = np.random.default_rng(2)
    X = rng.normal(1.0, 0.3, size=(30, 500))
    X[7] = X[2]
    X[20] = X[11] = X[4]
    d = hr.seq_dist(X)
    assert d[2, 7] == 0.0 and d[4, 11] == 0.0 and d[4, 20] == 0.0 and d[11, 20] == 0.0
    assert np.count_nonzero(d == 0.0) == 30 + 2 * 4
    merge, height, order = hr.hclust(d, method)
    assert_valid_r_dendrogram(merge, height, order, 30)
    assert height[:3].tolist() == [0.0, 0.0, 0.0] and height[3] > 0
    # the three zero-height merges are R's: singletons by index, then the triple's third member joins its cluster
    assert merge[:3].tolist() == [[-3, -8], [-5, -12], [-21, 2]]
    # n copies of one row: every height 0, merged by index
    n = 9
    merge, height, order = hr.hclust(hr.seq_dist(np.repeat(X[:1], n, axis=0)), method)
    assert_valid_r_dendrogram(merge, height, order, n)
    assert np.all(height == 0.0)
    assert merge.tolist() == [[-1, -2]] + [[-(i + 2), i] for i in range(1, n - 1)]
    assert order.tolist() == list(range(n, 2, -1)) + [1, 2]
