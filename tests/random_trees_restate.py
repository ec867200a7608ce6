"""NumPy restatement of the random-trees statistic of include/icnv.h (icnv_random_trees_dev, DESIGN K10): the permuted,
smoothed and median-centred matrices of a clade and their trees.

  - permutation of gene g in iteration r of a clade: NumPy's own Generator(Philox(key=[seed, token],
    counter=[0, g, r, 0])).permutation(n); Y[g, c] = x[g, S[pi_g(c)]].
  - runmean(k = window, endrule = "mean"): k = min(window, G), k2 = k // 2; output o is the sequential sum (gene order, one
    rounding per add) of x over [max(0, o - (k - 1 - k2)), min(G - 1, o + k2)], then one division by the window's length.
  - centring: oracle_np.center_columns(, "median").
  - trees: tests/hclust_restate.py on the sequential distances.
The recursion is the product's own driver (tumor_subclusters.random_trees_partition)."""
import numpy as np

import hclust_restate as hr
import oracle_np as onp
from infercnv_amd import tumor_subclusters as ts


def permutation(seed, token, g, r, n):
    bg = np.random.Philox(key=np.array([seed, token], dtype=np.uint64), counter=np.array([0, g, r, 0], dtype=np.uint64))
    return np.random.Generator(bg).permutation(n)


def runmean(X, window):
    """caTools::runmean(k = window, endrule = "mean") down the rows (genes) of every column of X (G x n)."""
    X = np.asarray(X, dtype=np.float64)
    G = X.shape[0]
    k = min(int(window), G)
    if k <= 1:
        return X.copy()
    k2 = k // 2
    o = np.arange(G)
    lo = np.maximum(0, o - (k - 1 - k2))
    hi = np.minimum(G - 1, o + k2)
    S = np.zeros_like(X)
    for j in range(int((hi - lo).max()) + 1):
        q = lo + j
        m = q <= hi
        S[m] = S[m] + X[q[m]]
    return S / (hi - lo + 1).astype(np.float64)[:, None]


def clade_matrix(x, cells, window, seed, token, iteration, permute=True, smooth=True, center=True):
    """The (G x n) matrix of one clade and iteration (-1: observed) after the chosen stages."""
    Y = np.asarray(x, dtype=np.float64)[:, np.asarray(cells)].copy()
    n = Y.shape[1]
    if permute and iteration >= 0:
        for g in range(Y.shape[0]):
            Y[g] = Y[g, permutation(seed, token, g, iteration, n)]
    if smooth:
        Y = runmean(Y, window)
    if center:
        Y = onp.center_columns(Y, "median")
    return Y


def tree(Z, method):
    return hr.hclust(hr.seq_dist(np.asarray(Z).T), method)


def clade_stat(x, cells, window, seed, token, n_iter, method):
    """(observed tree, max heights of the n_iter permuted trees) of one clade."""
    obs = tree(clade_matrix(x, cells, window, seed, token, -1), method)
    rand = np.array([tree(clade_matrix(x, cells, window, seed, token, r), method)[1].max() for r in range(n_iter)])
    return obs, rand


def clade_fn(x, window, seed, n_iter, method):
    """The driver's per-level callable on the restatement (tokens: FNV-1a-64 of the clade names, as the product's)."""
    def fn(clades):
        return [clade_stat(x, cells, window, seed, ts.fnv1a64(name), n_iter, method) for name, cells in clades]
    return fn


def partition(x, groups, p_val, method="ward.D2", window=101, max_recursion_depth=3, min_cluster_size_recurse=10, seed=0,
              n_iter=ts.RANDOM_TREES_ITERATIONS):
    """random_trees_partition on the restatement: (hc, subclusters) for the groups of the (already subtracted) G x C x."""
    return ts.random_trees_partition(groups, clade_fn(x, window, seed, n_iter, method), p_val, max_recursion_depth,
                                     min_cluster_size_recurse)


def planted_clones(n_per=30, G=300, seed=7, homogeneous=False):
    """A G x 2 n_per matrix (already reference-subtracted) with two clones: clone A gains genes 0-99 (one chromosome),
    clone B loses genes 150-249 (another); noise sd 0.3.  Returns (x, clone labels)."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 0.3, size=(G, 2 * n_per))
    clone = np.repeat([0, 1], n_per)
    rng.shuffle(clone)
    if not homogeneous:
        x[:100, clone == 0] += 0.6
        x[150:250, clone == 1] -= 0.6
    return x, clone
