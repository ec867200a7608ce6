"""Sequential restatement of the K33 contracts of include/icnv.h (icnv_paint_regions_dev, icnv_theta_box_dev, DESIGN K33),
written from the header alone: the paint as naive loops with the regions in order, the box statistics per series in Python
floats (one IEEE rounding per operation) on the quantile of tests/mcmc_diag_restate.py, and the two tables of
bayes_net.plotProbabilities.  The GPU and the host program of infercnv_amd/csrc/bayes_probs_host_check.cpp are held to it bit
for bit.  The box contract is the library's own, modelled on ggplot2's stat_boxplot: believed, not verified against ggplot2."""
import numpy as np

import mcmc_diag_restate as mr

BOX_FIELDS = ("ymin", "lower", "middle", "upper", "ymax", "n_low", "n_high")
MIN_CHAINS, MAX_CHAINS, MAX_POOLED = 2, 8, 8192
NAN = float("nan")


# ---- the paint ----------------------------------------------------------------------------------------------------------
def paint_refusal(G, C, gene_first, gene_count, cell_off, cell_idx):
    """None, or "ARG": what the device-side check answers before a byte is written."""
    off = [int(v) for v in cell_off]
    n = len(gene_first)
    if len(off) != n + 1 or off[0] != 0 or off[-1] < 0 or off[-1] > len(cell_idx):
        return "ARG"
    for r in range(n):
        if off[r + 1] < off[r] or gene_first[r] < 0 or gene_count[r] < 0 or gene_first[r] + gene_count[r] > G:
            return "ARG"
    for c in cell_idx[:off[-1]]:
        if c < 0 or c >= C:
            return "ARG"
    return None


def paint(G, C, gene_first, gene_count, cell_off, cell_idx, value):
    """The (C, G) matrix: +0.0, then region after region in order, element by element (the last writer stays)."""
    out = np.zeros((C, G), dtype=np.float64)
    value = np.asarray(value, dtype=np.float64)
    for r in range(len(gene_first)):
        for i in range(int(cell_off[r]), int(cell_off[r + 1])):
            c = int(cell_idx[i])
            for g in range(int(gene_first[r]), int(gene_first[r]) + int(gene_count[r])):
                out[c, g] = value[r]
    return out


def paint_cell_gene(G, C, cell_gene, value):
    """The same from a list of {"Genes", "Cells"} with arbitrary index vectors (R's expr.data[Genes, Cells] <- v), as the
    genes x cells matrix R holds."""
    out = np.zeros((G, C), dtype=np.float64)
    for cg, v in zip(cell_gene, value):
        for g in cg["Genes"]:
            for c in cg["Cells"]:
                out[int(g), int(c)] = v
    return out


# ---- the box statistics -------------------------------------------------------------------------------------------------
def box_refusal(n_regions, n_chains, n_keep, K):
    if n_regions < 0 or n_keep < 1 or not (MIN_CHAINS <= K <= MAX_CHAINS) or not (MIN_CHAINS <= n_chains <= MAX_CHAINS):
        return "ARG"
    if n_chains * n_keep > MAX_POOLED or n_regions * K > 2 ** 31 - 1:
        return "UNSUPPORTED"
    return None


def box_stats(y):
    """The seven fields of the pooled draws y (any shape)."""
    flat = np.asarray(y, dtype=np.float64).ravel()
    if np.isnan(flat).any():
        return [NAN] * 7
    srt = [float(v) for v in np.sort(flat + 0.0)]                # -0.0 + 0.0 is +0.0
    lower, middle, upper = (mr.quantile7(srt, p) for p in (0.25, 0.5, 0.75))
    iqr = upper - lower
    reach = 1.5 * iqr
    lo, hi = lower - reach, upper + reach
    n_low = sum(1 for v in srt if v < lo)
    n_high = sum(1 for v in srt if v > hi)
    inside = [v for v in srt if not v < lo and not v > hi]
    if n_low + n_high >= len(srt):
        inside = [NAN]
    return [inside[0], lower, middle, upper, inside[-1], float(n_low), float(n_high)]


def fences(y):
    """(lo, hi) of box_stats, for the tests that plant a draw on one."""
    srt = [float(v) for v in np.sort(np.asarray(y, dtype=np.float64).ravel() + 0.0)]
    lower, upper = mr.quantile7(srt, 0.25), mr.quantile7(srt, 0.75)
    reach = 1.5 * (upper - lower)
    return lower - reach, upper + reach


def theta_box(samples):
    """samples: (n_regions, n_chains, n_keep, K) -> (n_regions, K, 7)."""
    s = np.asarray(samples, dtype=np.float64)
    R, m, n, K = s.shape
    out = np.empty((R, K, 7))
    for r in range(R):
        for k in range(K):
            out[r, k] = box_stats(s[r, :, :, k])
    return out


# ---- the two tables -----------------------------------------------------------------------------------------------------
def cnv_table(names, box):
    """(row names, matrix) of cnvProbs.<p>.dat: one row <region>:State:<k> per (region, state)."""
    box = np.asarray(box, dtype=np.float64)
    R, K = box.shape[:2]
    return [f"{names[r]}:State:{k + 1}" for r in range(R) for k in range(K)], box.reshape(R * K, 7)


def cell_table(names, cells_of, cell_probabilities, cell_names):
    """(row names, matrix, column names) of cellProbs.<p>.dat: one row <region>:<cell name> per (region, cell) in the region's
    cell order, the K state probabilities of cell_probabilities[r][:, i] across."""
    rows, mat = [], []
    for r, name in enumerate(names):
        cp = np.asarray(cell_probabilities[r], dtype=np.float64)
        for i, c in enumerate(cells_of[r]):
            rows.append(f"{name}:{cell_names[int(c)]}")
            mat.append(cp[:, i])
    K = np.asarray(cell_probabilities[0]).shape[0] if len(names) else 0
    return rows, (np.array(mat) if mat else np.zeros((0, K))), [f"State:{k + 1}" for k in range(K)]


def file_names(threshold):
    """R's sprintf("cnvProbs.%s.pdf", BayesMaxPNormal) with the tables' extension; None: unset."""
    if threshold is None:
        return "cnvProbs.dat", "cellProbs.dat"
    p = ("%.15g" % threshold) if isinstance(threshold, float) else str(threshold)
    return f"cnvProbs.{p}.dat", f"cellProbs.{p}.dat"


# ---- seeded inputs shared by the tests, the corpus of the host program and the benchmark ----------------------------------
def _plant(view, lowest, highest):
    """Replace the smallest draws of the (chains, n) view by `lowest` and the largest by `highest`, in place."""
    order = np.argsort(view, axis=None, kind="stable")
    for i, v in enumerate(lowest):
        view[np.unravel_index(order[i], view.shape)] = v
    for i, v in enumerate(highest):
        view[np.unravel_index(order[-1 - i], view.shape)] = v


def make_box_samples(R, m, n, K, seed):
    """(R, m, n, K) theta-like samples (mcmc_diag_restate.make_samples) with the cases of the box contract planted where the
    shape has room for them (m n >= 16): region 0, state 0: its extreme draws moved ON the two fences (strict comparisons: they are
    whisker ends, not outliers); region 0, state 1: two draws below the lower fence and one above the upper; region 1: state 0 constant, state 1 a
    handful of tied values with both zeros; region 2: no cells (NaN)."""
    s = mr.make_samples(R, m, n, K, seed).copy()
    if m * n >= 16:
        for k, (below, above) in enumerate((((0.0,), (0.0,)), ((0.25, 0.5), (0.125,)))):
            view = s[0, :, :, k]
            lo, hi = fences(view)
            _plant(view, [lo - d for d in below], [hi + d for d in above])
            assert fences(view) == (lo, hi)                       # the planted draws sit outside the quartiles' reach
        if R > 1:
            s[1, :, :, 0] = 0.25
            s[1, :, :, 1] = np.random.default_rng(seed + 1).choice(np.array([-0.0, 0.0, 0.5, 0.5, 1.0, -1.0]), size=(m, n))
    if R > 2:
        s[2] = np.nan
    return s
