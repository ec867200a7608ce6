"""The non-DE masking kernels (DESIGN K12: de_kernels.hip, de_api.hip) at the shapes where their code takes another path: an
odd number of HBM merge passes (the second key buffer is the result) in the rank sum and in BH, jitter and merged segments in
a later wave, the grid-stride loops of the mask and the mean beyond 65535 cells, every regime of pnorm2 / pt2 and the ends
of the exact table, padded leading dimensions, in-place masking, the mean's non-finite fallback and the group bookkeeping.
Every result bit-equal (NaN = NaN) to tests/de_restate.py, as in tests/test_gpu_de.py; the CPU-side assertions say that the
inputs reach the path they were built for."""
import math

import numpy as np
import pytest

import de_edge_cases as ec
import de_restate as dr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infercnv_amd import device
    torch.cuda.set_device(0)
    device.init(0)
    return device


def same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    both_nan = np.isnan(a) & np.isnan(b)
    bad = ~both_nan & (a.view(np.uint64) != b.view(np.uint64))
    assert not bad.any(), f"{int(bad.sum())} differ, first at {np.argwhere(bad)[0]}: {a[bad][0]!r} vs {b[bad][0]!r}"


def on_dev(expr):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(expr, dtype=np.float64).T)).cuda()


def padded(expr, pad, fill=np.nan):
    """The (C, G) view of a (C, G + pad) device tensor whose padding columns hold `fill`."""
    x = on_dev(expr)
    wide = torch.full((x.shape[0], x.shape[1] + pad), fill, dtype=torch.float64, device="cuda")
    wide[:, :x.shape[1]] = x
    return wide, wide[:, :x.shape[1]]


def run_tests(dev, x, groups, cmps, test, jitter, seed=0):
    return tuple(t.cpu().numpy() for t in dev.de_tests(x, groups, cmps, test=test, jitter=jitter, seed=seed))


def restated(expr, groups, cmps, test="wilcoxon", jitter=True, seed=0, whole_matrix=False):
    """dr.de_tests; whole_matrix: the jitter of every (gene, cell) is added up front from ec.jitter_matrix -- a sample of it
    held to dr.jitter bit for bit -- because one Philox generator per value costs seconds at these sizes."""
    if whole_matrix and jitter and test == "wilcoxon":
        J = ec.jitter_matrix(seed, *expr.shape)
        assert ec.jitter_sample_matches(J, seed)
        return dr.de_tests(expr + J, groups, cmps, test=test, jitter_on=False)
    return dr.de_tests(expr, groups, cmps, test=test, jitter_on=jitter, seed=seed)


def check_tests(dev, expr, groups, cmps, test, jitter, seed=0, whole_matrix=False):
    got = run_tests(dev, on_dev(expr), groups, cmps, test, jitter, seed)
    ref = restated(expr, groups, cmps, test, jitter, seed, whole_matrix)
    for a, b in zip(got, ref):
        same(a, b)
    return got


def passes(n):
    """HBM merge passes of an n-key segment: runs of DE_CHUNK = 4096 doubled until one run holds it."""
    k, run = 0, 4096
    while run < n:
        run *= 2
        k += 1
    return k


# ---------------------------------------------------------------- 1. merge passes and buffers
MERGE_SIZES = [4096, 4097, 8192, 8193, 16385, 30]
# pairs that end in different buffers, in both orientations; the last two have both samples in the second buffer
MERGE_CMPS = [(5, 0), (1, 5), (2, 3), (4, 5), (3, 1), (0, 4), (2, 4), (4, 1)]


def build_merge_case():
    assert [passes(n) for n in MERGE_SIZES] == [0, 1, 1, 2, 3, 0]
    assert {(passes(MERGE_SIZES[a]) & 1, passes(MERGE_SIZES[b]) & 1) for a, b in MERGE_CMPS} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    groups, C = ec.sized_groups(MERGE_SIZES)
    expr = np.round(np.random.default_rng(21).normal(0.0, 1.0, size=(2, C)), 2)       # ties
    return expr, groups


@pytest.fixture(scope="module")
def merge_case():
    return build_merge_case()


def test_merge_pass_parity_wilcoxon(dev, merge_case):
    expr, groups = merge_case
    dev.de_stats(reset=True)
    check_tests(dev, expr, groups, MERGE_CMPS, "wilcoxon", False)
    st = dev.de_stats()
    assert st["segments_hbm"] == 4 * expr.shape[0] and st["segments_lds"] == 2 * expr.shape[0] and st["waves"] == 1


def test_merge_pass_parity_wilcoxon_jitter(dev, merge_case):
    expr, groups = merge_case
    dev.de_stats(reset=True)
    check_tests(dev, expr[1:], groups, MERGE_CMPS, "wilcoxon", True, seed=9, whole_matrix=True)
    assert dev.de_stats()["segments_hbm"] == 4


def test_long_groups_welch(dev, merge_case):
    expr, groups = merge_case
    check_tests(dev, expr, groups, MERGE_CMPS, "t", False)


@pytest.mark.parametrize("jitter", [False, True])
def test_short_finite_prefix_of_a_merged_segment(dev, jitter):
    # 5000 cells of which 10 (gene 0) or 50 (gene 1) are finite, against 12 cells: the exact table and the first size of the
    # normal branch, both reached from the finite prefix of an HBM-merged segment
    groups, C = ec.sized_groups([5000, 12])
    rng = np.random.default_rng(23)
    expr = rng.permutation(2 * C).reshape(2, C).astype(np.float64) * 0.125
    for g, keep in ((0, 10), (1, 50)):
        drop = rng.permutation(5000)[keep:]
        expr[g, drop] = rng.choice([np.nan, np.inf, -np.inf], size=drop.size)
        d = expr[g, drop]
        assert int(np.isfinite(expr[g, :5000]).sum()) == keep and np.isnan(d).any() and (d == np.inf).any() and (d == -np.inf).any()
    cmps = [(0, 1), (1, 0)]
    if not jitter:
        assert ec.wilcox_z(expr[0, groups[0]].tolist(), expr[0, groups[1]].tolist()) is None          # exact table
        assert ec.wilcox_z(expr[1, groups[0]].tolist(), expr[1, groups[1]].tolist()) is not None      # 50: normal
    dev.de_stats(reset=True)
    check_tests(dev, expr, groups, cmps, "wilcoxon", jitter, seed=4)
    assert dev.de_stats()["segments_hbm"] == 2


# ---------------------------------------------------------------- 2. BH through the merge path
@pytest.mark.parametrize("G", [4097, 8192, 8193])
def test_bh_rows_beyond_one_chunk(dev, G):
    groups, C = ec.sized_groups([3, 4, 60])
    rng = np.random.default_rng(G)
    expr = rng.integers(0, 4, size=(G, C)).astype(np.float64)
    const = np.unique([0, 1, 2047, 4095, G - 2])      # not the row's last gene: a NaN key there is in place without a merge
    expr[const] = rng.integers(0, 4, size=(const.size, 1))
    _, p, padj = check_tests(dev, expr, groups, [(0, 2), (1, 2), (0, 1)], "wilcoxon", False)
    assert np.isnan(p[:, const]).all()               # sigma = 0
    assert np.array_equal(np.isnan(padj), np.isnan(p)) and not np.isnan(p).all(axis=1).any()
    assert min(len(np.unique(r[~np.isnan(r)])) for r in p) < G // 4        # many tied p


# ---------------------------------------------------------------- 3. waves
def test_jitter_in_later_waves(dev, monkeypatch):
    sizes = [130, 150, 125]
    groups, C = ec.sized_groups(sizes)
    G = 200
    expr = np.round(np.random.default_rng(31).normal(0.0, 1.0, size=(G, C)), 1)
    cmps = [(0, 2), (1, 2), (0, 1)]
    x = on_dev(expr)
    monkeypatch.delenv("ICNV_DE_SCRATCH_MB", raising=False)
    dev.de_stats(reset=True)
    one = run_tests(dev, x, groups, cmps, "wilcoxon", True, seed=6)
    assert dev.de_stats()["waves"] == 1
    monkeypatch.setenv("ICNV_DE_SCRATCH_MB", "1")
    dev.de_stats(reset=True)
    many = run_tests(dev, x, groups, cmps, "wilcoxon", True, seed=6)
    assert dev.de_stats()["waves"] > 1
    ref = restated(expr, groups, cmps, seed=6, whole_matrix=True)
    for a, b, c in zip(many, one, ref):
        same(a, c)
        same(a, b)


@pytest.mark.parametrize("jitter", [False, True])
def test_merged_segments_in_later_waves(dev, monkeypatch, jitter):
    groups, C = ec.sized_groups([4097, 30])          # 1 MiB holds 15 genes of 4127 cells: three waves, one merge pass
    G = 40
    expr = np.round(np.random.default_rng(33).normal(0.0, 1.0, size=(G, C)), 2)
    monkeypatch.setenv("ICNV_DE_SCRATCH_MB", "1")
    dev.de_stats(reset=True)
    check_tests(dev, expr, groups, [(0, 1), (1, 0)], "wilcoxon", jitter, seed=8, whole_matrix=True)
    st = dev.de_stats()
    assert st["waves"] > 1 and st["segments_hbm"] == G


def test_error_names_the_smallest_position_across_waves(dev, monkeypatch):
    from infercnv_amd import IcnvError
    groups, C = ec.sized_groups([130, 150, 125])
    G = 200
    expr = np.random.default_rng(35).normal(0.0, 1.0, size=(G, C))
    expr[5, groups[1]] = np.nan                      # comparison 1, gene 5: k G + g = 205, in the first wave
    expr[180, groups[0]] = np.inf                    # comparison 0, gene 180: 180, in the second
    cmps = [(0, 2), (1, 2)]
    monkeypatch.setenv("ICNV_DE_SCRATCH_MB", "1")
    dev.de_stats(reset=True)
    with pytest.raises(IcnvError, match=r"comparison 0 \(groups 0, 2\), gene 180:"):
        dev.de_tests(on_dev(expr), groups, cmps, jitter=False)
    with pytest.raises(ValueError, match="comparison 0, gene 180:"):
        dr.de_tests(expr, groups, cmps, jitter_on=False)
    expr[180, groups[0][0]] = 0.0                    # without the second one the first is named
    with pytest.raises(IcnvError, match=r"comparison 1 \(groups 1, 2\), gene 5:"):
        dev.de_tests(on_dev(expr), groups, cmps, jitter=False)
    expr[5, groups[1][3]] = 0.0
    dev.de_stats(reset=True)
    check_tests(dev, expr, groups, cmps, "wilcoxon", False)
    assert dev.de_stats()["waves"] == 2              # the positions above were in different waves


# ---------------------------------------------------------------- 4. p-value regimes
def test_wilcoxon_ladder(dev):
    expr, groups, cmps = ec.wilcoxon_ladder()
    reg = ec.wilcoxon_regimes(expr, groups, cmps)
    ec.check_wilcoxon_ladder(reg)
    _, p, padj = check_tests(dev, expr, groups, cmps, "wilcoxon", False)
    assert (p[reg == 4] == 0.0).all() and np.isnan(p[reg == 0]).all() and (p[(reg > 0) & (reg < 4)] > 0.0).all()
    assert (padj[reg == 4] == 0.0).all()             # BH on rows with exact zeros
    assert p[4, 3] == 0.0 and 0.0 < p[5, 3] < 2e-307  # the two sides of the 37.5193 cut


def test_exact_table_ends(dev):
    expr, groups, cmps = ec.exact_ends()
    W, p, _ = check_tests(dev, expr, groups, cmps, "wilcoxon", False)
    for k, (qx, qy) in enumerate(cmps):
        assert {W[k, 0], W[k, 1]} == {0.0, float(len(groups[qx]) * len(groups[qy]))}
        exact = ec.wilcox_z(expr[0, groups[qx]].tolist(), expr[0, groups[qy]].tolist()) is None
        assert exact == (len(groups[qx]) < 50 and len(groups[qy]) < 50)
    assert p[0, 0] == 1.0 and p[4, 0] == p[5, 1] and 0.0 < p[4, 0] < 1e-28


def test_welch_ladder(dev):
    expr, groups, cmps = ec.welch_ladder()
    pts = ec.welch_points(expr, groups, cmps)
    sides = ec.check_welch_ladder(pts)
    assert {"lower", "upper"} == set(sides)
    t, p, padj = check_tests(dev, expr, groups, cmps, "t", False)
    same(t, pts[:, :, 0])
    assert p[0, 0] == 1.0 and p[5, 5] == 0.0 and 0.0 < p[4, 4] < 1e-10
    assert padj[5, 5] == 0.0                         # BH on a row with an exact zero and a deep-tail p


# ---------------------------------------------------------------- 5. mask and mean at size
BIG_C = 65540                                        # beyond the 65535 cells one launch of de_mask_kernel covers
_big = {}


def big_case(G):
    """(expr, padj, base, cell_cmps, exact mean) of the 65540-cell mask, built once per G."""
    if G not in _big:
        rng = np.random.default_rng(50 + G)
        expr = rng.normal(1.0, 0.3, size=(G, BIG_C))
        padj = rng.uniform(size=(4, G))
        padj[1, ::5] = np.nan                        # NA is never DE
        c = np.arange(BIG_C)
        base = np.where(c < 40000, 2, 0)             # "reference" cells count every normal, as mask_plan sets them
        cell_cmps = [[] if i < 40000 else ([i % 4] if i % 3 == 0 else ([i % 4, (i + 1) % 4] if i % 3 == 1 else [])) for i in range(BIG_C)]
        cell_cmps[BIG_C - 1] = [0, 1, 2, 3]
        base[65538], cell_cmps[65538] = 2, []        # beyond one grid: a cell no rule masks, and 65537 (count 0) that all do
        assert base[65537] == 0 and cell_cmps[65537] == []
        mean = ec.exact_mean_fast(expr)
        if G == 3:
            assert mean == dr.exact_mean(expr)
        _big[G] = (expr, padj, base, cell_cmps, mean)
    return _big[G]


@pytest.mark.parametrize("rule", ["any", "most", "all"])
@pytest.mark.parametrize("G", [3, 257])
def test_mask_and_mean_beyond_one_grid(dev, G, rule):
    expr, padj, base, cell_cmps, mean = big_case(G)
    x, pj = on_dev(expr), torch.from_numpy(padj).cuda()
    got, used = dev.mask_non_de(x, pj, 0.5, base, cell_cmps, 2, rule=rule)
    assert used == mean
    ref = dr.mask(expr, padj, 0.5, base, cell_cmps, 2, rule, mean)
    changed = ref != expr
    assert changed[:, 65537].all() and not changed[:, 65538].any() and not changed[:, :40000].any()
    assert changed[:, 40000:65535].any() and not changed[:, 40000:65535].all()
    same(got.cpu().numpy().T, ref)
    same(x.cpu().numpy().T, expr)                    # the input is not written
    got, used = dev.mask_non_de(x, pj, 0.5, base, cell_cmps, 2, rule=rule, mask_val=-7.25)
    assert used == -7.25
    same(got.cpu().numpy().T, np.where(changed, -7.25, expr))


def small_mask_case(G=37, C=90, seed=61):
    rng = np.random.default_rng(seed)
    expr = rng.normal(1.0, 0.3, size=(G, C))
    padj = rng.uniform(size=(3, G))
    base = np.where(np.arange(C) < 30, 2, 0)
    cell_cmps = [[] if i < 30 else [i % 3, (i + 1) % 3][: 1 + i % 2] for i in range(C)]
    return expr, padj, base, cell_cmps


@pytest.mark.parametrize("test,jitter", [("wilcoxon", True), ("wilcoxon", False), ("t", False)])
def test_de_tests_on_a_padded_view(dev, test, jitter):
    groups, C = ec.sized_groups([20, 55, 130])
    expr = np.round(np.random.default_rng(63).normal(0.0, 1.0, size=(37, C)), 1)
    cmps = [(0, 1), (1, 2), (2, 0)]
    flat = run_tests(dev, on_dev(expr), groups, cmps, test, jitter, seed=3)
    wide, view = padded(expr, 11)
    assert view.stride(0) == 48 and not view.is_contiguous()
    got = run_tests(dev, view, groups, cmps, test, jitter, seed=3)
    for a, b, c in zip(got, flat, dr.de_tests(expr, groups, cmps, test=test, jitter_on=jitter, seed=3)):
        same(a, b)
        same(a, c)
    assert torch.isnan(wide[:, 37:]).all()


@pytest.mark.parametrize("rule", ["any", "most", "all"])
def test_mask_on_padded_views(dev, rule):
    expr, padj, base, cell_cmps = small_mask_case()
    G, C = expr.shape
    pj = torch.from_numpy(padj).cuda()
    mean = dr.exact_mean(expr)
    ref = dr.mask(expr, padj, 0.4, base, cell_cmps, 2, rule, mean)
    assert (ref != expr).any() and (ref == expr).any()
    flat, used = dev.mask_non_de(on_dev(expr), pj, 0.4, base, cell_cmps, 2, rule=rule)
    assert used == mean
    same(flat.cpu().numpy().T, ref)
    wide, view = padded(expr, 11)
    out_wide = torch.full((C, G + 3), -12345.5, dtype=torch.float64, device="cuda")
    out, used = dev.mask_non_de(view, pj, 0.4, base, cell_cmps, 2, rule=rule, out=out_wide[:, :G])
    assert used == mean                              # the NaN padding of x is not part of the mean
    same(out_wide[:, :G].cpu().numpy().T, ref)
    assert (out_wide[:, G:] == -12345.5).all() and torch.isnan(wide[:, G:]).all()
    same(wide[:, :G].cpu().numpy().T, expr)
    # in place on the padded view: the mean is that of the unmasked matrix
    out, used = dev.mask_non_de(view, pj, 0.4, base, cell_cmps, 2, rule=rule, out=view)
    assert used == mean and out.data_ptr() == wide.data_ptr()
    same(wide[:, :G].cpu().numpy().T, ref)
    assert torch.isnan(wide[:, G:]).all()


@pytest.mark.parametrize("bad,want", [((np.inf,), np.inf), ((np.nan,), np.nan), ((np.inf, -np.inf), np.nan)])
def test_mean_fallback_is_r_mean(dev, bad, want):
    expr, padj, base, cell_cmps = small_mask_case(seed=67)
    for i, v in enumerate(bad):
        expr[5 + 20 * i, 31 + 40 * i] = v            # in cells that some rule masks and some rule keeps
    with np.errstate(invalid="ignore"):
        plain = float(np.mean(expr))
    assert plain == want or (math.isnan(plain) and math.isnan(want))
    for rule in ("any", "all"):
        got, used = dev.mask_non_de(on_dev(expr), torch.from_numpy(padj).cuda(), 0.4, base, cell_cmps, 2, rule=rule)
        assert used == want or (math.isnan(used) and math.isnan(want))
        same(got.cpu().numpy().T, dr.mask(expr, padj, 0.4, base, cell_cmps, 2, rule, want))


# ---------------------------------------------------------------- 6. group bookkeeping
@pytest.fixture(scope="module")
def book_case():
    rng = np.random.default_rng(71)
    return np.round(rng.normal(0.0, 1.0, size=(9, 120)), 1)


@pytest.mark.parametrize("test,jitter", [("wilcoxon", True), ("wilcoxon", False), ("t", False)])
def test_unused_and_empty_unused_groups_change_nothing(dev, book_case, test, jitter):
    A, B, U = np.arange(0, 40), np.arange(40, 100), np.arange(100, 120)
    plain = check_tests(dev, book_case, [A, B], [(0, 1), (1, 0)], test, jitter, seed=2)
    for extra in (U, np.zeros(0, dtype=np.int64)):
        got = check_tests(dev, book_case, [extra, A, extra, B, extra], [(1, 3), (3, 1)], test, jitter, seed=2)
        for a, b in zip(got, plain):
            same(a, b)


def test_empty_group_in_a_comparison_is_an_error(dev, book_case):
    from infercnv_amd import IcnvError
    A, B, E = np.arange(0, 40), np.arange(40, 100), np.zeros(0, dtype=np.int64)
    with pytest.raises(IcnvError, match=r"comparison 1 \(groups 2, 1\), gene 0:"):
        dev.de_tests(on_dev(book_case), [A, E, B], [(0, 2), (2, 1)], jitter=False)
    with pytest.raises(ValueError, match="comparison 1, gene 0:"):
        dr.de_tests(book_case, [A, E, B], [(0, 2), (2, 1)], jitter_on=False)
    with pytest.raises(IcnvError, match=r"comparison 0 \(groups 1, 1\), gene 0:"):
        dev.de_tests(on_dev(book_case), [A, E, B], [(1, 1)], jitter=True)


@pytest.mark.parametrize("test,jitter", [("wilcoxon", True), ("wilcoxon", False), ("t", False)])
def test_self_comparison(dev, book_case, test, jitter):
    groups = [np.arange(0, 40), np.arange(40, 100), np.arange(100, 120)]
    stat, p, _ = check_tests(dev, book_case, groups, [(1, 1), (0, 1), (2, 2)], test, jitter, seed=5)
    if test == "wilcoxon":                           # every value ties with itself: W = n^2 / 2, the normal branch, p = 1
        assert (stat[0] == 1800.0).all() and (stat[2] == 200.0).all() and (p[[0, 2]] == 1.0).all()
    else:
        assert (stat[[0, 2]] == 0.0).all() and (p[[0, 2]] == 1.0).all()


def test_shared_cell_ties_under_jitter(dev, book_case):
    # the jitter belongs to (gene, cell): a cell in both samples is an exact tie, so 20 vs 21 cells take the normal branch
    groups = [np.arange(0, 20), np.arange(19, 40), np.arange(50, 70)]
    expr = book_case + np.random.default_rng(73).normal(0.0, 1e-3, size=book_case.shape)     # no ties in the data
    for g in range(expr.shape[0]):
        v = [expr[g, c] + dr.jitter(7, g, c) for c in range(70)]
        assert dr.wilcox(v[0:20], v[19:40])[2] == 6 and ec.wilcox_z(v[0:20], v[19:40]) is not None
        assert ec.wilcox_z(v[0:20], v[50:70]) is None
    check_tests(dev, expr, groups, [(0, 1), (1, 0), (0, 2)], "wilcoxon", True, seed=7)


@pytest.mark.parametrize("test,jitter", [("wilcoxon", True), ("wilcoxon", False), ("t", False)])
def test_cell_twice_in_a_group(dev, book_case, test, jitter):
    groups = [np.array([3, 4, 5, 3, 9, 11, 3]), np.arange(40, 100), np.array([20, 21, 21, 22])]
    check_tests(dev, book_case, groups, [(0, 1), (1, 0), (2, 0)], test, jitter, seed=11)
