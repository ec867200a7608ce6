"""Non-DE gene masking on the GPU (icnv_de_tests_dev / icnv_mask_non_de_dev, DESIGN K12): every statistic, p-value,
adjusted p-value and masked value bit-equal to the sequential restatement of tests/de_restate.py."""
import os

import numpy as np
import pytest

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


def check_tests(dev, expr, groups, cmps, test, jitter, seed=0):
    stat, p, padj = dev.de_tests(on_dev(expr), groups, cmps, test=test, jitter=jitter, seed=seed)
    rs, rp, ra = dr.de_tests(expr, groups, cmps, test=test, jitter_on=jitter, seed=seed)
    same(stat.cpu().numpy(), rs)
    same(p.cpu().numpy(), rp)
    same(padj.cpu().numpy(), ra)
    return p.cpu().numpy(), padj.cpu().numpy()


def sized_groups(sizes, C):
    idx = np.arange(C)
    out, o = [], 0
    for s in sizes:
        out.append(idx[o:o + s])
        o += s
    return out


@pytest.mark.parametrize("G", [1, 63, 64, 65])
def test_wilcoxon_jitter_sizes(dev, G):
    sizes = [1, 2, 49, 50, 120]
    C = sum(sizes)
    rng = np.random.default_rng(G)
    expr = rng.normal(1.0, 0.2, size=(G, C))
    expr[:, :60] = np.round(expr[:, :60], 1)      # ties before the jitter
    groups = sized_groups(sizes, C)
    cmps = [(q, r) for q in (2, 3, 4) for r in range(5) if q != r]
    check_tests(dev, expr, groups, cmps, "wilcoxon", True, seed=G)


def test_wilcoxon_ties_zero_nonfinite_no_jitter(dev):
    sizes = [1, 2, 49, 50, 500]
    C = sum(sizes)
    rng = np.random.default_rng(1)
    G = 40
    expr = rng.integers(-2, 3, size=(G, C)).astype(np.float64) * 0.5
    expr[expr == 0] = np.where(rng.random(int((expr == 0).sum())) < 0.5, -0.0, 0.0)
    expr[3, 5] = np.nan
    expr[4, 60] = np.inf
    expr[5, 200] = -np.inf
    expr[6, 2] = np.nan                            # the 2-cell group keeps one value
    groups = sized_groups(sizes, C)
    cmps = [(4, q) for q in range(4)] + [(3, 2), (2, 3)]
    check_tests(dev, expr, groups, cmps, "wilcoxon", False)
    # no ties at all below 50: the exact branch on both sides of the 49/50 boundary
    expr2 = rng.permutation(G * C).reshape(G, C).astype(np.float64)
    check_tests(dev, expr2, groups, cmps, "wilcoxon", False)


def test_wilcoxon_segments_beyond_lds(dev):
    big = 2 * 4096 + 777
    sizes = [big, 300, 37]
    C = sum(sizes)
    rng = np.random.default_rng(7)
    G = 3
    expr = np.round(rng.normal(0.0, 1.0, size=(G, C)), 2)
    groups = sized_groups(sizes, C)
    cmps = [(0, 1), (1, 0), (2, 0)]
    check_tests(dev, expr, groups, cmps, "wilcoxon", False)
    check_tests(dev, expr[:1], groups, cmps, "wilcoxon", True, seed=3)


def test_wilcoxon_many_genes_tiny_scratch_and_repeat(dev, monkeypatch):
    sizes = [10, 12, 40]
    C = sum(sizes)
    rng = np.random.default_rng(11)
    G = 10000
    expr = rng.integers(0, 6, size=(G, C)).astype(np.float64)
    groups = sized_groups(sizes, C)
    cmps = [(0, 2), (1, 2)]
    p1, a1 = check_tests(dev, expr, groups, cmps, "wilcoxon", False)
    monkeypatch.setenv("ICNV_DE_SCRATCH_MB", "1")
    dev.de_stats(reset=True)
    stat, p, padj = dev.de_tests(on_dev(expr), groups, cmps, test="wilcoxon", jitter=False)
    assert dev.de_stats()["waves"] > 1
    same(p.cpu().numpy(), p1)
    same(padj.cpu().numpy(), a1)


def test_jitter_seeds_and_scratch(dev, monkeypatch):
    sizes = [30, 45, 60]
    C = sum(sizes)
    rng = np.random.default_rng(5)
    G = 70
    expr = np.round(rng.normal(0.0, 1.0, size=(G, C)), 1)
    groups = sized_groups(sizes, C)
    cmps = [(0, 2), (1, 2), (0, 1)]
    x = on_dev(expr)
    a = dev.de_tests(x, groups, cmps, seed=1)[1].cpu().numpy()
    b = dev.de_tests(x, groups, cmps, seed=1)[1].cpu().numpy()
    c = dev.de_tests(x, groups, cmps, seed=2)[1].cpu().numpy()
    same(a, b)
    assert not np.array_equal(a, c)
    monkeypatch.setenv("ICNV_DE_SCRATCH_MB", "1")
    same(dev.de_tests(x, groups, cmps, seed=2)[1].cpu().numpy(), c)
    check_tests(dev, expr, groups, cmps, "wilcoxon", True, seed=2)


def test_empty_sample_is_an_error(dev):
    from infercnv_amd import IcnvError
    expr = np.ones((3, 6))
    expr[1, 4:] = np.nan
    with pytest.raises(IcnvError, match="gene 1"):
        dev.de_tests(on_dev(expr), [np.arange(4), np.arange(4, 6)], [(0, 1)], jitter=False)


def test_welch(dev):
    sizes = [1, 2, 3, 49, 50, 500]
    C = sum(sizes)
    rng = np.random.default_rng(3)
    G = 65
    expr = rng.normal(0.0, 1.0, size=(G, C)) * rng.uniform(0.1, 3.0, size=(G, 1)) + rng.normal(0, 1, size=(G, 1))
    expr[2, :] = 1.5                               # constant: NA
    expr[3, 10] = np.nan
    expr[4, 70] = np.inf
    expr[5, 3:6] = np.nan                          # 3-cell group down to 0 / 2 values
    expr[6, 3:5] = np.nan
    groups = sized_groups(sizes, C)
    cmps = [(5, q) for q in range(5)] + [(3, 4), (4, 3)]
    p, _ = check_tests(dev, expr, groups, cmps, "t", False)
    assert np.isnan(p[0]).all() and np.isnan(p[:, 2]).all()


def make_obj(G, normals, subclusters, seed=0, missing=()):
    from infercnv_amd import GeneOrder, InfercnvObject
    rng = np.random.default_rng(seed)
    C = sum(normals) + sum(sum(s) for s in subclusters)
    expr = rng.normal(1.0, 0.3, size=(G, C))
    refs, obs, subs, o = {}, {}, {}, 0
    for k, n in enumerate(normals):
        refs[f"normal_{k}"] = np.arange(o, o + n)
        expr[: G // 3, o:o + n] += 0.5 * (k + 1)
        o += n
    for q, sizes in enumerate(subclusters):
        name = f"tumor_{q}"
        cells = {}
        for s, n in enumerate(sizes):
            cells[f"{name}.{s + 1}"] = np.arange(o, o + n)
            expr[G // 2:, o:o + n] -= 0.4 * (s + 1)
            o += n
        obs[name] = np.concatenate(list(cells.values()))
        if name not in missing:
            subs[name] = cells
    obj = InfercnvObject(expr_data=expr, gene_order=GeneOrder(chr=np.array(["1"] * G)), reference_grouped_cell_indices=refs,
                         observation_grouped_cell_indices=obs, tumor_subclusters={"subclusters": subs})
    return obj


def restated_mask(obj, thresh, test_use, center_val, rule, seed, jitter):
    from infercnv_amd import mask_non_de as mn
    groups, pairs, entries = mn._comparisons(obj)
    G, C = obj.expr_data.shape
    if pairs:
        _, _, padj = dr.de_tests(obj.expr_data, groups, pairs, test=test_use, jitter_on=jitter, seed=seed)
    else:
        padj = np.zeros((0, G))
    base, cell_cmps = mn.mask_plan(C, obj, entries, mn._final(entries))
    mv = dr.exact_mean(obj.expr_data) if center_val is None else center_val
    return dr.mask(obj.expr_data, padj, thresh, base, cell_cmps, len(obj.reference_grouped_cell_indices), rule, mv)


@pytest.mark.parametrize("rule", ["any", "most", "all"])
@pytest.mark.parametrize("n_normal", [1, 2, 3])
def test_mask_rules(dev, rule, n_normal):
    from infercnv_amd.mask_non_de import mask_non_DE_genes_basic
    obj = make_obj(30, [12, 9, 15][:n_normal], [[8, 3, 20], [6], [7, 7]], seed=n_normal, missing=("tumor_2",))
    for test_use, jitter in (("wilcoxon", True), ("t", False)):
        got = mask_non_DE_genes_basic(obj, p_val_thresh=0.2, test_use=test_use, require_DE_all_normals=rule, seed=4, jitter=jitter)
        same(got.expr_data, restated_mask(obj, 0.2, test_use, None, rule, 4, jitter))
    got = mask_non_DE_genes_basic(obj, p_val_thresh=0.2, center_val=-7.0, require_DE_all_normals=rule, seed=4)
    same(got.expr_data, restated_mask(obj, 0.2, "wilcoxon", -7.0, rule, 4, True))


def test_mask_shared_cells_and_no_subclusters(dev):
    from infercnv_amd.mask_non_de import get_DE_genes_basic, mask_non_DE_genes_basic
    obj = make_obj(20, [10, 8], [[9, 6]], seed=9)
    subs = obj.tumor_subclusters["subclusters"]["tumor_0"]
    subs["tumor_0.3"] = np.concatenate([subs["tumor_0.1"][:4], subs["tumor_0.2"][:3]])   # cells in two subclusters
    got = mask_non_DE_genes_basic(obj, p_val_thresh=0.3, seed=2)
    same(got.expr_data, restated_mask(obj, 0.3, "wilcoxon", None, "any", 2, True))
    res = get_DE_genes_basic(obj, p_val_thresh=0.3, seed=2)
    assert list(res) == [f"tumor_0.{s},normal_{k}" for s in (1, 2, 3) for k in (0, 1)]
    obj.tumor_subclusters = None
    got = mask_non_DE_genes_basic(obj)
    same(got.expr_data, restated_mask(obj, 0.05, "wilcoxon", None, "any", 0, True))


def test_reference_example_object(dev, golden_dir):
    from infercnv_amd import GeneOrder, InfercnvObject
    from infercnv_amd.mask_non_de import get_DE_genes_basic, mask_non_DE_genes_basic
    d = np.load(os.path.join(golden_dir, "infercnv_object_example.npz"))
    obj = InfercnvObject(expr_data=d["expr_data"], gene_order=GeneOrder(chr=d["chr_codes"]),
                         reference_grouped_cell_indices={"normal": d["ref_normal"]},
                         observation_grouped_cell_indices={"tumor": d["obs_tumor"]},
                         tumor_subclusters={"subclusters": {"tumor": {"tumor_s1": d["obs_tumor"]}}})
    for jitter in (True, False):   # 10 vs 10 cells: the exact branch with jitter, ties and the normal approximation without
        res = get_DE_genes_basic(obj, seed=1, jitter=jitter)
        _, _, padj = dr.de_tests(obj.expr_data, [d["ref_normal"], d["obs_tumor"]], [(0, 1)], jitter_on=jitter, seed=1)
        same(np.array(list(res["tumor_s1,normal"]["pvals"].values())), padj[0])
        got = mask_non_DE_genes_basic(obj, seed=1, jitter=jitter)
        same(got.expr_data, restated_mask(obj, 0.05, "wilcoxon", None, "any", 1, jitter))
