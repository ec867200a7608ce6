"""The data layer of plot_cnv on the GPU (icnv_quantiles_excluding / icnv_heatmap_bins / icnv_heatmap_raster, DESIGN K17) and
infercnv_amd.heatmap.plot_cnv, against the sequential restatement of tests/heatmap_restate.py.  Every comparison is exact:
bit-equal doubles, equal integers, byte-equal files."""
import json
import os

import numpy as np
import pytest

import heatmap_restate as hmr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from infercnv_amd import GeneOrder, IcnvError, InfercnvObject   # noqa: E402
from infercnv_amd import heatmap as hm                           # noqa: E402
from infercnv_amd import tumor_subclusters as ts                 # noqa: E402


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infercnv_amd import device
    torch.cuda.set_device(0)
    device.init(0)
    return device


def same(a, b):
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    assert a.shape == b.shape
    bad = a.view(np.uint64) != b.view(np.uint64)
    assert not bad.any(), f"{int(bad.sum())} differ, first at {np.argwhere(bad)[0]}: {a[bad][0]!r} vs {b[bad][0]!r}"


def on_dev(dev, x_cg, padded):
    """(C, G) host matrix -> CUDA tensor; padded: the padded_matrix layout with NaN in the padding (never to be read)."""
    x_cg = np.ascontiguousarray(x_cg, dtype=np.float64)
    if not padded:
        return torch.from_numpy(x_cg).cuda()
    C, G = x_cg.shape
    ld = (G + 15) // 16 * 16 + 16
    full = torch.full((C, ld), float("nan"), dtype=torch.float64, device="cuda")
    view = full[:, :G]
    view.copy_(torch.from_numpy(x_cg))
    return view


# ---------------------------------------------------------------- quantiles
SHAPES = {"7x13": (7, 13, False), "67x1000_padded": (67, 1000, True), "1031x3057": (1031, 3057, False)}
PROBS = [(0.01, 0.99), (0.0, 1.0), (0.0, 0.01, 0.25, 1.0 / 3.0, 0.5, 0.75, 0.99, 1.0)]
CENTER = 1.0
DATA = ["normal", "dominant_other", "dominant_excluded", "identical", "kept1", "kept2", "mix", "mix_drop_zero"]
_qcache = {}


def quant_case(shape, kind):
    """(x (C, G), exclude, sorted-based restatement per probability set), made once."""
    key = (shape, kind)
    if key in _qcache:
        return _qcache[key]
    C, G, _ = SHAPES[shape]
    rng = np.random.default_rng(17)
    x = rng.normal(1.0, 0.1, size=(C, G))
    exclude = CENTER
    if kind == "dominant_other":
        x[rng.random((C, G)) < 0.9] = 1.05
    elif kind == "dominant_excluded":
        x[rng.random((C, G)) < 0.9] = CENTER
    elif kind == "identical":
        x[:] = CENTER
        x[rng.random((C, G)) < 0.3] = 0.93
        x[0, 0] = 0.93
    elif kind == "kept1":
        x[:] = CENTER
        x[C // 2, G // 3] = 1.25
    elif kind == "kept2":
        x[:] = CENTER
        x[C // 2, G // 3] = 1.25
        x[C - 1, G - 1] = 0.75
    elif kind in ("mix", "mix_drop_zero"):
        pool = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308, 1e300, -1e300, 1.0, -1.0,
                         0.5, -0.5, 3.0, 1e-300, -1e-300])
        x = np.where(rng.random((C, G)) < 0.7, rng.choice(pool, size=(C, G)), rng.normal(0.0, 2.0, size=(C, G)))
        exclude = float("nan") if kind == "mix" else 0.0
    ref = [hmr.quantiles_excluding(x, exclude, p) for p in PROBS]
    _qcache[key] = (x, exclude, ref)
    return _qcache[key]


@pytest.mark.parametrize("kind", DATA)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_quantiles(dev, shape, kind):
    x, exclude, ref = quant_case(shape, kind)
    t = on_dev(dev, x, SHAPES[shape][2])
    dev.heatmap_stats(reset=True)
    for probs, want in zip(PROBS, ref):
        got = dev.quantiles_excluding(t, exclude, probs)
        same(got["lo"], want["lo"])
        same(got["hi"], want["hi"])
        same(got["quantiles"], want["quantiles"])
        assert (got["n_kept"], got["n_excluded"]) == (want["n_kept"], want["n_excluded"])
        same(got["min"], want["min"])
        same(got["max"], want["max"])
    st = dev.heatmap_stats()
    assert st["calls"] == len(PROBS) and len(PROBS) <= st["radix_passes"] <= 8 * len(PROBS) and st["candidates"] <= 4096 * len(PROBS)


def test_quantiles_refusals(dev):
    x, exclude, _ = quant_case("67x1000_padded", "normal")

    def refused(xm, excl, probs):
        t = on_dev(dev, xm, True)
        n = len(probs)
        outs = [np.full(n, -7.0), np.full(2 * n, -7.0), np.full(2, -7, dtype=np.int64), np.full(2, -7.0)]
        with pytest.raises(IcnvError) as e:
            dev.quantiles_excluding_into(t, excl, probs, *outs)
        assert e.value.code == 1
        for o in outs:
            assert (o == -7).all()

    for bad in (float("nan"), float("inf"), float("-inf")):
        xm = x.copy()
        xm[-1, -1] = bad
        refused(xm, exclude, (0.01, 0.99))
    refused(np.full_like(x, CENTER), CENTER, (0.01, 0.99))      # n_kept == 0
    refused(x, exclude, (0.5, 1.5))
    refused(x, exclude, (-0.1,))
    refused(x, exclude, (float("nan"),))
    refused(x, exclude, tuple(np.linspace(0, 1, 9)))


# ---------------------------------------------------------------- bins
def bins_case(nb):
    rng = np.random.default_rng(170 + nb)
    breaks = np.linspace(0.8, 1.2, nb) if nb > 2 else np.array([0.9, 1.1])
    C, G = 41, 2500                      # more than one chunk of a row, and a ragged one
    x = rng.normal(1.0, 0.12, size=(C, G))
    x[3, :nb] = breaks                   # exactly on every break
    x[5, :nb] = np.nextafter(breaks, np.inf)
    x[7, :nb] = np.nextafter(breaks, -np.inf)
    x[9, :4] = [-np.inf, np.inf, -1e300, 1e300]
    return x, breaks


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("nb", [2, 16, 257])
def test_bins(dev, nb, padded):
    x, breaks = bins_case(nb)
    t = on_dev(dev, x, padded)
    rows = np.unique(np.concatenate([np.random.default_rng(3).permutation(x.shape[0])[:29], [3, 5, 7, 9]]))
    np.random.default_rng(4).shuffle(rows)          # a permuted subset that holds the planted cells
    for r in (None, rows):
        got = dev.heatmap_bins(t, breaks, r)
        want = hmr.bins(x, breaks, np.arange(x.shape[0]) if r is None else r)
        assert got.dtype == np.int64 and np.array_equal(got, want)
        assert int(got.sum()) == (x.shape[0] if r is None else rows.size) * x.shape[1]


def test_bins_refusals(dev):
    x, breaks = bins_case(16)
    t = on_dev(dev, x, False)
    out = np.full(300, -7, dtype=np.int64)

    def refused(tt, br, rows):
        with pytest.raises(IcnvError) as e:
            dev.heatmap_bins(tt, br, rows, out=out)
        assert e.value.code == 1 and (out == -7).all()

    refused(t, breaks[:1], None)
    refused(t, np.linspace(0, 1, 258), None)
    refused(t, breaks[::-1], None)
    refused(t, np.array([0.8, 0.9, 0.9, 1.0]), None)
    refused(t, np.array([0.8, np.inf]), None)
    refused(t, breaks, [0, 41])
    refused(t, breaks, [-1])
    xn = x.copy()
    xn[-1, -1] = np.nan
    refused(on_dev(dev, xn, False), breaks, None)
    got = dev.heatmap_bins(on_dev(dev, xn, False), breaks, np.arange(40))     # the NaN's cell is not listed
    assert np.array_equal(got, hmr.bins(xn, breaks, np.arange(40)))


# ---------------------------------------------------------------- raster
@pytest.mark.parametrize("padded", [False, True])
def test_raster(dev, padded):
    rng = np.random.default_rng(171)
    C, G = 41, 300
    x = rng.normal(1.0, 0.12, size=(C, G))
    breaks = np.linspace(0.8, 1.2, 16)
    x[2, :16] = breaks
    t = on_dev(dev, x, padded)
    order = rng.permutation(C)[:29]
    for H in (1, 13, 29, 64):
        for W in (1, 77, 300, 701):
            got = dev.heatmap_raster(t, breaks, order, H, W)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (H, W)
            assert np.array_equal(got.cpu().numpy(), hmr.raster(x, breaks, order, H, W)), (H, W)
    out = torch.full((5, 7), 99, dtype=torch.uint8, device="cuda")
    xn = x.copy()
    xn[order[2], :] = np.nan                        # pixel row 0 of 5 shows order[(1 * 29) // 10]
    with pytest.raises(IcnvError):
        dev.heatmap_raster(on_dev(dev, xn, padded), breaks, order, 5, 7, out=out)
    with pytest.raises(IcnvError):
        dev.heatmap_raster(t, breaks, [C], 5, 7, out=out)
    assert (out.cpu().numpy() == 99).all()


# ---------------------------------------------------------------- plot_cnv end to end
def synthetic_object():
    """300 genes over 4 chromosomes, 96 cells: observation groups of 60, 2 and 1 cells, reference groups of 31 and 2."""
    rng = np.random.default_rng(172)
    G, C = 300, 96
    chrs = np.repeat(["chr1", "chr2", "chr7", "chrX"], [120, 90, 60, 30])
    expr = rng.normal(1.0, 0.04, size=(G, C))
    expr[120:210, 5:40] += 0.12                 # a gain and a loss, so that the trees have something to find
    expr[0:60, 30:70] -= 0.1
    expr[rng.random((G, C)) < 0.4] = 1.0        # the mass that denoising leaves on the centre
    perm = rng.permutation(C)
    refs = {"normal_a": np.sort(perm[:31]), "nb": np.sort(perm[31:33])}
    obs = {"tumor_big": np.sort(perm[33:93]), "pair": np.sort(perm[93:95]), "a_single_cell_group": perm[95:96]}
    return InfercnvObject(expr_data=expr, gene_order=GeneOrder(chr=chrs), reference_grouped_cell_indices=refs,
                          observation_grouped_cell_indices=obs, gene_names=np.array([f"G{i}" for i in range(G)]),
                          cell_names=np.array([f"cell-{i:02d}" for i in range(C)]))


def with_subclusters(obj, by_groups):
    """tumor_subclusters as the library's own steps leave them, with trees from the restatement: one tree for the big group
    split in two subclusters by cutree, none for the groups of 2 and 1; or all_observations."""
    import hclust_restate as hr
    x_cg = np.asarray(obj.expr_data).T
    names = obj.cells()
    out = obj.copy()

    def tree(cells):
        m, h, o = hr.hclust(hr.seq_dist(x_cg[cells]), "ward.D2")
        return ts.HClust(m, h, o, names[cells], "ward.D2")

    if by_groups:
        hc, subs = {}, {}
        for g, cells in obj.observation_grouped_cell_indices.items():
            cells = np.asarray(cells)
            if cells.size > 2:
                hc[g] = tree(cells)
                cut = hmr.cutree_k(hc[g].merge, 2)
                subs[g] = {f"{g}_s{k}": cells[cut == k] for k in (1, 2)}
            else:
                hc[g], subs[g] = None, {f"{g}_s1": cells}
        # a Leiden-style group: the list of its partitions' trees, a partition of one cell among them
        big = np.asarray(obj.observation_grouped_cell_indices["tumor_big"])
        parts = [big[:40], big[40:59], big[59:]]
        hc["tumor_big"] = [tree(p) for p in parts if p.size >= 2]
        subs["tumor_big"] = {f"tumor_big_s{i + 1}": p for i, p in enumerate(parts)}
    else:
        cells = np.sort(np.concatenate([np.asarray(v) for v in obj.observation_grouped_cell_indices.values()]))
        t = tree(cells)
        cut = hmr.cutree_k(t.merge, 2)
        hc = {"all_observations": t}
        subs = {"all_observations": {f"all_observations_s{k}": cells[cut == k] for k in (1, 2)}}
    out.tumor_subclusters = {"hc": hc, "subclusters": subs}
    return out


def check_plot(dev, obj, tmp_path, **kw):
    got_dir, want_dir = str(tmp_path / "got"), str(tmp_path / "want")
    ret = hm.plot_cnv(obj, got_dir, **kw)
    page, layout = hmr.plot_cnv(obj, want_dir, **kw)
    names = sorted(os.listdir(want_dir))
    assert f"{kw.get('output_filename', 'infercnv')}.observation_groupings.txt" in names
    extra = {n for n in os.listdir(got_dir) if n.endswith((".png", ".json"))}
    assert sorted(set(os.listdir(got_dir)) - extra) == names
    for n in names:
        with open(os.path.join(got_dir, n), "rb") as a, open(os.path.join(want_dir, n), "rb") as b:
            assert a.read() == b.read(), n
    name = kw.get("output_filename", "infercnv")
    if kw.get("output_format", "png") == "png":
        assert extra == {f"{name}.heatmap.png", f"{name}.heatmap_layout.json"}
        assert np.array_equal(hmr.png_decode(os.path.join(got_dir, f"{name}.heatmap.png")), page)
        with open(os.path.join(got_dir, f"{name}.heatmap_layout.json")) as f:
            assert json.load(f) == json.loads(json.dumps(layout))
    else:
        assert not extra
    return ret, names


ROUTES = [
    dict(sub=None, cluster_by_groups=True, x_range="auto"),
    dict(sub=None, cluster_by_groups=False, k_obs_groups=3, x_range=(0.85, 1.2), write_expr_matrix=True),
    dict(sub=None, cluster_by_groups=False, k_obs_groups=1, x_range=None, color_safe_pal=True, cluster_references=False),
    dict(sub=True, cluster_by_groups=True, x_range="auto", write_expr_matrix=True, output_filename="run7"),
    dict(sub=False, cluster_by_groups=False, k_obs_groups=3, x_range="auto", hclust_method="average"),
    dict(sub=False, cluster_by_groups=False, k_obs_groups=1, x_range=(0.9, 1.1), output_format=None),
]


@pytest.mark.parametrize("route", range(len(ROUTES)))
def test_plot_cnv_synthetic(dev, tmp_path, route):
    kw = dict(ROUTES[route])
    sub = kw.pop("sub")
    obj = synthetic_object()
    if sub is not None:
        obj = with_subclusters(obj, sub)
    ret, names = check_plot(dev, obj, tmp_path, png_res=40, x_center=1.0, **kw)
    assert ret["x.center"] == 1.0 and ret["png_res"] == 40 and ret["cluster_by_groups"] == kw["cluster_by_groups"]
    assert any(n.startswith("General_HCL_") for n in names) == (not kw["cluster_by_groups"])
    if kw["x_range"] == "auto":
        x = np.asarray(obj.expr_data)
        q = hmr.quantiles_excluding(x, 1.0, (0.01, 0.99))["quantiles"]
        d = max(abs(1.0 - q[0]), abs(q[1] - 1.0))
        assert ret["x.range"] == (1.0 - d, 1.0 + d)


def test_plot_cnv_default_center_and_resolution(dev, tmp_path):
    """x.center = mean(expr.data) and R's page at 300 dpi (3000 pixels wide)."""
    ret, _ = check_plot(dev, synthetic_object(), tmp_path)
    assert ret["png_res"] == 300


def test_plot_cnv_golden(dev, tmp_path, golden_dir):
    d = np.load(os.path.join(golden_dir, "infercnv_object_example.npz"), allow_pickle=True)
    expr = np.asarray(d["expr_data"], dtype=np.float64)
    G, C = expr.shape
    assert (G, C) == (4613, 20)
    obj = InfercnvObject(expr_data=expr, gene_order=GeneOrder(chr=d["chr_levels"][d["chr_codes"]]),
                         reference_grouped_cell_indices={"normal": d["ref_normal"]},
                         observation_grouped_cell_indices={"tumor": d["obs_tumor"]})
    check_plot(dev, obj, tmp_path, png_res=60, write_expr_matrix=True)
    check_plot(dev, obj, tmp_path / "b", png_res=60, cluster_by_groups=False, k_obs_groups=2, hclust_method="ward.D2")


def test_plot_cnv_not_implemented(dev, tmp_path):
    obj = synthetic_object()
    for kw in (dict(ref_contig="chr1"), dict(plot_chr_scale=True), dict(write_phylo=True), dict(output_format="pdf")):
        with pytest.raises(NotImplementedError):
            hm.plot_cnv(obj, str(tmp_path), **kw)
    with pytest.raises(ValueError):
        hm.plot_cnv(obj, str(tmp_path), hclust_method="nope")
    with pytest.raises(ValueError):
        hm.plot_cnv(obj, str(tmp_path), x_center=1.0, x_range=(1.05, 1.2))
    assert os.listdir(str(tmp_path)) == []
