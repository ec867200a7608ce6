"""The exact matrix sum on the GPU (icnv_matrix_sum_dev / icnv_matrix_sum, DESIGN K23), plot_per_group, plot_subclusters and
sample_object's device assembly, against the sequential restatement of tests/sampling_restate.py.  Every comparison is exact:
bit-equal doubles, byte-equal files."""
import ctypes as ct
import math
import os
import struct

import numpy as np
import pytest

import heatmap_restate as hmr
import sampling_restate as sr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from infercnv_amd import GeneOrder, InfercnvObject, _lib, sampling   # noqa: E402
from infercnv_amd import heatmap as hm                               # noqa: E402
from infercnv_amd import tumor_subclusters as ts                     # noqa: E402


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infercnv_amd import device
    torch.cuda.set_device(0)
    device.init(0)
    return device


def same_bits(a, b):
    return (a != a and b != b) or struct.pack("<d", a) == struct.pack("<d", b)


def padded(x_cg):
    """The [:, :G] view of a (C, G + 5) CUDA matrix whose padding holds NaN (never to be read)."""
    C, G = x_cg.shape
    full = torch.full((C, G + 5), float("nan"), dtype=torch.float64, device="cuda")
    full[:, :G] = torch.from_numpy(x_cg)
    return full[:, :G]


# ---------------------------------------------------------------- matrix_sum: shapes and values
SHAPES = [(1, 1), (1, 65), (3, 257), (70, 1000), (4097, 33)]       # (C, G): one value .. 34 tiles of 4096 values
KINDS = ["counts", "around_one", "cancel", "spread", "subnormal", "huge_pairs", "zeros"]
_cases = {}


def values(shape, kind):
    """((C, G) matrix, its exact sum), made once."""
    key = (shape, kind)
    if key in _cases:
        return _cases[key]
    C, G = shape
    n = C * G
    rng = np.random.default_rng(23)
    if kind == "counts":
        v = rng.poisson(3.0, n).astype(np.float64) * rng.integers(1, 2000, n)
    elif kind == "around_one":
        v = rng.normal(1.0, 0.08, n)
    elif kind == "cancel":                      # [1, 1e100, 1, -1e100] over every lane, wavefront and workgroup
        v = np.resize(np.array([1.0, 1e100, 1.0, -1e100]), n)
        v[n - n % 4:] = 0.5
        v = v[rng.permutation(n)] if n > 8 else v
    elif kind == "spread":                      # exponents over 1e-300 .. 1e300, every large value with its negative
        half = rng.random(n // 2) * 10.0 ** rng.integers(-300, 301, n // 2)
        v = np.concatenate([half, -half, np.full(n - 2 * (n // 2), 1e-300)])
        v[: n // 8] = rng.normal(0.0, 1.0, n // 8)
        v = v[rng.permutation(n)]
    elif kind == "subnormal":
        v = rng.integers(-2 ** 45, 2 ** 45, n).astype(np.float64) * 5e-324
    elif kind == "huge_pairs":                  # partial sums overflow, the total does not
        v = np.resize(np.array([1.7e308, 1.7e308, -1.7e308, -1.7e308]), n)
        v[n - n % 4:] = 3.0
        v = np.sort(v)[::-1].copy() if n > 4 else v
    else:
        v = np.resize(np.array([0.0, -0.0, -0.0]), n)
    x = np.ascontiguousarray(v.reshape(C, G))
    _cases[key] = (x, sr.exact_sum(x))
    return _cases[key]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_matrix_sum(dev, shape, kind):
    x, want = values(shape, kind)
    got = dev.matrix_sum(torch.from_numpy(x).cuda())
    got_padded = dev.matrix_sum(padded(x))
    print(shape, kind, got, got_padded, want)
    assert same_bits(got, want) and same_bits(got_padded, want)
    if kind == "zeros":
        assert math.copysign(1.0, got) == 1.0
    try:
        by_fsum = math.fsum(x.ravel())
    except OverflowError:                       # "intermediate overflow in fsum": the contract still holds
        assert kind == "huge_pairs"
    else:
        assert same_bits(got, by_fsum)
        assert same_bits(dev.matrix_mean(torch.from_numpy(x).cuda()), by_fsum / x.size)


def test_matrix_sum_all_negative_zero(dev):
    assert same_bits(dev.matrix_sum(torch.full((3, 7), -0.0, dtype=torch.float64, device="cuda")), 0.0)


def test_matrix_sum_overflow_to_infinity(dev):
    x = np.full((2, 3), 1.7e308)
    assert dev.matrix_sum(torch.from_numpy(x).cuda()) == math.inf == sr.exact_sum(x)
    assert dev.matrix_sum(torch.from_numpy(-x).cuda()) == -math.inf
    edge = np.array([[1.7976931348623157e308, 2.0 ** 970, 0.0]])       # the tie at the top of the range rounds to even: Inf
    assert dev.matrix_sum(torch.from_numpy(edge).cuda()) == math.inf == sr.exact_sum(edge)
    below = np.array([[1.7976931348623157e308, 2.0 ** 969, 0.0]])
    assert dev.matrix_sum(torch.from_numpy(below).cuda()) == 1.7976931348623157e308 == sr.exact_sum(below)


# ---------------------------------------------------------------- matrix_sum: rules and entries
PLACES = {"first": 0, "last": 70 * 1000 - 1, "end_of_workgroup": 4095, "start_of_workgroup": 4096}


@pytest.mark.parametrize("place", list(PLACES))
def test_matrix_sum_special_values(dev, place):
    base, _ = values((70, 1000), "around_one")
    at = np.unravel_index(PLACES[place], base.shape)
    other = np.unravel_index(33333, base.shape)
    for special, partner, want in ((math.nan, None, math.nan), (math.inf, None, math.inf), (-math.inf, None, -math.inf),
                                   (math.inf, -math.inf, math.nan), (math.inf, math.inf, math.inf), (math.nan, math.inf, math.nan),
                                   (-math.inf, 1.7e308, -math.inf)):
        x = base.copy()
        x[at] = special
        if partner is not None:
            x[other] = partner
        assert same_bits(sr.exact_sum(x), want)
        for t in (torch.from_numpy(x).cuda(), padded(x)):
            assert same_bits(dev.matrix_sum(t), want)


def test_matrix_sum_host_entry(dev):
    for shape in SHAPES:
        for kind in ("around_one", "spread"):
            x, want = values(shape, kind)
            assert same_bits(dev.matrix_sum(x), want)
            wide = np.full((shape[0], shape[1] + 5), np.nan)
            wide[:, :shape[1]] = x
            assert same_bits(dev.matrix_sum(wide[:, :shape[1]]), want)
    with pytest.raises(TypeError):
        dev.matrix_sum(np.zeros((3, 4), dtype=np.float32))
    with pytest.raises(TypeError):
        dev.matrix_sum(np.zeros((4, 3)).T)


def test_matrix_sum_argument_errors(dev):
    L = _lib.load()
    x = torch.ones((4, 8), dtype=torch.float64, device="cuda")
    host = np.ones((4, 8))
    out = ct.c_double(-1.0)
    p, hp, null = ct.c_void_p(x.data_ptr()), ct.c_void_p(host.ctypes.data), ct.c_void_p(0)
    for ptr, ld, G, C, res in ((null, 8, 8, 4, ct.byref(out)), (p, 8, 8, 4, None), (p, 8, 0, 4, ct.byref(out)), (p, 8, 8, 0, ct.byref(out)),
                               (p, 1 << 31, 1 << 31, 1, ct.byref(out)), (p, 8, 8, 1 << 31, ct.byref(out)), (p, 7, 8, 4, ct.byref(out)),
                               (p, 8, -1, 4, ct.byref(out))):
        assert L.icnv_matrix_sum_dev(ptr, ld, G, C, res, None) == _lib.ERR_ARG
        assert L.icnv_matrix_sum(hp if ptr is p else ptr, ld, G, C, res) == _lib.ERR_ARG
    assert out.value == -1.0
    assert L.icnv_matrix_sum_dev(p, 8, 8, 4, ct.byref(out), None) == _lib.OK and out.value == 32.0


# ---------------------------------------------------------------- plot_per_group
def group_object(with_ts):
    """40 genes on 3 contigs; reference groups of 9 and 12 cells, observation groups of 6, 31 and 1 cells (the one-cell group
    last: with tumor_subclusters it has no tree, and plot_cnv(cluster_by_groups = FALSE) stops there, as R does)."""
    sizes = {"ref/A": 9, "ref B": 12, "obs:6": 6, "obs31": 31, "single": 1}
    rng = np.random.default_rng(11)
    C, G = sum(sizes.values()), 40
    perm = rng.permutation(C)
    groups, at = {}, 0
    for name, n in sizes.items():
        groups[name] = np.sort(perm[at:at + n]).astype(np.int64)
        at += n
    expr = rng.normal(1.0, 0.1, size=(G, C))
    expr[10:25, groups["obs31"][:14]] += 0.3
    expr[rng.random((G, C)) < 0.05] = 1.0
    obj = InfercnvObject(expr_data=expr, gene_order=GeneOrder(chr=np.repeat(["chr1", "chr2", "chrX"], [15, 15, 10])),
                         reference_grouped_cell_indices={k: groups[k] for k in ("ref/A", "ref B")},
                         observation_grouped_cell_indices={k: groups[k] for k in ("obs:6", "obs31", "single")},
                         gene_names=np.array([f"G{i}" for i in range(G)]), cell_names=np.array([f"cell-{i:02d}" for i in range(C)]))
    if with_ts:
        hc, subs = {}, {}
        for name, cells in groups.items():
            if cells.size >= 2:
                hc[name] = ts.hclust(obj, cells, "ward.D2")
                cut = ts.cutree_h(hc[name].merge, hc[name].height, float(np.sort(hc[name].height)[-2]) if cells.size > 2 else -1.0)
                subs[name] = {f"{sr.make_filename(name)}_s{k}": cells[cut == k] for k in np.unique(cut)}     # (they name files)
            else:
                subs[name] = {f"{name}_s1": cells}
        obj.tumor_subclusters = {"hc": hc, "subclusters": subs}
    return obj


def listing(path):
    return sorted(os.listdir(path)) if os.path.isdir(path) else []


def same_directories(a, b):
    assert listing(a) == listing(b)
    for name in listing(a):
        with open(os.path.join(a, name), "rb") as f, open(os.path.join(b, name), "rb") as g:
            assert f.read() == g.read(), name
    return listing(a)


def by_hand(obj, out_dir, stop_at=None, on_references=True, on_observations=True, output_format="png", k_obs_groups=1,
            write_expr_matrix=True, base="infercnv_per_group"):
    """The restatement's per-group objects through the public plot_cnv, with the restatement's centre and range; the groups
    before `stop_at`.  The one-cell group stops inside plot_cnv (after expr.<name>.dat, as in R); a sampled group before it."""
    expr = np.asarray(obj.expr_data)
    center = sr.exact_sum(expr) / expr.size
    q = hmr.quantiles_excluding(expr, center, (0.01, 0.99))["quantiles"]
    t = obj.tumor_subclusters
    for tag, name, cells, group_ts in sr.per_group_objects(obj.reference_grouped_cell_indices, obj.observation_grouped_cell_indices,
                                                           t["hc"] if t else None, t["subclusters"] if t else None,
                                                           on_references, on_observations):
        if name == stop_at and name != "single":
            return
        one = InfercnvObject(expr_data=expr[:, cells], gene_order=obj.gene_order, observation_grouped_cell_indices={name: np.arange(len(cells))},
                             tumor_subclusters=None if group_ts is None else
                             {"hc": group_ts["hc"], "subclusters": {g: {s: np.asarray(v) for s, v in d.items()} for g, d in group_ts["subclusters"].items()}},
                             gene_names=obj.gene_names, cell_names=obj.cell_names[cells])
        draw = lambda: hm.plot_cnv(one, out_dir=out_dir, title=f"inferCNV {name}", obs_title=name, ref_title="", cluster_by_groups=False,
                                   cluster_references=False, k_obs_groups=k_obs_groups, contig_cex=1, x_center=center,
                                   x_range=(float(q[0]), float(q[1])), color_safe_pal=False,
                                   output_filename=f"{base}_{tag}_{sr.make_filename(name)}", output_format=output_format, png_res=40,
                                   dynamic_resize=0, ref_contig=None, write_expr_matrix=write_expr_matrix, useRaster=True)
        if name == stop_at:
            with pytest.raises(ValueError, match="all_observations"):
                draw()
            return
        draw()


def first_above(obj, above_m, on_references=True):
    groups = (list(obj.reference_grouped_cell_indices.items()) if on_references else []) + list(obj.observation_grouped_cell_indices.items())
    return next((name for name, cells in groups if len(cells) > above_m), None)


PER_GROUP = {"plain": dict(), "no_figure": dict(output_format=None), "observations_only": dict(on_references=False),
             "two_dendrogram_groups": dict(k_obs_groups=2, write_expr_matrix=False)}


@pytest.mark.parametrize("with_ts", [False, True], ids=["no_subclusters", "subclusters"])
@pytest.mark.parametrize("case", list(PER_GROUP))
def test_plot_per_group(dev, tmp_path, case, with_ts):
    obj = group_object(with_ts)
    kw = PER_GROUP[case]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    stop_at = "single" if with_ts else None                     # no tree for one cell: R's as.dendrogram(NULL) stops
    if stop_at:
        with pytest.raises(ValueError, match="all_observations"):
            sampling.plot_per_group(obj, out_dir=a, png_res=40, **kw)
    else:
        assert sampling.plot_per_group(obj, out_dir=a, png_res=40, **kw) is None
    by_hand(obj, b, stop_at, **kw)
    names = same_directories(a, b)
    drawn = [("REF", "ref_A"), ("REF", "ref B")] * (kw.get("on_references", True)) + [("OBS", "obs_6"), ("OBS", "obs31")] + \
        ([] if with_ts else [("OBS", "single")])
    per_group = ["heatmap_thresholds.txt", "observation_groupings.txt"] + \
        (["heatmap.png", "heatmap_layout.json"] if kw.get("output_format", "png") == "png" else []) + \
        (["observations.txt"] if kw.get("write_expr_matrix", True) else [])
    expected = {f"infercnv_per_group_{tag}_{g}.{suffix}" for tag, g in drawn for suffix in per_group}
    if kw.get("write_expr_matrix", True):
        expected |= {f"expr.infercnv_per_group_{tag}_{g}.dat" for tag, g in drawn + ([("OBS", "single")] if with_ts else [])}
    others = set(names) - expected
    assert expected <= set(names) and others and all(n.startswith("General_HCL_") and n.endswith("_members.txt") for n in others)


@pytest.mark.parametrize("with_ts", [False, True], ids=["no_subclusters", "subclusters"])
@pytest.mark.parametrize("sample_kw", [dict(n_cells=5, above_m=5), dict(every_n=3, above_m=5), dict(n_cells=5, above_m=9),
                                       dict(every_n=3, above_m=12), dict(n_cells=5, above_m=100)],
                         ids=lambda d: "-".join(f"{k}{v}" for k, v in d.items()))
def test_plot_per_group_sampled(dev, tmp_path, sample_kw, with_ts):
    """R's plot_per_group(sample = TRUE) stops at the first group above above_m (sample_object files the new tree under the
    group's name, plot_cnv reads all_observations; every_n stops inside sample_object): the groups before it are drawn as
    without sampling, then ValueError."""
    obj = group_object(with_ts)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    stop_at = first_above(obj, sample_kw["above_m"]) or ("single" if with_ts else None)
    text = "all_observations" if stop_at == "single" else (r"infercnv_sampling\.R:274" if "every_n" in sample_kw else "was sampled")
    if stop_at:
        with pytest.raises(ValueError, match=text):
            sampling.plot_per_group(obj, sample=True, out_dir=a, png_res=40, write_expr_matrix=False, **sample_kw)
    else:
        sampling.plot_per_group(obj, sample=True, out_dir=a, png_res=40, write_expr_matrix=False, **sample_kw)
    by_hand(obj, b, stop_at, write_expr_matrix=False)
    names = same_directories(a, b)
    assert bool(names) == (stop_at != "ref/A")


# ---------------------------------------------------------------- plot_subclusters
def test_plot_subclusters(dev, tmp_path):
    obj = group_object(True)
    subs = obj.tumor_subclusters["subclusters"]
    subs["all_observations"] = {"obs31_s1": subs["obs31"]["obs31_s1"][::-1].copy()}     # a repeated name: replaces in place
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    got = ts.plot_subclusters(obj, a, output_filename="subs")
    ref, obs = sr.subcluster_object(obj.reference_grouped_cell_indices, obj.observation_grouped_cell_indices, obj.tumor_subclusters["subclusters"])
    assert list(got.reference_grouped_cell_indices) == list(ref) and list(got.observation_grouped_cell_indices) == list(obs)
    assert list(obs).index("obs31_s1") < list(obs).index("single_s1")
    for d, want in ((got.reference_grouped_cell_indices, ref), (got.observation_grouped_cell_indices, obs)):
        for k, v in want.items():
            assert np.asarray(d[k]).tolist() == v
    assert got.tumor_subclusters is None and got.expr_data is obj.expr_data and obj.tumor_subclusters is not None
    hand = InfercnvObject(expr_data=obj.expr_data, gene_order=obj.gene_order, reference_grouped_cell_indices={k: np.asarray(v) for k, v in ref.items()},
                          observation_grouped_cell_indices={k: np.asarray(v) for k, v in obs.items()}, gene_names=obj.gene_names,
                          cell_names=obj.cell_names)
    hm.plot_cnv(hand, out_dir=b, cluster_by_groups=True, output_filename="subs", write_expr_matrix=False)
    assert same_directories(a, b) == ["subs.heatmap.png", "subs.heatmap_layout.json", "subs.heatmap_thresholds.txt",
                                      "subs.observation_groupings.txt"]


# ---------------------------------------------------------------- sample_object on the device
def test_sample_object_device_assembly(dev):
    obj = group_object(True)
    x = torch.from_numpy(np.ascontiguousarray(obj.expr_data.T)).cuda()
    for kw in (dict(n_cells=4), dict(n_cells=20), dict(every_n=3, above_m=5), dict(n_cells=20, on_references=False)):
        host = sampling.sample_object(obj, seed=7, **kw)
        on_device = sampling.sample_object(obj, seed=7, x_dev=x, **kw)
        meta, x_new = sampling.sample_object(obj, seed=7, x_dev=x, return_device=True, **kw)
        assert host.expr_data.shape[1] == len(host.cells()) and list(host.cells()) == list(on_device.cells()) == list(meta.cells())
        assert np.array_equal(host.expr_data.view(np.uint64), on_device.expr_data.view(np.uint64))
        assert np.array_equal(x_new.cpu().numpy().view(np.uint64), np.ascontiguousarray(host.expr_data.T).view(np.uint64))
        assert meta.expr_data is None
        if kw.get("n_cells") == 20:                             # up-sampled groups hold duplicated columns
            assert len(set(sampling.sample_plan(obj, seed=7, **kw).source.tolist())) < host.expr_data.shape[1]
