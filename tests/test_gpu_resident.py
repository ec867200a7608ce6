"""Device-resident infercnv objects on the GPU (DESIGN K32): the reference z-score gene filter (icnv_zscore_gene_filter_dev)
against the exact restatement of tests/zscore_restate.py, bit for bit; its refusals; the kept-gene set of a resident object
against the host route's; and the steps that take a DeviceMatrix, against the same steps on the host copy of the object."""
import contextlib
import ctypes as ct
import os
import struct

import numpy as np
import pytest

import zscore_restate as zr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from infercnv_amd import DeviceMatrix, GeneOrder, InfercnvObject, _lib   # noqa: E402
from infercnv_amd import tumor_subclusters as ts                         # noqa: E402


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infercnv_amd import device
    torch.cuda.set_device(0)
    device.init(0)
    return device


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return (a != a and b != b) or struct.pack("<d", a) == struct.pack("<d", b)


# ---------------------------------------------------------------- the kernel against the exact restatement
C_CELLS = 40
GENES = [1, 63, 64, 65, 257]          # one lane; one short of, exactly, one past a workgroup's 64 genes; five workgroups
N_REFS = [1, 2, 33]                   # one row; two wavefronts' rows; every wavefront with several rows, not a multiple of 4
KINDS = ["expr", "edge"]
_cases = {}


def ref_list(n_ref):
    """n_ref cells scattered over the 40, in no ascending order."""
    order = (np.arange(C_CELLS) * 17 + 5) % C_CELLS           # a permutation of 0 .. 39 (17 and 40 are coprime)
    cells = order[:n_ref].astype(np.int32)
    assert n_ref < 3 or np.any(np.diff(cells) < 0)
    return cells


def host_row_means(x, cells):
    """The host route's row means (tumor_subclusters.zscore_outlier_genes before its comparison)."""
    ref = x[:, cells]
    m, s = ts._r_mean(ref), ts._r_sd(ref)
    with np.errstate(all="ignore"):
        z = np.abs((ref - m) / s)
    return np.array([ts._r_mean(z[g]) for g in range(z.shape[0])])


def plant(x, cells, g, target):
    """Give gene g values mean +- t * sd over the listed cells, with t iterated until the host route's row mean of the gene is
    `target` (the gene's own values move the mean and the sd, so t is found by a few fixed-point steps)."""
    signs = np.where(np.arange(cells.size) % 2 == 0, 1.0, -1.0)
    t = target
    for _ in range(40):
        ref = x[:, cells]
        m, s = ts._r_mean(ref), ts._r_sd(ref)
        x[g, cells] = m + signs * t * s
        r = host_row_means(x, cells)[g]
        if abs(r - target) <= 1e-13:
            break
        t *= target / r
    return x


def case(G, n_ref, kind):
    """((G, C) matrix, cells, (mean, sd, row_mean) of the restatement), made once and never changed."""
    key = (G, n_ref, kind)
    if key in _cases:
        return _cases[key]
    rng = np.random.default_rng(1000 * G + 10 * n_ref + len(kind))
    cells = ref_list(n_ref)
    if kind == "expr":
        # the matrix the filter reads in run(): residuals around 1 with a few gene-wide shifts
        x = 1.0 + 0.08 * rng.standard_normal((G, C_CELLS))
        x[rng.random(G) < 0.2] += 0.15
        if G >= 63 and n_ref >= 2:
            # one gene a hair above the 0.8 of the decision and one a hair below
            for _ in range(3):                                 # (planting one moves the other's mean and sd a little)
                x = plant(x, cells, 7, 0.8 * (1 + 1e-8))
                x = plant(x, cells, 40, 0.8 * (1 - 1e-8))
    else:
        # signed zeros, subnormals, the smallest normal, ordinary values and 1e300 (of one sign: the contract's bound on a mean
        # is relative to the sum of the |values|)
        pool = np.array([0.0, -0.0, 5e-324, -3e-310, 2.2250738585072014e-308, 1.0, -2.5, 1e-5, 1e300, 1e300 * (1 + 2.0 ** -50)])
        x = pool[rng.integers(0, pool.size, size=(G, C_CELLS))]
        x[0, cells[0]] = 1e300
    x = np.asfortranarray(x)
    x.setflags(write=False)
    _cases[key] = (x, cells, zr.zscore_gene_filter(x, cells))
    return _cases[key]


def to_dev(x):
    return torch.from_numpy(np.array(x.T, order="C")).cuda()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_ref", N_REFS)
@pytest.mark.parametrize("G", GENES)
def test_zscore_filter_matches_exact_restatement(dev, G, n_ref, kind):
    x, cells, (mean, sd, row_mean) = case(G, n_ref, kind)
    got_mean, got_sd, got_rows = dev.zscore_gene_filter(to_dev(x), cells)
    got_rows = got_rows.cpu().numpy()
    print(f"G={G} n_ref={n_ref} {kind}: mean {got_mean!r} / {mean!r}  sd {got_sd!r} / {sd!r}  "
          f"row means differing: {int((bits(got_rows) != bits(row_mean)).sum() - (np.isnan(got_rows) & np.isnan(row_mean)).sum())}")
    assert same_bits(got_mean, mean)
    assert same_bits(got_sd, sd)
    if G * n_ref < 2:
        assert got_sd != got_sd and np.isnan(got_rows).all()      # R's sd of one value
    both_nan = np.isnan(got_rows) & np.isnan(row_mean)
    assert np.array_equal(bits(got_rows)[~both_nan], bits(row_mean)[~both_nan])
    if kind == "edge":
        assert np.isfinite(got_sd) or G * n_ref < 2               # 1e300 squared leaves the double range; the sd does not


def test_zscore_filter_padded_rows_and_repeated_cells(dev):
    """Rows that lie further apart than G (the padding holds NaN and is never read), and a cell listed twice counts twice."""
    x, _, _ = case(65, 33, "expr")
    cells = np.array([9, 3, 9, 31, 0], dtype=np.int32)
    want = zr.zscore_gene_filter(x, cells)
    full = torch.full((C_CELLS, 65 + 7), float("nan"), dtype=torch.float64, device="cuda")
    full[:, :65] = to_dev(x)
    mean, sd, rows = dev.zscore_gene_filter(full[:, :65], cells)
    assert same_bits(mean, want[0]) and same_bits(sd, want[1])
    assert np.array_equal(bits(rows.cpu().numpy()), bits(want[2]))


def test_zscore_filter_planted_genes_and_kept_set(dev):
    """The planted genes fall on their sides of 0.8, and a resident object keeps the genes the host object keeps.  The host
    route's row means differ from the device's by at most an ulp, so the sets agree whenever no host row mean lies within
    1e-9 of 0.8: asserted on the data, which were made to meet it."""
    for G, n_ref in [(63, 2), (65, 33), (257, 33)]:
        x, cells, (_, _, row_mean) = case(G, n_ref, "expr")
        host_rows = host_row_means(x, cells)
        assert np.abs(host_rows - 0.8).min() >= 1e-9
        assert 0.8 < host_rows[7] < 0.8 * (1 + 1e-7) and 0.8 * (1 - 1e-7) < host_rows[40] < 0.8
        assert row_mean[7] >= 0.8 > row_mean[40]
        obj = InfercnvObject(np.array(x), GeneOrder(np.array(["chr1"] * G)),
                             reference_grouped_cell_indices={"a": cells[: max(1, n_ref // 2)], "b": cells[max(1, n_ref // 2):]},
                             observation_grouped_cell_indices={"t": np.setdiff1d(np.arange(C_CELLS), cells).astype(np.int32)})
        res = obj.to_device()
        DeviceMatrix.stats(reset=True)
        kept_host, kept_dev = ts.zscore_kept_genes(obj), ts.zscore_kept_genes(res)
        assert DeviceMatrix.stats()["fetches"] == 0
        assert np.array_equal(kept_host, kept_dev)
        assert 7 not in kept_dev and 40 in kept_dev
        assert np.array_equal(ts.zscore_outlier_genes(res), np.flatnonzero(row_mean >= 0.8))


def test_zscore_filter_refusals_leave_the_outputs_alone(dev):
    L = _lib.load()
    x = torch.ones((C_CELLS, 65), dtype=torch.float64, device="cuda")
    rows = torch.full((65,), 7.0, dtype=torch.float64, device="cuda")
    out = (ct.c_double * 2)(7.0, 7.0)
    good = np.array([3, 1, 2], dtype=np.int32)
    ip = lambda a: a.ctypes.data_as(ct.POINTER(ct.c_int32))
    xp, rp, null = ct.c_void_p(x.data_ptr()), ct.c_void_p(rows.data_ptr()), ct.c_void_p(0)
    stream = ct.c_void_p(torch.cuda.current_stream().cuda_stream)
    calls = {
        "null matrix": (null, 65, 65, C_CELLS, ip(good), 3, out, rp),
        "null list": (xp, 65, 65, C_CELLS, None, 3, out, rp),
        "null mean_sd": (xp, 65, 65, C_CELLS, ip(good), 3, None, rp),
        "null row_mean": (xp, 65, 65, C_CELLS, ip(good), 3, out, null),
        "no reference cell": (xp, 65, 65, C_CELLS, ip(good), 0, out, rp),
        "negative count": (xp, 65, 65, C_CELLS, ip(good), -1, out, rp),
        "negative index": (xp, 65, 65, C_CELLS, ip(np.array([3, -1, 2], dtype=np.int32)), 3, out, rp),
        "index == C": (xp, 65, 65, C_CELLS, ip(np.array([3, 1, C_CELLS], dtype=np.int32)), 3, out, rp),
        "no gene": (xp, 65, 0, C_CELLS, ip(good), 3, out, rp),
        "no cell": (xp, 65, 65, 0, ip(good), 3, out, rp),
        "ld < G": (xp, 64, 65, C_CELLS, ip(good), 3, out, rp),
    }
    for what, args in calls.items():
        assert L.icnv_zscore_gene_filter_dev(*args, stream) == _lib.ERR_ARG, what
        assert L.icnv_last_error().decode().startswith("zscore_gene_filter:"), what
    torch.cuda.synchronize()
    assert out[0] == 7.0 and out[1] == 7.0 and bool((rows == 7.0).all())
    with pytest.raises(_lib.IcnvError):
        dev.zscore_gene_filter(x, np.array([C_CELLS], dtype=np.int32))
    with pytest.raises(TypeError):
        dev.zscore_gene_filter(x.cpu(), good)
    # and the same arguments made good run
    mean, sd, rows = dev.zscore_gene_filter(x, good)
    assert mean == 1.0 and sd == 0.0 and bool(torch.isnan(rows).all())   # a constant matrix: 0 / 0 in every z


# ---------------------------------------------------------------- run() on a resident object against run() on its host copy
HOST_MATRIX_ENTRIES = ("icnv_smooth_chain", "icnv_viterbi_cells", "icnv_viterbi_groups", "icnv_select_genes", "icnv_scale_genes",
                       "icnv_remove_outliers", "icnv_normalize_log2", "icnv_gene_stats", "icnv_average_bounds", "icnv_median_filter",
                       "icnv_median_filter_na", "icnv_ingest_counts", "icnv_smooth_windows", "icnv_block_mean_sd", "icnv_cells_mean_sd",
                       "icnv_gather_values", "icnv_state_consensus", "icnv_states_to_proxy", "icnv_cnv_runs", "icnv_matrix_sum")


class _Recording:
    """A stand-in for the handle of _lib.load() that notes the name of every entry that is looked up."""

    def __init__(self, real, names):
        self._real, self._names = real, names

    def __getattr__(self, name):
        self._names.append(name)
        return getattr(self._real, name)


@contextlib.contextmanager
def no_crossing(G, C, allow=()):
    """Nothing of the matrix's size crosses while the body runs: no DeviceMatrix upload or fetch, no host-buffer matrix entry
    of the library, and no torch.from_numpy / Tensor.cpu of a float64 array of G * C elements or more or of any array of the
    matrix's shape (the text of the files and the pixels of the plots are products of the run, not the matrix).  allow: shapes
    a caller names and explains."""
    seen, names = [], []

    def matrix_sized(shape, dtype):
        n = int(np.prod(shape)) if len(shape) else 1
        if tuple(shape) in allow:
            return False
        return (n >= G * C and "float64" in str(dtype)) or tuple(shape) in ((C, G), (G, C))

    real_from_numpy, real_cpu, real_handle = torch.from_numpy, torch.Tensor.cpu, _lib.load()

    def from_numpy(a):
        if matrix_sized(a.shape, a.dtype):
            seen.append(("from_numpy", tuple(a.shape), str(a.dtype)))
        return real_from_numpy(a)

    def cpu(t, *args, **kwargs):
        if t.is_cuda and matrix_sized(tuple(t.shape), t.dtype):
            seen.append(("cpu", tuple(t.shape), str(t.dtype)))
        return real_cpu(t, *args, **kwargs)

    DeviceMatrix.stats(reset=True)
    torch.from_numpy, torch.Tensor.cpu, _lib._lib = from_numpy, cpu, _Recording(real_handle, names)
    try:
        yield
    finally:
        torch.from_numpy, torch.Tensor.cpu, _lib._lib = real_from_numpy, real_cpu, real_handle
    stats = DeviceMatrix.stats()
    assert stats["fetches"] == 0 and stats["uploads"] == 0, stats
    assert not seen, seen
    host_entries = sorted(set(n for n in names if n in HOST_MATRIX_ENTRIES))
    assert not host_entries, host_entries
    assert any(n.endswith("_dev") for n in names)


class Hook:
    def __init__(self, *more):
        self.seen, self.more = {}, more

    def __call__(self, step, label, obj):
        self.seen[step] = obj
        for h in self.more:
            h(step, label, obj)


def tree_bytes(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def same_matrix(res, host, what):
    """A resident matrix against the host route's array: the same shape and the same bits (NaN payloads included)."""
    assert isinstance(res, DeviceMatrix), (what, type(res))
    got = res.to_host()
    host = np.asarray(host, dtype=np.float64)
    assert got.shape == host.shape, what
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(host).view(np.uint64)), what


def compare_objects(res, host, what):
    from infercnv_amd import bayes_net
    if isinstance(host, bayes_net.MCMCInferCNV):
        assert list(res.cnv_regions) == list(host.cnv_regions), what
        assert np.array_equal(bits(res.cnv_means), bits(host.cnv_means)), what
        return
    same_matrix(res.expr_data, host.expr_data, what)
    assert (res.hspike is None) == (host.hspike is None), what
    if host.hspike is not None:
        same_matrix(res.hspike.expr_data, host.hspike.expr_data, what + " hspike")
    assert list(res.genes()) == list(host.genes()) and list(res.cells()) == list(host.cells()), what
    if host.tumor_subclusters is not None:
        hs, rs = host.tumor_subclusters["subclusters"], res.tumor_subclusters["subclusters"]
        assert list(hs) == list(rs), what
        for g in hs:
            assert list(hs[g]) == list(rs[g]), what
            for name in hs[g]:
                assert np.array_equal(np.asarray(hs[g][name]), np.asarray(rs[g][name])), (what, g, name)


def run_both(make_obj, tmp_path, hooked, checkpoints=False, allow=(), **kw):
    """run() on the object and on its resident form, same arguments: the returned objects, every object an on_step hook saw
    and every file written under out_dir are compared bit for bit and byte for byte.  Both runs write into the SAME out_dir,
    one after the other (the path is one of the options an object carries into its .rds).  Returns ({form: result}, the host
    run's files, {form: hook})."""
    import shutil
    from infercnv_amd import pipeline, run
    outs, hooks, results = {}, {}, {}
    out = tmp_path / "out"
    for form in ("host", "resident"):
        if out.exists():
            shutil.rmtree(out)
        obj = make_obj()
        hook = None
        if hooked:
            hook = Hook(*([pipeline.rds_checkpoints(str(out), "all", **kw)] if checkpoints else []))
            os.makedirs(out, exist_ok=True)
        if form == "resident":
            obj = obj.to_device()                           # the one upload, before the watch begins
            G, C = results["host"].expr_data.shape
            with no_crossing(G, C, allow):
                results[form] = run(obj, out_dir=str(out), on_step=hook, **kw)
        else:
            results[form] = run(obj, out_dir=str(out), on_step=hook, **kw)
        outs[form], hooks[form] = tree_bytes(out), hook
    assert results["resident"].is_resident()
    compare_objects(results["resident"], results["host"], "returned object")
    if hooked:
        assert list(hooks["host"].seen) == list(hooks["resident"].seen)
        for step, o in hooks["host"].seen.items():
            compare_objects(hooks["resident"].seen[step], o, f"step {step}")
    assert sorted(outs["host"]) == sorted(outs["resident"])
    for name, data in outs["host"].items():
        assert outs["resident"][name] == data, name
    return results, outs["host"], hooks


@pytest.fixture(scope="module")
def example(golden_dir):
    d = np.load(os.path.join(golden_dir, "infercnv_object_example.npz"))
    return {k: d[k] for k in d.files}


def example_obj(ex, permute=False):
    chr_names = ex["chr_levels"][ex["chr_codes"] - ex["chr_codes"].min()]
    # (expr.data is a double matrix in R and in a DeviceMatrix: the integer counts of the file are handed over as doubles, so that
    # the object of step 1 is saved as the same R type from both forms)
    counts, start, stop = ex["count_data"].astype(np.float64), ex["gene_start"], ex["gene_stop"]
    if permute:                                             # the chromosomes' genes interleaved: chr_layout() has work to do
        p = np.random.default_rng(5).permutation(counts.shape[0])
        counts, chr_names, start, stop = counts[p], chr_names[p], start[p], stop[p]
    return InfercnvObject(expr_data=counts, count_data=counts.copy(), gene_order=GeneOrder(chr_names, start, stop),
                          reference_grouped_cell_indices={"normal": ex["ref_normal"]},
                          observation_grouped_cell_indices={"tumor": ex["obs_tumor"]})


@pytest.fixture(scope="module")
def run_inputs(golden_dir):
    d = np.load(os.path.join(golden_dir, "example_run_inputs.npz"))
    x = d["mant"].astype(np.float64) / 10.0 ** d["neg_exp"].astype(np.float64)
    refs = {str(n): d[f"ref_{i}"] for i, n in enumerate(d["ref_names"])}
    obs = {str(n): d[f"obs_{i}"] for i, n in enumerate(d["obs_names"])}
    return {"counts": x, "chr": d["chr_levels"][d["chr_codes"]], "refs": refs, "obs": obs}


def inputs_obj(ri):
    return InfercnvObject(expr_data=ri["counts"], count_data=ri["counts"], gene_order=GeneOrder(chr=ri["chr"]),
                          reference_grouped_cell_indices=ri["refs"], observation_grouped_cell_indices=ri["obs"])


def test_run_example_fused_route_with_plots(dev, example, tmp_path):
    """The golden example through the fused ingest and the fused chain (no hook), denoised, with both plots' PNGs and matrix
    files.  On the parent commit the resident run stops at DeviceMatrix.__array__."""
    _, files, _ = run_both(lambda: example_obj(example), tmp_path, hooked=False, cutoff=1, cluster_by_groups=True, denoise=True,
                        HMM=False, write_expr_matrix=True)
    assert "infercnv.heatmap.png" in files and "infercnv.preliminary.heatmap.png" in files and "infercnv.observations.txt" in files


def test_run_example_on_step_route_with_checkpoints(dev, example, tmp_path):
    """The step-by-step route: every step's object, and rds_checkpoints saving them from the device, byte for byte."""
    _, files, _ = run_both(lambda: example_obj(example), tmp_path, hooked=True, checkpoints=True, cutoff=1, cluster_by_groups=True,
                        denoise=True, HMM=False, no_plot=True, prune_outliers=True, scale_data=True)
    assert "run.final.infercnv_obj" in files and "14_invert_log_transform.infercnv_obj" in files


def test_run_example_permuted_gene_order(dev, example, tmp_path):
    obj = example_obj(example, permute=True)
    assert obj.chr_layout()[0] is not None
    run_both(lambda: example_obj(example, permute=True), tmp_path, hooked=True, cutoff=1, cluster_by_groups=True, denoise=True,
             HMM=True, HMM_type="i3", analysis_mode="samples", BayesMaxPNormal=0, no_plot=True, seed=3)


def test_run_inputs_i6_samples_with_bayes(dev, run_inputs, tmp_path):
    """The i6 HMM on whole samples with the hidden spike-in, the Bayesian filter, the reports and the HMM plots."""
    _, files, _ = run_both(lambda: inputs_obj(run_inputs), tmp_path, hooked=True, cutoff=1, HMM=True, HMM_type="i6",
                        analysis_mode="samples", denoise=True, sd_amplifier=2, BayesMaxPNormal=0.5, seed=7, no_prelim_plot=True)
    assert any(f.startswith("HMM_CNV_predictions.") and f.endswith("pred_cnv_genes.dat") for f in files)
    assert any(f.startswith("17_HMM_pred") and f.endswith("pred_cnv_regions.dat") for f in files)


@pytest.mark.parametrize("method", ["leiden", "random_trees"])
def test_run_inputs_i3_subclusters(dev, run_inputs, tmp_path, method):
    """The i3 HMM on tumor subclusters by both partition methods; then add_to_seurat's device pass on the resident result and
    its resident state object against the host pair."""
    from infercnv_amd import seurat_interaction
    results, _, hooks = run_both(lambda: inputs_obj(run_inputs), tmp_path, hooked=True, cutoff=1, HMM=True, HMM_type="i3",
                                 analysis_mode="subclusters", tumor_subcluster_partition_method=method, leiden_method="simple",
                                 k_nn=10, BayesMaxPNormal=0, no_plot=True, seed=7)
    assert hooks["resident"].seen[17].expr_data.kind == "states"
    want = seurat_interaction.device_pass(results["host"], hooks["host"].seen[17], "i3")
    G, C = results["host"].expr_data.shape
    with no_crossing(G, C):
        got = seurat_interaction.device_pass(results["resident"], hooks["resident"].seen[17], "i3")
    for a, b in zip(got[1:], want[1:]):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert [n for n, _ in got[0]] == [n for n, _ in want[0]]


def test_run_inputs_leiden_pca_fused(dev, run_inputs, tmp_path):
    """The default Leiden route (PCA) with the z-score gene filter of step 15 on the device, no hook, no HMM.  The route's
    2000 x 2000 Gram matrices go to numpy.linalg.eigh by design (DESIGN K18), on both forms alike; with 184 cells they happen to
    hold more elements than the expression matrix, so their shape is named here."""
    run_both(lambda: inputs_obj(run_inputs), tmp_path, hooked=False, allow=((2000, 2000),), cutoff=1, HMM=False,
             analysis_mode="subclusters", no_plot=True, seed=7)


def test_run_inputs_cells_mode(dev, run_inputs, tmp_path):
    run_both(lambda: inputs_obj(run_inputs), tmp_path, hooked=True, cutoff=1, HMM=True, HMM_type="i6", analysis_mode="cells",
             BayesMaxPNormal=0.5, no_plot=True, seed=7)


def test_save_and_post_run_entries(dev, example, tmp_path):
    """save_infercnv_obj and apply_median_filtering on a resident object against its host copy.  A plain file is the same
    bytes.  With compress=True a CUDA tensor of any size is deflated on the device in pieces (DESIGN K28), a host array
    below the writer's device threshold by zlib on the host, as before this type existed: two valid gzip streams of the same
    bytes, compared inflated."""
    import gzip
    from infercnv_amd import noise_reduction, rds, run
    host = run(example_obj(example), out_dir=str(tmp_path / "o"), cutoff=1, HMM=False, no_plot=True, up_to_step=15)
    res = host.to_device()
    G, C = host.expr_data.shape
    for compress in (False, True):
        with no_crossing(G, C):
            rds.save_infercnv_obj(res, str(tmp_path / f"res{compress}.rds"), compress=compress)
        rds.save_infercnv_obj(host, str(tmp_path / f"host{compress}.rds"), compress=compress)
        got, want = (tmp_path / f"res{compress}.rds").read_bytes(), (tmp_path / f"host{compress}.rds").read_bytes()
        assert (gzip.decompress(got) == gzip.decompress(want)) if compress else (got == want)
    with no_crossing(G, C):
        filtered = noise_reduction.apply_median_filtering(res)
    same_matrix(filtered.expr_data, noise_reduction.apply_median_filtering(host).expr_data, "apply_median_filtering")
