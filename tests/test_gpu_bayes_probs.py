"""The probability heatmaps and tables of the Bayesian filter on the GPU (icnv_paint_regions_dev, icnv_theta_box_dev, DESIGN
K33): the paint and the box statistics bit-equal to the sequential restatement of tests/bayes_probs_restate.py; then
bayes_net.postProbNormal, kept_regions and plotProbabilities on the planted object of test_gpu_bayes.py, both routes, and run()
with pipeline.bayes_probabilities_hook on example/run.R's 184 cells, host and resident."""
import ctypes as ct
import functools
import os

import numpy as np
import pytest

import bayes_probs_restate as pr
import table_text_restate as tt
from test_gpu_bayes import MU6, TAU6, planted_object, same

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = -7.5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infercnv_amd import device
    torch.cuda.set_device(0)
    device.init(0)
    return device


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


# ---- the paint --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def paint_case(G, C):
    """Regions that are a whole row, one gene, empty (no genes; no cells), ending on the last gene, a cell listed by two
    overlapping regions and twice by one (the later value must win: -0.0 and NaN among the values, and a later value smaller
    than an earlier one), then seeded random rectangles with unsorted cell lists.  -> the region arrays and the restated matrix."""
    rng = np.random.default_rng(1000 * G + C)
    regs = [(0, G, list(range(C)), 0.75),
            (G // 2, 1, [0], -0.0),
            (G, 0, list(range(C)), 9.0),
            (0, G, [], 8.0),
            (max(0, G - 3), min(3, G), [C - 1, 0], float("nan")),
            (max(0, G - 2), min(2, G), [C - 1, C - 1], 0.5),
            (0, 1, [C // 2], 0.25)]
    for _ in range(12):
        g0 = int(rng.integers(0, G))
        ng = int(rng.integers(1, G - g0 + 1))
        cells = rng.choice(C, size=int(rng.integers(1, C + 1)), replace=False)
        regs.append((g0, ng, [int(c) for c in cells], float(rng.choice([0.125, 0.5, 1.0 - 2.0 ** -53, 1e-300, 0.75]))))
    g0 = np.array([r[0] for r in regs], dtype=np.int32)
    ng = np.array([r[1] for r in regs], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum([len(r[2]) for r in regs])]).astype(np.int64)
    idx = np.array([c for r in regs for c in r[2]], dtype=np.int32)
    val = np.array([r[3] for r in regs], dtype=np.float64)
    assert pr.paint_refusal(G, C, g0, ng, off, idx) is None
    want = pr.paint(G, C, g0, ng, off, idx, val)
    want.setflags(write=False)
    return (g0, ng, off, idx, val), want


def padded(C, G, pad):
    full = torch.full((C, G + pad), SENTINEL, dtype=torch.float64, device="cuda")
    return full, full[:, :G]


@pytest.mark.parametrize("C", [1, 3, 40])
@pytest.mark.parametrize("G", [1, 63, 64, 65, 257])
def test_paint_bit_equal_to_the_restatement(dev, G, C):
    arrays, want = paint_case(G, C)
    for pad in (0, 5):
        full, out = padded(C, G, pad)
        assert dev.paint_regions(out, *arrays) is out
        got = full.cpu().numpy()
        assert np.array_equal(bits(got[:, :G]), bits(want)), (G, C, pad)
        assert (got[:, G:] == SENTINEL).all()                                       # the padding columns are not touched
    as_tensors = [torch.from_numpy(a).cuda() for a in arrays]                        # the arrays may live on the device already
    full, out = padded(C, G, 0)
    dev.paint_regions(out, *as_tensors)
    assert np.array_equal(bits(out.cpu().numpy()), bits(want))


def test_paint_no_regions_gives_the_zero_matrix(dev):
    full, out = padded(3, 65, 5)
    e32, e64 = np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.int64)
    dev.paint_regions(out, e32, e32, e64, e32, np.zeros(0))
    got = full.cpu().numpy()
    assert np.array_equal(bits(got[:, :65]), np.zeros((3, 65), dtype=np.uint64)) and (got[:, 65:] == SENTINEL).all()
    full, out = padded(3, 65, 0)                                                     # regions, none of which paints
    dev.paint_regions(out, np.array([0, 65], dtype=np.int32), np.array([65, 0], dtype=np.int32), np.array([0, 0, 2]),
                      np.array([0, 1], dtype=np.int32), np.array([1.0, 2.0]))
    assert np.array_equal(bits(out.cpu().numpy()), np.zeros((3, 65), dtype=np.uint64))


def test_paint_five_thousand_one_cell_runs(dev):
    """The per-cell route's shape (K25): every region is one cell, cell_off = 0, 1, 2, ..; runs of one cell overlap."""
    G, C, R = 300, 700, 5000
    rng = np.random.default_rng(25)
    g0 = rng.integers(0, G - 1, size=R).astype(np.int32)
    ng = np.minimum(rng.integers(1, 40, size=R), G - g0).astype(np.int32)
    idx = rng.integers(0, C, size=R).astype(np.int32)
    off = np.arange(R + 1, dtype=np.int64)
    val = rng.random(R)
    want = pr.paint(G, C, g0, ng, off, idx, val)
    hits = np.zeros((C, G), dtype=np.int32)
    for r in range(R):
        hits[idx[r], g0[r]:g0[r] + ng[r]] += 1
    assert (hits > 1).sum() > 1000                                                   # the order of the regions matters here
    out = torch.full((C, G), SENTINEL, dtype=torch.float64, device="cuda")
    dev.paint_regions(out, g0, ng, off, idx, val)
    assert np.array_equal(bits(out.cpu().numpy()), bits(want))


def test_paint_refusals_leave_every_sentinel(dev):
    from infercnv_amd import _lib
    G, C = 65, 3
    good = (np.array([1, 0], dtype=np.int32), np.array([3, 65], dtype=np.int32), np.array([0, 2, 3], dtype=np.int64),
            np.array([0, 2, 1], dtype=np.int32), np.array([0.5, 0.25]))
    cases = {"a gene run past G": (np.array([63, 0], dtype=np.int32), good[1], good[2], good[3], good[4]),
             "a cell >= C": (good[0], good[1], good[2], np.array([0, 3, 1], dtype=np.int32), good[4]),
             "a negative cell": (good[0], good[1], good[2], np.array([0, -1, 1], dtype=np.int32), good[4]),
             "a non-monotone cell_off": (good[0], good[1], np.array([0, 2, 1], dtype=np.int64), good[3], good[4]),
             "cell_off[n] > n_idx": (good[0], good[1], np.array([0, 2, 4], dtype=np.int64), good[3], good[4]),
             "cell_off[0] != 0": (good[0], good[1], np.array([1, 2, 3], dtype=np.int64), good[3], good[4]),
             "a negative gene count": (good[0], np.array([3, -1], dtype=np.int32), good[2], good[3], good[4])}
    for what, arrays in cases.items():
        assert pr.paint_refusal(G, C, *arrays[:4]) == "ARG", what
        full, out = padded(C, G, 5)
        with pytest.raises(ValueError):
            dev.paint_regions(out, *arrays)
        torch.cuda.synchronize()
        assert bool((full == SENTINEL).all()), what
        t = [torch.from_numpy(a).cuda() for a in arrays]
        rc = _lib.load().icnv_paint_regions_dev(ct.c_void_p(out.data_ptr()), G, C, G + 5, 2, *(ct.c_void_p(x.data_ptr()) for x in t[:4]),
                                                3, ct.c_void_p(t[4].data_ptr()), None)
        torch.cuda.synchronize()
        assert rc == _lib.ERR_ARG and bool((full == SENTINEL).all()), what
    full, out = padded(C, G, 5)
    dev.paint_regions(out, *good)                                                    # and the good arrays paint
    assert np.array_equal(bits(out.cpu().numpy()), bits(pr.paint(G, C, *good)))
    with pytest.raises(ValueError):
        dev.paint_regions(out, good[0], good[1][:1], good[2], good[3], good[4])
    with pytest.raises(TypeError):
        dev.paint_regions(out.to(torch.float32), *good)


# ---- the box statistics -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def box_case(m, n, K):
    s = pr.make_box_samples(5, m, n, K, seed=100 * K + n)
    s.setflags(write=False)
    want = pr.theta_box(s)
    want.setflags(write=False)
    return s, want


def gpu_box(dev, s):
    return dev.theta_box(torch.from_numpy(np.array(s)).cuda()).cpu().numpy()


# one draw per chain, both parities, a sort length that is no power of two, the default schedule, and the 8 192 limit at K = 8
@pytest.mark.parametrize("K,n_keep", [(K, n) for K in (2, 3, 6, 8) for n in (1, 20, 21, 100, 1000)] + [(8, 1024)])
def test_box_bit_equal_to_the_restatement(dev, K, n_keep):
    s, want = box_case(K, n_keep, K)
    for R in (1, 2, 5):
        got = gpu_box(dev, s[:R])
        same(got, want[:R])
        assert not np.signbit(got[got == 0.0]).any()                                 # -0.0 is reported as +0.0
    assert np.isnan(want[2]).all()                                                   # the region without cells
    if K * n_keep >= 16:
        lo, hi = pr.fences(s[0, :, :, 0])
        assert want[0, 0, 0] <= lo and want[0, 0, 4] >= hi                           # the draws ON the fences are whisker ends
        assert (want[0, 0, 0] == lo or want[0, 0, 5] == 0) and want[0, 1, 5] >= 2 and want[0, 1, 6] >= 1
        assert (want[1, 0] == [0.25] * 5 + [0.0, 0.0]).all()                         # the constant series
        assert set(want[1, 1, :5]) <= {-1.0, 0.0, 0.5, 1.0}                          # the tied values


@pytest.mark.parametrize("m,n,K", [(2, 4096, 8), (8, 37, 2), (4, 5, 5)])
def test_box_chain_count_is_its_own_parameter(dev, m, n, K):
    s, want = box_case(m, n, K)
    same(gpu_box(dev, s[:2]), want[:2])


def test_box_no_regions_and_refusals(dev):
    from infercnv_amd import _lib
    L = _lib.load()
    assert tuple(dev.theta_box(torch.zeros((0, 6, 100, 6), dtype=torch.float64, device="cuda")).shape) == (0, 6, 7)
    for shape, code in (((1, 8, 1025, 3), _lib.ERR_UNSUPPORTED), ((1, 3, 20, 9), _lib.ERR_ARG), ((1, 9, 20, 3), _lib.ERR_ARG),
                        ((1, 6, 20, 1), _lib.ERR_ARG)):
        R, m, n, K = shape
        assert pr.box_refusal(R, m, n, K) == ("ARG" if code == _lib.ERR_ARG else "UNSUPPORTED")
        t = torch.zeros(shape, dtype=torch.float64, device="cuda")
        with pytest.raises(_lib.IcnvError) as e:
            dev.theta_box(t)
        assert e.value.code == code
        box = torch.full((R, K, 7), 7.0, dtype=torch.float64, device="cuda")
        assert L.icnv_theta_box_dev(ct.c_void_p(t.data_ptr()), R, m, n, K, ct.c_void_p(box.data_ptr()), None) == code
        torch.cuda.synchronize()
        assert bool((box == 7.0).all())                                              # nothing ran
    with pytest.raises(TypeError):
        dev.theta_box(torch.zeros((1, 3, 20), dtype=torch.float64, device="cuda"))


# ---- bayes_net on the planted object ----------------------------------------------------------------------------------
SCHED = dict(n_adapt=10, n_burn=5, n_keep=30)
ROUTES = ("dict", "table")


@functools.lru_cache(maxsize=None)
def planted(route, keep_samples=False, reassign=True):
    """The planted object with two of its three regions cut in two by a neutral gap (five regions), through the sampler."""
    from infercnv_amd import bayes_net
    obj, states, _ = planted_object()
    states = states.copy()
    states[30:34, 20:] = 3
    states[150:152, 20:] = 3
    m = bayes_net.inferCNVBayesNet(obj, states, "i6", by="consensus", seed=4, mu=MU6, sig=TAU6, route=route, keep_samples=keep_samples,
                                   reassignCNVs=reassign, **SCHED)
    assert len(m.cnv_regions) == 5
    return m, states


def test_box_of_the_samplers_own_samples(dev):
    m, _ = planted("dict", keep_samples=True)
    samples = np.stack([np.asarray(m.cnv_probabilities[r]).reshape(6, SCHED["n_keep"], 6) for r in range(3)])
    same(gpu_box(dev, samples), pr.theta_box(samples))


def restated_matrix(m):
    from infercnv_amd import bayes_net
    G, C = m.infercnv_obj.expr_data.shape
    return pr.paint(G, C, *bayes_net._region_arrays(m), 1.0 - m.cnv_means[2]).T


def tree(root):
    return {f: open(os.path.join(root, f), "rb").read() for f in sorted(os.listdir(root))}


@pytest.mark.parametrize("route", ROUTES)
def test_post_prob_normal_equals_plot_cnv_of_the_restated_matrix(dev, tmp_path, route):
    from infercnv_amd import bayes_net, heatmap
    m, _ = planted(route)
    x = bayes_net.normal_probability_matrix(m)
    want = restated_matrix(m)
    assert x.is_cuda and np.array_equal(bits(x.cpu().numpy().T), bits(want)) and 0 < (want != 0).mean() < 1
    title, name = " (1 - Probabilities of Normal) Before Filtering", "infercnv.NormalProbabilities.PreFiltering"
    bayes_net.postProbNormal(m, title, name, out_dir=str(tmp_path / "got"), useRaster=True)
    host = m.infercnv_obj.copy()
    host.expr_data = want
    heatmap.plot_cnv(host, out_dir=str(tmp_path / "want"), k_obs_groups=1, cluster_by_groups=True, title=title, output_filename=name,
                     write_expr_matrix=False, x_center=0, x_range=(0, 1), useRaster=True)
    got, ref = tree(tmp_path / "got"), tree(tmp_path / "want")
    assert list(got) == list(ref) and {name + ".heatmap.png", name + ".heatmap_layout.json", name + ".heatmap_thresholds.txt",
                                       name + ".observation_groupings.txt"} <= set(got)
    for f in ref:
        assert got[f] == ref[f], f
    import copy
    quiet = copy.copy(m)
    quiet.args = dict(m.args, no_plot=True, out_dir=str(tmp_path / "quiet"))
    assert bayes_net.postProbNormal(quiet, title, name) is None and not os.path.exists(tmp_path / "quiet")
    loud = copy.copy(m)
    loud.args = dict(m.args, out_dir=str(tmp_path / "own"))                          # out_dir defaults to the object's
    bayes_net.postProbNormal(loud, title, name)
    assert tree(tmp_path / "own") == ref


def same_object(a, b):
    assert list(a.cnv_regions) == list(b.cnv_regions) and a.args == b.args and len(a.cell_gene) == len(b.cell_gene)
    assert np.array_equal(bits(a.cnv_means), bits(b.cnv_means))
    for i in range(len(b.cell_gene)):
        x, y = a.cell_gene[i], b.cell_gene[i]
        assert x["cnv_regions"] == y["cnv_regions"] and x["State"] == y["State"]
        assert np.array_equal(x["Genes"], y["Genes"]) and np.array_equal(x["Cells"], y["Cells"])
        assert np.array_equal(bits(a.cell_probabilities[i]), bits(b.cell_probabilities[i]))
    assert (a.table is None) == (b.table is None)
    if b.table is not None:
        for f in ("col", "chr", "gene_first", "gene_count", "row_first", "state", "ordinal", "token", "cell_off", "cell_idx"):
            assert np.array_equal(getattr(a.table, f), getattr(b.table, f)), f
        assert np.array_equal(bits(a.cell_prob_rows), bits(b.cell_prob_rows))


@pytest.mark.parametrize("reassign", [True, False])
@pytest.mark.parametrize("route", ROUTES)
def test_kept_regions_is_the_filters_object(dev, tmp_path, route, reassign):
    import copy
    from infercnv_amd import bayes_net
    m, states = planted(route, reassign=reassign)
    m = copy.copy(m)
    m.args = dict(m.args, out_dir=str(tmp_path / "bayes"))
    kept = bayes_net.kept_regions(m, 0.5)
    assert not os.path.exists(tmp_path / "bayes")                                    # nothing is written
    f, _ = bayes_net.filterHighPNormals(m, states, 0.5)
    assert 0 < len(f.cnv_regions) < 5 and len(m.cnv_regions) == 5
    same_object(kept, f)
    if reassign:
        assert [cg["State"] for cg in kept.cell_gene] != [m.cell_gene[list(m.cnv_regions).index(n)]["State"] for n in kept.cnv_regions]
    same_object(bayes_net.kept_regions(m, 2.0), bayes_net.filterHighPNormals(m, states, 2.0)[0])     # nothing is removed


def expected_tables(m, box):
    names = list(m.cnv_regions)
    rows, mat = pr.cnv_table(names, box)
    cnv = tt.file_bytes(mat.T, "cell_rows", list(range(len(rows))), rows, pr.BOX_FIELDS, quoted=False, sep="\t")
    rows, mat, cols = pr.cell_table(names, [m.cell_gene[r]["Cells"] for r in range(len(names))],
                                    [m.cell_probabilities[r] for r in range(len(names))], m.infercnv_obj.cells())
    return cnv, tt.file_bytes(mat.T, "cell_rows", list(range(len(rows))), rows, cols, quoted=False, sep="\t")


@pytest.mark.parametrize("route", ROUTES)
def test_plot_probabilities_whatever_the_batching(dev, tmp_path, route):
    from infercnv_amd import bayes_net
    m, states = planted(route)
    held, _ = planted(route, keep_samples=True)
    samples = np.stack([np.asarray(held.cnv_probabilities[r]).reshape(6, SCHED["n_keep"], 6) for r in range(5)])
    want_box = pr.theta_box(samples)
    per_region = 6 * SCHED["n_keep"] * 6 * 8
    one = bayes_net.plotProbabilities(m, str(tmp_path / "one"))
    for regions_per_batch in (1, 3):
        p = bayes_net.plotProbabilities(m, max_sample_bytes=regions_per_batch * per_region + 8)
        same(p.box, want_box)
        assert np.array_equal(bits(p.cell_probs), bits(one.cell_probs)) and list(p.regions) == list(m.cnv_regions)
    same(one.box, want_box)
    assert np.array_equal(one.cell_off, np.arange(6) * 200) and one.cell_probs.shape == (1000, 6)
    dev.bayes_stats(reset=True)
    p = bayes_net.plotProbabilities(held, str(tmp_path / "held"), max_sample_bytes=1)      # the held samples, one region a batch
    assert dev.bayes_stats()["calls"] == 0                                           # not sampled again
    same(p.box, want_box)
    bayes_net.plotProbabilities(m, str(tmp_path / "device"), device_rows=1)          # the route of a per-cell table
    cnv, cell = expected_tables(m, want_box)
    for sub in ("one", "held", "device"):
        assert sorted(os.listdir(tmp_path / sub)) == ["cellProbs.0.dat", "cnvProbs.0.dat"]       # BayesMaxPNormal is 0 before the filter
        assert open(tmp_path / sub / "cnvProbs.0.dat", "rb").read() == cnv, sub
        assert open(tmp_path / sub / "cellProbs.0.dat", "rb").read() == cell, sub
    kept = bayes_net.kept_regions(m, 0.5)                                            # the filtered object: its own regions
    pk = bayes_net.plotProbabilities(kept, str(tmp_path / "kept"))
    idx = [list(m.cnv_regions).index(name) for name in kept.cnv_regions]
    assert 0 < len(idx) < 5 and sorted(os.listdir(tmp_path / "kept")) == ["cellProbs.0.5.dat", "cnvProbs.0.5.dat"]
    same(pk.box, want_box[idx])
    cnv, cell = expected_tables(kept, want_box[idx])
    assert open(tmp_path / "kept" / "cnvProbs.0.5.dat", "rb").read() == cnv
    assert open(tmp_path / "kept" / "cellProbs.0.5.dat", "rb").read() == cell


# ---- run() with the hook ----------------------------------------------------------------------------------------------
RUN_ARGS = dict(cutoff=1, HMM=True, HMM_type="i6", leiden_method="simple", k_nn=10, BayesMaxPNormal=0.5, seed=7, no_prelim_plot=True)
NEW_FILES = ["cellProbs.0.5.dat", "cnvProbs.0.5.dat"] + [f"infercnv.NormalProbabilities.{when}Filtering.{what}" for when in ("Pre", "Post")
                                                          for what in ("heatmap.png", "heatmap_layout.json", "heatmap_thresholds.txt",
                                                                       "observation_groupings.txt")]


@pytest.fixture(scope="module")
def run_inputs(golden_dir):
    d = np.load(os.path.join(golden_dir, "example_run_inputs.npz"))
    x = d["mant"].astype(np.float64) / 10.0 ** d["neg_exp"].astype(np.float64)
    refs = {str(n): d[f"ref_{i}"] for i, n in enumerate(d["ref_names"])}
    obs = {str(n): d[f"obs_{i}"] for i, n in enumerate(d["obs_names"])}
    return {"counts": x, "chr": d["chr_levels"][d["chr_codes"]], "refs": refs, "obs": obs}


def run_once(ri, out, hooked, resident_shape=None, **kw):
    """run() on example/run.R's inputs into out; hooked: with bayes_probabilities_hook beside a recording hook;
    resident_shape: (G, C) of the host run's result -- the object goes to the device first and nothing of that size may cross."""
    import shutil
    from infercnv_amd import pipeline, run
    from test_gpu_resident import Hook, inputs_obj, no_crossing, tree_bytes
    if os.path.exists(out):
        shutil.rmtree(out)
    args = dict(RUN_ARGS, **kw)
    hook = Hook(*([pipeline.bayes_probabilities_hook(str(out), **args)] if hooked else []))
    obj = inputs_obj(ri)
    if resident_shape is not None:
        obj = obj.to_device()                                                        # the one upload, before the watch begins
        with no_crossing(*resident_shape):
            result = run(obj, out_dir=str(out), on_step=hook, **args)
    else:
        result = run(obj, out_dir=str(out), on_step=hook, **args)
    return result, hook, tree_bytes(out)


def check_hooked_against_plain(mode, plain, hooked):
    from infercnv_amd import pipeline
    (res_p, hook_p, files_p), (res_h, hook_h, files_h) = plain, hooked
    bayes_dir = pipeline.file_tokens(True, "i6", mode, "leiden", 0.5)["bayes_dir"]
    new = sorted(set(files_h) - set(files_p))
    assert new == sorted(os.path.join(bayes_dir, f) for f in NEW_FILES)
    for f, data in files_p.items():
        assert files_h[f] == data, f                                                 # every other file, byte for byte
    assert np.array_equal(bits(res_h.expr_data), bits(res_p.expr_data))
    assert list(hook_h.seen) == list(hook_p.seen) and 18 in hook_p.seen and 19 in hook_p.seen
    for step, o in hook_p.seen.items():
        if step != 18:
            assert np.array_equal(bits(hook_h.seen[step].expr_data), bits(o.expr_data)), step
    assert np.array_equal(bits(hook_h.seen[18].cnv_means), bits(hook_p.seen[18].cnv_means))
    return bayes_dir


@pytest.fixture(scope="module")
def subcluster_runs(dev, run_inputs, tmp_path_factory):
    out = tmp_path_factory.mktemp("k33") / "out"                                     # the SAME out_dir, one run after the other
    plain = run_once(run_inputs, out, False, analysis_mode="subclusters")
    hooked = run_once(run_inputs, out, True, analysis_mode="subclusters")
    return out, plain, hooked


def test_run_with_the_hook_subclusters(dev, subcluster_runs):
    _, plain, hooked = subcluster_runs
    bayes_dir = check_hooked_against_plain("subclusters", plain, hooked)
    files = hooked[2]
    lines = files[os.path.join(bayes_dir, "cnvProbs.0.5.dat")].decode().splitlines()
    kept = hooked[1].more[0].probabilities
    assert lines[0].split("\t") == list(pr.BOX_FIELDS) and len(lines) == 1 + 6 * len(kept.regions) and len(kept.regions) > 0
    assert len(kept.regions) <= len(hooked[1].seen[18].cnv_regions)
    assert len(files[os.path.join(bayes_dir, "cellProbs.0.5.dat")].decode().splitlines()) == 1 + int(kept.cell_off[-1])


def test_run_with_the_hook_resident(dev, run_inputs, subcluster_runs):
    """The same on obj.to_device(): no upload, no fetch, and every file of the host run byte for byte."""
    from test_gpu_resident import compare_objects
    out, _, hooked = subcluster_runs
    res, hook, files = run_once(run_inputs, out, True, resident_shape=hooked[0].expr_data.shape, analysis_mode="subclusters")
    assert res.is_resident()
    compare_objects(res, hooked[0], "returned object")
    assert list(hook.seen) == list(hooked[1].seen)
    for step, o in hooked[1].seen.items():
        compare_objects(hook.seen[step], o, f"step {step}")
    assert sorted(files) == sorted(hooked[2])
    for f, data in hooked[2].items():
        assert files[f] == data, f


def test_run_with_the_hook_no_plot(dev, run_inputs, subcluster_runs):
    """no_plot = True: the Bayes directory holds what it holds without the hook."""
    from infercnv_amd import pipeline
    out, plain, _ = subcluster_runs
    _, _, files = run_once(run_inputs, out, True, analysis_mode="subclusters", no_plot=True)
    bayes_dir = pipeline.file_tokens(True, "i6", "subclusters", "leiden", 0.5)["bayes_dir"]
    in_dir = lambda fs: {f: d for f, d in fs.items() if f.startswith(bayes_dir + os.sep)}
    assert in_dir(files) == in_dir(plain[2]) and not any("NormalProbabilities" in f or "Probs." in f for f in files)


def test_run_with_the_hook_cells_mode(dev, run_inputs, tmp_path):
    out = tmp_path / "out"
    plain = run_once(run_inputs, out, False, analysis_mode="cells")
    hooked = run_once(run_inputs, out, True, analysis_mode="cells")
    check_hooked_against_plain("cells", plain, hooked)
