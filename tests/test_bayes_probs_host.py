"""The K33 probability heatmaps and tables without a GPU: the reference's own stored run (tests/golden/mcmc_probabilities.npz,
mcmc_cell_gene.npz) through the restated paint, the filter's kept set and the cellProbs table; the box restatement of
tests/bayes_probs_restate.py against matplotlib.cbook.boxplot_stats; the run() hook's directory and no-op cases; the two tables
byte for byte against tests/table_text_restate.py.

TOL_BOX is 10 x the largest relative difference measured over THIS file's series between the contract's quantile
((1 - h) xl + h xh) and numpy.percentile's (which matplotlib uses) on the CPU it was written on; the measured value stands
beside the constant.  It bounds a rounding difference between two interpolation formulas, not the method."""
import ctypes as ct
import os

import numpy as np
import pytest

import bayes_probs_restate as pr
import mcmc_diag_restate as mr
import table_text_restate as tt

TOL_BOX = 2.2e-15        # measured 2.14e-16: lower, middle, upper vs numpy.percentile; the whisker ends are draws and agree exactly
FENCE_GAP = 1e-9         # no draw of the series below lies this close to a fence: a count cannot hinge on an ulp


def fixture_regions(golden_dir):
    cg = np.load(os.path.join(golden_dir, "mcmc_cell_gene.npz"))
    return [(str(n), cg[f"genes_{i}"].astype(np.int64) - 1, cg[f"cells_{i}"].astype(np.int64) - 1) for i, n in enumerate(cg["names"])]


def stored_object(golden_dir, out_dir=None):
    """The reference's stored MCMC run as a dict-route MCMCInferCNV (no infercnv object behind it: 20 cells, 4 400 gene rows)."""
    from infercnv_amd import bayes_net
    z = np.load(os.path.join(golden_dir, "mcmc_probabilities.npz"))
    states = np.load(os.path.join(golden_dir, "hmm_states_example.npz"))["HMM_states"]
    regs = fixture_regions(golden_dir)
    m = bayes_net.MCMCInferCNV(infercnv_obj=None)
    m.cnv_regions = [n for n, _, _ in regs]
    m.cell_gene = [{"cnv_regions": n, "Genes": g, "Cells": c, "State": int(states[g[0], c[0]])} for n, g, c in regs]
    m.cnv_means = z["theta_means"].copy()
    m.cnv_probabilities = [None] * 9
    m.cell_probabilities = [z["cell_probabilities"][i] for i in range(9)]
    m.mu = np.zeros(6)
    m.args = {"HMM_type": "i6", "postMcmcMethod": "removeCNV", "reassignCNVs": True, "out_dir": out_dir, "BayesMaxPNormal": 0}
    return m, states


def test_stored_run_painted(golden_dir):
    """1 - theta_means[2] over the nine regions: the run-based restatement of the paint (the arrays the kernel takes, from
    bayes_net._region_arrays) equals R's expr.data[Genes, Cells] <- v loop, and the values are the ones the issue quotes."""
    from infercnv_amd import bayes_net
    m, states = stored_object(golden_dir)
    value = 1.0 - m.cnv_means[2]
    assert [round(float(v), 4) for v in value] == [0.6246, 0.8564, 0.8129, 0.6260, 0.8105, 0.5595, 0.5595, 0.4992, 0.5295]
    G, C = states.shape
    g0, ng, off, idx = bayes_net._region_arrays(m)
    assert pr.paint_refusal(G, C, g0, ng, off, idx) is None and off[-1] == 90 and idx.dtype == np.int32
    got = pr.paint(G, C, g0, ng, off, idx, value)
    want = pr.paint_cell_gene(G, C, m.cell_gene, value)
    assert np.array_equal(got.T, want)
    assert int((want != 0).sum()) == sum(len(cg["Genes"]) * len(cg["Cells"]) for cg in m.cell_gene)     # the nine are disjoint
    assert set(np.unique(want)) == {0.0} | {float(v) for v in value}


def test_stored_run_kept_regions(golden_dir, tmp_path):
    """At R's default threshold the kept set is the eight regions other than index 7; kept_regions is filterHighPNormals'
    object, field by field, and writes nothing."""
    from infercnv_amd import bayes_net
    m, states = stored_object(golden_dir, out_dir=str(tmp_path / "k"))
    kept = bayes_net.kept_regions(m, 0.5)
    assert not os.path.exists(tmp_path / "k")
    assert list(kept.cnv_regions) == [n for i, n in enumerate(m.cnv_regions) if i != 7] and len(m.cnv_regions) == 9
    f, _ = bayes_net.filterHighPNormals(m, states, 0.5)
    assert os.path.exists(tmp_path / "k" / "CNV_State_Probabilities.dat")
    assert list(kept.cnv_regions) == list(f.cnv_regions) and kept.args == f.args and kept.args["BayesMaxPNormal"] == 0.5
    assert np.array_equal(kept.cnv_means, f.cnv_means)
    for a, b in zip(kept.cell_gene, f.cell_gene):
        assert a["cnv_regions"] == b["cnv_regions"] and a["State"] == b["State"]
        assert np.array_equal(a["Genes"], b["Genes"]) and np.array_equal(a["Cells"], b["Cells"])
    for a, b in zip(kept.cell_probabilities, f.cell_probabilities):
        assert np.array_equal(a, b)
    assert [cg["State"] for cg in kept.cell_gene] == [int(np.argmax(m.cnv_means[:, i])) + 1 for i in range(9) if i != 7]
    assert m.args["BayesMaxPNormal"] == 0 and len(m.cell_gene) == 9                     # the input object is untouched


def record_of(m, cells, box=None):
    from infercnv_amd import bayes_net
    _, _, off, idx = bayes_net._region_arrays(m)
    R, K = len(m.cnv_regions), 6
    return bayes_net.CnvProbabilities(regions=bayes_net._region_names(m), box=np.zeros((R, K, 7)) if box is None else box,
                                      cell_off=off, cell_idx=idx, cell_probs=np.concatenate([cp.T for cp in m.cell_probabilities]),
                                      cell_names=cells, threshold=m.args.get("BayesMaxPNormal"))


def test_stored_run_cell_table_round_trips(golden_dir, tmp_path):
    from infercnv_amd import bayes_net
    m, _ = stored_object(golden_dir)
    kept = bayes_net.kept_regions(m, 0.5)
    cells = np.array([f"cell_{i + 1}" for i in range(20)])
    probs = record_of(kept, cells)
    cnv_path, cell_path = bayes_net.write_cnv_probabilities(probs, str(tmp_path))
    assert (os.path.basename(cnv_path), os.path.basename(cell_path)) == ("cnvProbs.0.5.dat", "cellProbs.0.5.dat") == pr.file_names(0.5)
    lines = open(cell_path).read().splitlines()
    assert lines[0].split("\t") == [f"State:{k}" for k in range(1, 7)] and len(lines) == 1 + 8 * 10
    z = np.load(os.path.join(golden_dir, "mcmc_probabilities.npz"))["cell_probabilities"]
    row = 1
    for i in (0, 1, 2, 3, 4, 5, 6, 8):
        for j, c in enumerate(m.cell_gene[i]["Cells"]):
            f = lines[row].split("\t")
            assert f[0] == f"{m.cnv_regions[i]}:cell_{c + 1}"
            got = np.array([float(v) for v in f[1:]])
            assert np.abs(got - z[i, :, j]).max() <= 5e-16 and abs(got.sum() - 1.0) < 1e-14      # 15 significant digits of k / 6000
            row += 1
    names, mat, cols = pr.cell_table(list(kept.cnv_regions), [cg["Cells"] for cg in kept.cell_gene], kept.cell_probabilities, cells)
    assert open(cell_path, "rb").read() == tt.file_bytes(mat.T, "cell_rows", list(range(len(names))), names, cols, quoted=False, sep="\t")


def box_series():
    """Dirichlet-like draws as the sampler keeps them, (K chains, n_keep) per (region, state), one state constant."""
    for K in (3, 6):
        for n in (20, 21, 100, 1000):
            s = mr.make_samples(8, K, n, K, seed=33 * K + n).copy()
            s[:, :, :, K - 1] = 0.125
            for r in range(s.shape[0]):
                for k in range(K):
                    yield K, n, k == K - 1, s[r, :, :, k]


def test_box_against_matplotlib(capsys):
    from matplotlib import cbook
    worst, n_series, n_out = 0.0, 0, 0
    for K, n, constant, y in box_series():
        flat = y.ravel()
        got = pr.box_stats(y)
        lo, hi = pr.fences(y)
        if not constant:
            assert np.abs(flat - lo).min() > FENCE_GAP and np.abs(flat - hi).min() > FENCE_GAP
        st = cbook.boxplot_stats(flat, whis=1.5)[0]
        want = [st["whislo"], st["q1"], st["med"], st["q3"], st["whishi"]]
        assert got[5] == float((st["fliers"] < st["q1"]).sum()) and got[6] == float((st["fliers"] > st["q3"]).sum())
        assert got[0] == want[0] and got[4] == want[4]                                       # draws, not interpolations
        if constant:
            assert got == [0.125] * 5 + [0.0, 0.0]
        worst = max(worst, max(abs(g - w) / abs(w) for g, w in zip(got[1:4], want[1:4])))
        n_series += 1
        n_out += int(got[5] + got[6])
    with capsys.disabled():
        print(f"\n[bayes_probs] box vs matplotlib.cbook.boxplot_stats: {worst:.3g} over {n_series} series, {n_out} outliers")
    assert n_series == 288 and n_out > 100
    assert worst <= TOL_BOX


def test_box_degenerate_and_planted():
    assert all(v != v for v in pr.box_stats(np.full((3, 20), np.nan)))
    y = np.array([0.0, -0.0, 0.0, -0.0])
    got = pr.box_stats(y)
    assert got == [0.0] * 7 and not any(np.signbit(v) for v in got)                          # -0.0 is reported as +0.0
    base = np.arange(1.0, 42.0)                                                              # quartiles 11, 21, 31: fences -19, 61
    assert pr.fences(base) == (-19.0, 61.0)
    assert pr.box_stats(base) == [1.0, 11.0, 21.0, 31.0, 41.0, 0.0, 0.0]
    on = base.copy()
    on[0], on[40] = -19.0, 61.0                                                              # ON the fences: strict comparisons keep them
    assert pr.fences(on) == (-19.0, 61.0) and pr.box_stats(on) == [-19.0, 11.0, 21.0, 31.0, 61.0, 0.0, 0.0]
    out = base.copy()
    out[0], out[1], out[40] = -19.5, -100.0, 61.5
    assert pr.fences(out) == (-19.0, 61.0) and pr.box_stats(out) == [3.0, 11.0, 21.0, 31.0, 40.0, 2.0, 1.0]
    assert pr.box_stats([0.25, 0.75]) == [0.25, 0.375, 0.5, 0.625, 0.75, 0.0, 0.0]           # N = 2


def test_refusals_need_no_gpu():
    from infercnv_amd import _lib
    L = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "icnv.h")).read()
    for name in ("icnv_paint_regions_dev", "icnv_theta_box_dev"):
        assert name in _lib.PROTOTYPES and hasattr(L, name) and name + "(" in header
    assert "believed, not verified against ggplot2" in header
    buf = np.zeros(8)
    p = ct.c_void_p(buf.ctypes.data)          # never dereferenced: every call below fails before any device work
    code = {"ARG": _lib.ERR_ARG, "UNSUPPORTED": _lib.ERR_UNSUPPORTED}
    for R, m, n, K in ((1, 6, 0, 6), (-1, 6, 100, 6), (1, 1, 100, 6), (1, 9, 100, 6), (1, 6, 100, 1), (1, 6, 100, 9),
                       (1, 8, 1025, 8), (1, 2, 4100, 2), (2 ** 30, 2, 20, 8)):
        want = pr.box_refusal(R, m, n, K)
        assert want is not None
        assert L.icnv_theta_box_dev(p, R, m, n, K, p, None) == code[want], (R, m, n, K)
    assert L.icnv_theta_box_dev(None, 1, 6, 100, 6, p, None) == _lib.ERR_ARG
    for ok in ((0, 6, 100, 6), (1, 8, 1024, 8), (3, 2, 1, 2), (1, 6, 19, 6)):                # unlike K31: no regions, n_keep from 1 up
        assert pr.box_refusal(*ok) is None
    assert L.icnv_theta_box_dev(p, 0, 6, 100, 6, p, None) == 0
    for G, C, ld in ((0, 4, 4), (4, 0, 4), (4, 4, 3)):
        assert L.icnv_paint_regions_dev(p, G, C, ld, 0, None, None, None, None, 0, None, None) == _lib.ERR_ARG
    assert L.icnv_paint_regions_dev(None, 4, 4, 4, 0, None, None, None, None, 0, None, None) == _lib.ERR_ARG
    assert L.icnv_paint_regions_dev(p, 4, 4, 4, 1, None, p, p, p, 1, p, None) == _lib.ERR_ARG
    assert L.icnv_paint_regions_dev(p, 4, 4, 4, -1, p, p, p, p, 1, p, None) == _lib.ERR_ARG
    G, C = 7, 3
    good = ([1, 0], [3, 7], [0, 2, 3], [0, 2, 1])
    assert pr.paint_refusal(G, C, *good) is None
    for bad in (([5, 0], [3, 7], [0, 2, 3], [0, 2, 1]), ([1, 0], [3, 7], [0, 2, 3], [0, 3, 1]), ([1, 0], [3, 7], [0, 2, 1], [0, 2, 1]),
                ([1, 0], [3, 7], [0, 2, 4], [0, 2, 1]), ([1, -1], [3, 7], [0, 2, 3], [0, 2, 1]), ([1, 0], [3, 7], [1, 2, 3], [0, 2, 1])):
        assert pr.paint_refusal(G, C, *bad) == "ARG"


def hand_record():
    from infercnv_amd import bayes_net
    box = np.zeros((2, 2, 7))
    box[0, 0] = [0.125, 0.25, 1.0 / 3.0, 0.5, 0.75, 0.0, 12.0]
    box[0, 1] = [1e-05, 0.0001, 0.5, 100000.0, 1234567.0, 3.0, 0.0]
    box[1, 0] = [np.nan] * 7
    box[1, 1] = [2.0, 2.0, 2.0, 2.0, 2.0, 0.0, 0.0]
    probs = np.array([[0.0, 1.0], [1.0 / 3.0, 2.0 / 3.0], [0.5, 0.5], [1.0 / 6000.0, 5999.0 / 6000.0]])
    return bayes_net.CnvProbabilities(regions=np.array(["chr1-region_1", "chr2-region_12"]), box=box, cell_off=np.array([0, 3, 4]),
                                      cell_idx=np.array([2, 0, 1, 2]), cell_probs=probs, cell_names=np.array(["a", "b", "c c"]),
                                      threshold=0.5)


HAND_CNV = ("ymin\tlower\tmiddle\tupper\tymax\tn_low\tn_high\n"
            "chr1-region_1:State:1\t0.125\t0.25\t0.333333333333333\t0.5\t0.75\t0\t12\n"
            "chr1-region_1:State:2\t1e-05\t1e-04\t0.5\t1e+05\t1234567\t3\t0\n"
            "chr2-region_12:State:1\tNaN\tNaN\tNaN\tNaN\tNaN\tNaN\tNaN\n"
            "chr2-region_12:State:2\t2\t2\t2\t2\t2\t0\t0\n")
HAND_CELL = ("State:1\tState:2\n"
             "chr1-region_1:c c\t0\t1\n"
             "chr1-region_1:a\t0.333333333333333\t0.666666666666667\n"
             "chr1-region_1:b\t0.5\t0.5\n"
             "chr2-region_12:c c\t0.000166666666666667\t0.999833333333333\n")


def test_tables_byte_for_byte(tmp_path):
    from infercnv_amd import bayes_net
    probs = hand_record()
    assert probs.box_fields == pr.BOX_FIELDS == bayes_net.BOX_TABLE_COLUMNS
    cnv_path, cell_path = bayes_net.write_cnv_probabilities(probs, str(tmp_path / "sub"))
    assert open(cnv_path, "rb").read() == HAND_CNV.encode() and open(cell_path, "rb").read() == HAND_CELL.encode()
    names, mat = pr.cnv_table(list(probs.regions), probs.box)
    assert list(probs.cnv_row_names()) == names and np.array_equal(probs.cnv_table(), mat, equal_nan=True)
    assert open(cnv_path, "rb").read() == tt.file_bytes(mat.T, "cell_rows", list(range(4)), names, pr.BOX_FIELDS, quoted=False, sep="\t")
    cells_of = [probs.cell_idx[0:3], probs.cell_idx[3:4]]
    names, mat, cols = pr.cell_table(list(probs.regions), cells_of, [probs.cell_probs[0:3].T, probs.cell_probs[3:4].T], probs.cell_names)
    assert list(probs.cell_row_names()) == names and tuple(cols) == probs.cell_columns()
    assert open(cell_path, "rb").read() == tt.file_bytes(mat.T, "cell_rows", list(range(4)), names, cols, quoted=False, sep="\t")
    for thr, want in ((None, ("cnvProbs.dat", "cellProbs.dat")), (0, ("cnvProbs.0.dat", "cellProbs.0.dat")),
                      (0.25, ("cnvProbs.0.25.dat", "cellProbs.0.25.dat")), (1e-05, ("cnvProbs.1e-05.dat", "cellProbs.1e-05.dat"))):
        probs.threshold = thr
        assert probs.file_names() == want == pr.file_names(thr)


def test_hook_directory_and_no_op_cases(monkeypatch, tmp_path, caplog):
    import logging
    from infercnv_amd import bayes_net, pipeline
    calls = []

    class Obj:
        args = {"HMM_type": "i6", "out_dir": "elsewhere"}

    monkeypatch.setattr(bayes_net, "postProbNormal", lambda obj, title, name, **kw: calls.append(("heat", getattr(obj, "args", obj), title, name, kw)))
    monkeypatch.setattr(bayes_net, "kept_regions", lambda obj, thr: calls.append(("kept", thr)) or "kept object")
    monkeypatch.setattr(bayes_net, "plotProbabilities", lambda obj, out_dir, **kw: calls.append(("tables", obj, out_dir, kw)) or "record")
    args = dict(HMM=True, HMM_type="i6", analysis_mode="subclusters", BayesMaxPNormal=0.3, cutoff=1, denoise=True, k_obs_groups=2,
                cluster_by_groups=False, useRaster=False)
    hook = pipeline.bayes_probabilities_hook(str(tmp_path), max_sample_bytes=777, **args)
    want_dir = os.path.join(str(tmp_path), pipeline.file_tokens(True, "i6", "subclusters", "leiden", 0.3)["bayes_dir"])
    assert hook.out_dir == want_dir and os.path.basename(want_dir) == "BayesNetOutput.HMMi6.leiden.hmm_mode-subclusters"
    for step in list(range(1, 18)) + [19, 20, 21, 22]:
        hook(step, "label", object())
    assert calls == [] and hook.probabilities is None
    pipeline.chain_hooks(hook)(18, "Run Bayesian Network Model on HMM predicted CNVs", Obj())
    assert [c[0] for c in calls] == ["heat", "kept", "tables", "heat"] and hook.probabilities == "record"
    pre, kept, tables, post = calls
    assert pre[2:] == (" (1 - Probabilities of Normal) Before Filtering", "infercnv.NormalProbabilities.PreFiltering",
                       {"out_dir": want_dir, "useRaster": False})
    assert pre[1]["k_obs_groups"] == 2 and pre[1]["cluster_by_groups"] is False and pre[1]["out_dir"] == "elsewhere"
    assert "k_obs_groups" not in Obj.args                                                    # the caller's object is left alone
    assert kept == ("kept", 0.3) and tables == ("tables", "kept object", want_dir, {"max_sample_bytes": 777})
    assert post[1] == "kept object"
    assert post[2:] == (" (1 - Probabilities of Normal) With Threshold 0.3", "infercnv.NormalProbabilities.PostFiltering",
                        {"out_dir": want_dir, "useRaster": False})
    for off in (dict(no_plot=True), dict(plot_probabilities=False)):
        del calls[:]
        caplog.clear()
        quiet = pipeline.bayes_probabilities_hook(str(tmp_path), **dict(args, **off))
        with caplog.at_level(logging.INFO, logger="infercnv_amd"):
            quiet(17, "HMM", Obj())
            quiet(18, "mcmc", Obj())
        assert calls == [] and len(caplog.records) == 1 and os.listdir(tmp_path) == []
    assert "plot_probabilities" in pipeline.IGNORED_OPTIONS    # run()'s own argument stays accepted and ignored
    with pytest.raises(ValueError):
        pipeline.bayes_probabilities_hook(str(tmp_path), analysis_mode="regions")


def test_post_prob_normal_writes_nothing_with_no_plot(tmp_path):
    from infercnv_amd import bayes_net
    m = bayes_net.MCMCInferCNV(infercnv_obj=None)
    m.args = {"HMM_type": "i6", "no_plot": True, "out_dir": str(tmp_path / "x")}
    assert bayes_net.postProbNormal(m, "t", "name") is None and not os.path.exists(tmp_path / "x")
