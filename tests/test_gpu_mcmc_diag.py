"""The convergence diagnostics of the Bayesian filter's chains on the GPU (icnv_mcmc_diag_dev, DESIGN K31): every field of
every chain and every pooled field bit-equal to the sequential restatement of tests/mcmc_diag_restate.py; then
bayes_net.mcmc_diagnostics on the planted object of test_gpu_bayes.py, both routes, whatever the batching, and the run() hook."""
import ctypes as ct
import functools
import glob
import os

import numpy as np
import pytest

import mcmc_diag_restate as mr
from test_gpu_bayes import MU6, TAU6, planted_object, same

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


@functools.lru_cache(maxsize=None)
def case(m, n, K, R=7):
    """Seeded samples (R, m, n, K) with region 2 empty (NaN) and constants planted, and the restatement's answer (computed once)."""
    s = mr.make_samples(R, m, n, K, seed=1000 * K + n)
    if R > 2:
        s[2] = np.nan                                           # a region without cells
    if R > 3:
        s[3, 0, :, 1] = 0.25                                    # one constant chain of (region 3, state 1)
        s[4, :, :, 0] = 0.25                                    # every chain of (region 4, state 0) constant: W == 0
        s[5, 1, 5:9, K - 1] = [-0.0, 0.0, -0.0, 0.0]            # both zeros among the pooled draws
    s.setflags(write=False)
    cs, po = mr.diag(s)
    cs.setflags(write=False)
    po.setflags(write=False)
    return s, cs, po


def run(dev, s):
    cs, po = dev.mcmc_diag(torch.from_numpy(np.array(s)).cuda())
    return cs.cpu().numpy(), po.cpu().numpy()


# P = 13 at 20 and 21 (both parities of the window ends), acf50 NaN up to 50, a sort length that is no power of two, the
# default schedule, and the 8 192 limit at K = 6
@pytest.mark.parametrize("n_keep", [20, 21, 64, 100, 1000, 1365])
@pytest.mark.parametrize("K", [3, 6])
def test_bit_equal_to_the_restatement(dev, K, n_keep):
    s, want_cs, want_po = case(K, n_keep, K)
    cs, po = run(dev, s)
    same(cs, want_cs)
    same(po, want_po)
    assert np.isnan(cs[2]).all() and np.isnan(po[2]).all()                           # the empty region
    assert (cs[3, 1, 0, :4] == [0.25, 0.0, 0.0, 0.0]).all() and np.isnan(cs[3, 1, 0, 4:]).all()
    assert np.isnan(po[4, 0, 5]) and po[4, 0, 6] == 0.0 and (po[4, 0, :5] == [0.25, 0.0, 0.25, 0.25, 0.25]).all()
    assert np.isnan(cs[..., 8]).all() == (n_keep <= 50)
    one_cs, one_po = run(dev, s[:1])                                                 # one region: the same numbers
    same(one_cs, want_cs[:1])
    same(one_po, want_po[:1])


@pytest.mark.parametrize("m,n,K", [(2, 4096, 8), (8, 1024, 2), (4, 37, 5)])
def test_chain_count_is_its_own_parameter(dev, m, n, K):
    """n_chains != K; 2 x 4096 reaches the largest AR order (36) and the longest sort with the fewest wavefronts."""
    s, want_cs, want_po = case(m, n, K, R=2)
    cs, po = run(dev, s)
    same(cs, want_cs)
    same(po, want_po)


def test_host_twin_equals_device_entry(dev):
    s, want_cs, want_po = case(3, 100, 3)
    cs, po = dev.mcmc_diag_host(s)
    same(cs, want_cs)
    same(po, want_po)


def test_refusals_leave_the_outputs_alone(dev):
    from infercnv_amd import _lib
    L = _lib.load()
    for shape, code in (((1, 6, 19, 6), _lib.ERR_ARG), ((1, 9, 20, 3), _lib.ERR_ARG), ((1, 3, 20, 9), _lib.ERR_ARG),
                        ((1, 6, 20, 1), _lib.ERR_ARG), ((1, 6, 1366, 6), _lib.ERR_UNSUPPORTED)):
        R, m, n, K = shape
        assert mr.refusal(R, m, n, K) == ("ARG" if code == _lib.ERR_ARG else "UNSUPPORTED")
        t = torch.zeros(shape, dtype=torch.float64, device="cuda")
        with pytest.raises(_lib.IcnvError) as e:
            dev.mcmc_diag(t)
        assert e.value.code == code
        cs = torch.full((R, K, m, 9), 7.0, dtype=torch.float64, device="cuda")
        po = torch.full((R, K, 7), 7.0, dtype=torch.float64, device="cuda")
        assert L.icnv_mcmc_diag_dev(ct.c_void_p(t.data_ptr()), R, m, n, K, ct.c_void_p(cs.data_ptr()), ct.c_void_p(po.data_ptr()), None) == code
        torch.cuda.synchronize()
        assert bool((cs == 7.0).all()) and bool((po == 7.0).all())                   # nothing ran
    with pytest.raises(TypeError):
        dev.mcmc_diag(torch.zeros((1, 3, 20), dtype=torch.float64, device="cuda"))


# ---- bayes_net.mcmc_diagnostics ---------------------------------------------------------------------------------------
SCHED = dict(n_adapt=10, n_burn=5, n_keep=30)


def five_regions():
    """The planted object with two of its three regions cut in two by a neutral gap: five regions."""
    obj, states, tum = planted_object()
    states = states.copy()
    states[30:34, 20:] = 3
    states[150:152, 20:] = 3
    return obj, states


def expected_text(names, cs, po):
    from infercnv_amd.heatmap import r_num
    K = po.shape[1]
    lines = ["\t".join(mr.TABLE_COLUMNS)]
    for (r, k), row in zip(((r, k) for r in range(len(names)) for k in range(K)), mr.table(cs, po)):
        lines.append("\t".join([f"{names[r]}:State:{k + 1}"] + [r_num(v) for v in row]))
    return ("\n".join(lines) + "\n").encode()


@pytest.mark.parametrize("route", ["dict", "table"])
def test_mcmc_diagnostics_whatever_the_batching(dev, tmp_path, route):
    from infercnv_amd import bayes_net
    obj, states = five_regions()
    kw = dict(by="consensus", seed=4, mu=MU6, sig=TAU6, route=route, **SCHED)
    m = bayes_net.inferCNVBayesNet(obj, states, "i6", **kw)
    kept = bayes_net.inferCNVBayesNet(obj, states, "i6", keep_samples=True, **kw)
    assert len(m.cnv_regions) == 5 and m.cnv_probabilities[0] is None and kept.cnv_probabilities[0] is not None
    samples = np.stack([np.asarray(kept.cnv_probabilities[r]).reshape(6, SCHED["n_keep"], 6) for r in range(5)])
    want_cs, want_po = mr.diag(samples)
    per_region = 6 * SCHED["n_keep"] * 6 * 8
    for regions_per_batch in (1, 3, 5):
        d = bayes_net.mcmc_diagnostics(m, max_sample_bytes=regions_per_batch * per_region + 8)
        same(d.chain_stats, want_cs)
        same(d.pooled, want_po)
        assert list(d.regions) == list(m.cnv_regions)
    d = bayes_net.mcmc_diagnostics(kept, max_sample_bytes=1, out_dir=str(tmp_path / "held"))      # the held samples, one region a batch
    same(d.chain_stats, want_cs)
    same(d.pooled, want_po)
    bayes_net.mcmc_diagnostics(m, out_dir=str(tmp_path / "again"))
    want = expected_text(list(m.cnv_regions), want_cs, want_po)
    assert b"NaN" in want                                                            # acf50 at 30 kept draws
    for sub in ("held", "again"):
        assert open(tmp_path / sub / "CNV_MCMC_Diagnostics.dat", "rb").read() == want
    os.makedirs(tmp_path / "device")
    bayes_net.write_mcmc_diagnostics(d, str(tmp_path / "device"), device_rows=1)     # the route of a per-cell table
    assert open(tmp_path / "device" / "CNV_MCMC_Diagnostics.dat", "rb").read() == want
    f, _ = bayes_net.filterHighPNormals(m, states, 0.5)                              # the filtered object: its own regions
    df = bayes_net.mcmc_diagnostics(f)
    idx = [list(m.cnv_regions).index(name) for name in f.cnv_regions]
    assert 0 < len(idx) < 5
    same(df.pooled, want_po[idx])


def test_hook_writes_under_the_bayes_directory(dev, tmp_path):
    from infercnv_amd import bayes_net, pipeline
    obj, states, _ = planted_object()
    m = bayes_net.inferCNVBayesNet(obj, states, "i6", by="consensus", seed=4, mu=MU6, sig=TAU6, **SCHED)
    seen = []
    args = dict(HMM=True, HMM_type="i6", analysis_mode="samples")
    hook = pipeline.chain_hooks(pipeline.mcmc_diagnostics_hook(str(tmp_path), **args), lambda s, l, o: seen.append(s))
    hook(17, "HMM", object())
    assert glob.glob(str(tmp_path / "*")) == []
    hook(18, "Run Bayesian Network Model on HMM predicted CNVs", m)
    files = glob.glob(str(tmp_path / "BayesNetOutput.*" / "CNV_MCMC_Diagnostics.dat"))
    assert len(files) == 1 and os.path.basename(os.path.dirname(files[0])) == "BayesNetOutput.HMMi6.hmm_mode-samples"
    lines = open(files[0]).read().splitlines()
    assert lines[0].split("\t") == list(mr.TABLE_COLUMNS) and len(lines) == 1 + 3 * 6 and seen == [17, 18]
    assert lines[1].startswith(m.cnv_regions[0] + ":State:1\t")
