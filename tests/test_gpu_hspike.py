"""The hidden spike-in on the GPU (icnv_group_gene_tables[_dev], icnv_hspike_simulate[_dev], DESIGN K15): the group gene tables
and every simulated element bit-equal to the sequential restatement of tests/hspike_restate.py, the argument errors, and one
run from integer counts to i6 CNV calls."""
import ctypes as ct

import numpy as np
import pytest

import hspike_restate as hr

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


# ---------------------------------------------------------------- tables
SIZES = [1, 2, 63, 64, 65, 3000]


def table_case(G, seed):
    """genes x cells with zeros, negative zeros, cancellation rows (1e8 +- 1) and fractional values; the six group sizes, one
    overlapping non-contiguous group, and cells that belong to no group."""
    rng = np.random.default_rng(seed)
    C = sum(SIZES) + 150
    expr = rng.poisson(1.5, size=(G, C)).astype(np.float64) * rng.uniform(0.5, 2.0, size=(1, C))
    zero = expr == 0
    expr[zero] = np.where(rng.random(int(zero.sum())) < 0.3, -0.0, 0.0)
    for g in range(0, G, 7):                                   # cancellation: 1e8 +- 1 around a mean that is no double
        expr[g] = 1e8 + rng.integers(-1, 2, size=C)
    for g in range(3, G, 11):
        expr[g] = rng.normal(0.0, 1e-3, size=C) + np.where(rng.random(C) < 0.5, 1e8, -1e8)
    perm = rng.permutation(C - 100)                            # the last 100 cells: in no group
    groups, o = [], 0
    for s in SIZES:
        groups.append(np.sort(perm[o:o + s]))
        o += s
    groups.append(np.concatenate([groups[5][::37], groups[2][::2], perm[o:o + 20]]))   # overlaps, not contiguous, unsorted
    return expr, groups


@pytest.mark.parametrize("G", [1, 17, 4000, 10001])
def test_group_gene_tables_bit_equal(dev, G):
    expr, groups = table_case(G, G)
    x = on_dev(expr)
    m, v, nz = dev.group_gene_tables(x, groups)
    rm, rv, rn = hr.group_gene_tables(expr, groups)
    same(m.cpu().numpy(), rm)
    same(v.cpu().numpy(), rv)
    assert np.array_equal(nz.cpu().numpy(), rn)
    assert np.isnan(rv[0]).all()                               # the one-cell group: NaN, as R's var
    same(m.cpu().numpy(), dev.group_means(x, groups).cpu().numpy())
    # a leading dimension larger than G
    wide = torch.full((x.shape[0], G + 5), float("nan"), dtype=torch.float64, device=x.device)
    wide[:, :G] = x
    m2, v2, nz2 = dev.group_gene_tables(wide[:, :G], groups)
    same(m2.cpu().numpy(), rm)
    same(v2.cpu().numpy(), rv)
    assert np.array_equal(nz2.cpu().numpy(), rn)


def test_group_gene_tables_host_flavour(dev):
    from infercnv_amd import _lib
    expr, groups = table_case(17, 99)
    x = np.asfortranarray(expr)
    idx, off = _lib.pack_groups(groups)
    idx, ip = _lib.i32(idx)
    off, op = _lib.i32(off)
    n = len(groups)
    m, v, nz = np.empty((n, 17)), np.empty((n, 17)), np.empty((n, 17), dtype=np.int32)
    _lib.check(_lib.load().icnv_group_gene_tables(x.ctypes.data_as(ct.c_void_p), 17, x.shape[1], ip, op, n, m.ctypes.data_as(ct.c_void_p),
                                                  v.ctypes.data_as(ct.c_void_p), nz.ctypes.data_as(ct.c_void_p)))
    rm, rv, rn = hr.group_gene_tables(expr, groups)
    same(m, rm)
    same(v, rv)
    assert np.array_equal(nz, rn)


def test_group_gene_tables_argument_errors(dev):
    from infercnv_amd import _lib
    x = on_dev(np.ones((4, 6)))
    for groups in ([np.array([0, 1]), np.array([], dtype=np.int64)], [np.array([0, 6])]):
        with pytest.raises(_lib.IcnvError) as e:
            dev.group_gene_tables(x, groups)
        assert e.value.code == _lib.ERR_ARG


# ---------------------------------------------------------------- simulation
def splines():
    """A variance spline over log(m + 1) in [0.5, 6] and a dropout spline over log(m) in [-3, 5], fitted on the host: means
    below e^0.5 - 1 and above e^6 - 1, row means below e^-3 and above e^5 fall outside the fitted ranges.  Left of its range
    the variance spline goes below 0: the variance is 0 there and a mean under 0.5 gives an all-zero row."""
    from infercnv_amd.smooth_spline import smooth_spline
    rng = np.random.default_rng(3)
    x = np.sort(rng.uniform(0.5, 6.0, 400))
    fv = smooth_spline(x, 1.1 * x - 0.5 + 0.2 * np.sin(3 * x) + 0.05 * rng.standard_normal(400))
    x2 = np.sort(rng.uniform(-3.0, 5.0, 400))
    fp = smooth_spline(x2, 1.0 / (1.0 + np.exp(1.5 * (x2 - 1.0))) + 0.01 * rng.standard_normal(400))
    return fv, fp


def as_tuple(f):
    return (f.knots, f.coef, f.xmin, f.range)


def sim_means(n_genes, seed):
    rng = np.random.default_rng(seed)
    m = np.exp(rng.uniform(np.log(1e-3), np.log(3e4), n_genes))
    special = [0.0, 1e-3, 0.3, 2.0e4, 1099511627776.0, 0.6]     # m = 0, an all-zero row, left of the range, right, 2^40
    m[:min(n_genes, len(special))] = special[:min(n_genes, len(special))]
    return m


@pytest.mark.parametrize("n_genes,num_cells", [(1, 1), (1, 257), (63, 64), (63, 100), (4400, 100), (4400, 1), (10000, 64), (10000, 257)])
def test_simulate_bit_equal(dev, n_genes, num_cells):
    fv, fp = splines()
    tokens = [hr.fnv1a64("simnorm_cell_a"), hr.fnv1a64("spike_tumor_cell_a"), 7]
    means = np.vstack([sim_means(n_genes, 10 * n_genes + k) for k in range(3)])
    if n_genes > 1:
        means[1, 0], means[1, 1] = means[0, 1], 0.0           # the first row of every matrix differs in kind
    else:
        means[:, 0] = [0.0, 5.0, 3.0e4]
    seed = 11
    out = dev.hspike_simulate(means, num_cells, fv, fp, seed, tokens).cpu().numpy()
    assert out.shape == (3, num_cells, n_genes)
    for k in range(3):
        ref = hr.simulate(means[k], num_cells, as_tuple(fv), as_tuple(fp), seed, tokens[k])
        same(out[k].T, ref)
    if n_genes >= 63:
        g = np.nonzero(means[0] == 1e-3)[0][0]
        assert (out[0][:, g] == 0).all()                        # the all-zero row stays
        assert (out[0] > 0).any() and (out[0] == 0).any()
    again = dev.hspike_simulate(means, num_cells, fv, fp, seed, tokens).cpu().numpy()
    same(again, out)                                            # same seed, same matrices
    if n_genes >= 63 and num_cells >= 64:
        twin = dev.hspike_simulate(np.vstack([means[0], means[0]]), num_cells, fv, fp, seed, tokens[:2]).cpu().numpy()
        same(twin[0], out[0])
        assert (twin[0] != twin[1]).any()                       # another token, another matrix


def test_simulate_elementwise_restatement_and_host_flavour(dev):
    """The array restatement is the element-by-element one (numpy.random.Philox), and the host flavour is the device one."""
    from infercnv_amd import _lib
    fv, fp = splines()
    means = sim_means(40, 5)
    ref = hr.simulate_elementwise(means, 33, as_tuple(fv), as_tuple(fp), 2, 12345)
    same(hr.simulate(means, 33, as_tuple(fv), as_tuple(fp), 2, 12345), ref)
    same(dev.hspike_simulate(means, 33, fv, fp, 2, [12345]).cpu().numpy()[0].T, ref)
    out = np.empty((33, 40))
    m, mp = _lib.f64(means)
    tok = np.array([12345], dtype=np.uint64)
    _lib.check(_lib.load().icnv_hspike_simulate(mp, 40, 33, 1, _lib.f64(fv.knots)[1], _lib.f64(fv.coef)[1], fv.nk, fv.xmin, fv.range,
                                                _lib.f64(fp.knots)[1], _lib.f64(fp.coef)[1], fp.nk, fp.xmin, fp.range, 2,
                                                tok.ctypes.data_as(ct.POINTER(ct.c_uint64)), out.ctypes.data_as(ct.c_void_p)))
    same(out.T, ref)


def test_simulate_argument_errors(dev):
    from infercnv_amd import _lib
    from infercnv_amd.smooth_spline import SmoothSpline
    fv, fp = splines()
    means = np.array([[1.0, 2.0, 3.0]])

    def fails(m, a, b, word):
        with pytest.raises(_lib.IcnvError) as e:
            dev.hspike_simulate(m, 10, a, b, 0, [1])
        assert e.value.code == _lib.ERR_ARG and word in str(e.value)

    bad = fv.coef.copy()
    bad[3] = np.inf
    fails(means, SmoothSpline(fv.knots, bad, fv.xmin, fv.range), fp, "not finite")
    bad[3] = np.nan
    fails(means, fv, SmoothSpline(fv.knots, bad, fv.xmin, fv.range), "not finite")
    fails(np.array([[1.0, 2.0 ** 40 + 1.0, 3.0]]), fv, fp, "2^40")
    fails(np.array([[1.0, np.nan, 3.0]]), fv, fp, "not finite")
    three = SmoothSpline(np.array([0, 0, 0, 0, 1, 1, 1.0]), np.array([1.0, 2.0, 3.0]), 0.0, 1.0)
    fails(means, three, fp, "nk")
    fails(means, fv, three, "nk")


# ---------------------------------------------------------------- counts to i6 CNV calls
def test_counts_to_i6_calls(dev):
    from infercnv_amd import hmm, ops
    from infercnv_amd.hidden_spike import build_and_add_hspike, fit_splines, _table_groups
    from infercnv_amd.infercnv_object import GeneOrder, InfercnvObject

    counts, chrs, refs, obs, dup, dele = hr.synthetic_counts()
    raw = InfercnvObject(expr_data=counts, count_data=counts, gene_order=GeneOrder(chrs), reference_grouped_cell_indices=refs,
                         observation_grouped_cell_indices=obs, gene_names=np.array([f"g{j}" for j in range(counts.shape[0])]))
    logged, _ = ops.ingest_counts(raw, min_mean_expr_cutoff=0.1, min_cells_per_gene=3)          # steps 2-4
    kept = np.array([int(n[1:]) for n in logged.gene_names])
    norm = logged.copy()
    norm.expr_data = np.asfortranarray(logged.count_data, dtype=np.float64)
    norm = ops.normalize_counts_by_seq_depth(norm)                                             # step 3 alone: what the hspike is built from
    with_hs = build_and_add_hspike(norm, seed=4)
    hs = with_hs.hspike

    # the whole hspike against the restatement, given the library's spline coefficients
    groups = _table_groups(norm)
    rm, rv, rn = hr.group_gene_tables(norm.expr_data, groups)
    m, v, nz = dev.group_gene_tables(on_dev(norm.expr_data), groups)
    same(m.cpu().numpy(), rm)
    same(v.cpu().numpy(), rv)
    assert np.array_equal(nz.cpu().numpy(), rn)
    fv, fp = fit_splines(rm, rv, rn / np.array([len(g) for g in groups], dtype=np.float64)[:, None])
    r_counts, r_norm, r_chrs, r_refs, r_obs, r_names = hr.build_hspike(norm.expr_data, refs, obs, as_tuple(fv), as_tuple(fp), seed=4)
    same(hs.count_data, r_counts)
    assert list(hs.gene_order.chr) == r_chrs and list(hs.cell_names) == r_names
    assert all(np.array_equal(hs.reference_grouped_cell_indices[k], r_refs[k]) for k in r_refs) and list(hs.reference_grouped_cell_indices) == list(r_refs)
    assert all(np.array_equal(hs.observation_grouped_cell_indices[k], r_obs[k]) for k in r_obs) and list(hs.observation_grouped_cell_indices) == list(r_obs)
    # the normalised matrix: the target is a median of column sums of non-integers, summed in another order on the device
    assert np.allclose(hs.expr_data, r_norm, rtol=1e-12, atol=0, equal_nan=True)

    # the existing chain with its hspike mirror, the spike distributions and the i6 HMM on the cells
    work = logged.copy()
    work.hspike = ops.log2xplus1(hs)                                                          # step 4's mirror
    _, hmm_in = ops.hip_smooth_chain(work, return_hmm_input=True)
    dists = hmm.get_spike_dists(hmm_in.hspike)
    check_levels(dists)
    states = hmm.predict_CNV_via_HMM_on_indiv_cells(hmm_in, dists).expr_data
    tumor = obs["tumor"]
    for region, side in ((dup, 1), (dele, -1)):
        rows = np.nonzero(np.isin(kept, region))[0]
        modal = np.bincount(states[np.ix_(rows, tumor)].astype(np.int64).ravel(), minlength=7).argmax()
        assert (modal - 3) * side > 0, f"modal state {modal} of the planted region"


def check_levels(dists):
    from infercnv_amd import hmm
    assert list(sorted(dists, key=lambda k: float(k[4:]))) == list(hmm.CNV_LEVELS) and len(dists) == 6
    means = [dists[k]["mean"] for k in hmm.CNV_LEVELS]
    assert all(a < b for a, b in zip(means[:-1], means[1:])), means
    assert abs(means[2] - 1.0) < min(means[2] - means[1], means[3] - means[2]), means
