"""The window smoothers of step 10 on the GPU (icnv_smooth_windows[_dev], DESIGN K16): "runmeans" and "coordinates" bit-equal to
the sequential restatement of tests/smooth_windows_restate.py, K10's running mean as an independent witness, a generic weighted
table against the product's own pyramid stage, padded layouts, tiles whose span exceeds the LDS budget, every refusal of the
contract, the ops wrappers and the chain with smooth_method."""
import ctypes as ct

import numpy as np
import pytest

import oracle_np as onp
import smooth_windows_restate as swr
from parity_util import check_denoise_flips

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from infercnv_amd import GeneOrder, IcnvError, InfercnvObject, _lib, ops   # noqa: E402
from infercnv_amd import smooth_windows as sw                               # noqa: E402


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
    bad = a.view(np.uint64) != b.view(np.uint64)
    assert not bad.any(), f"{int(bad.sum())} differ, first at {np.argwhere(bad)[0]}: {a[bad][0]!r} vs {b[bad][0]!r}"


def on_dev(expr):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(expr, dtype=np.float64).T)).cuda()


def back(t):
    return t.cpu().numpy().T


# ---------------------------------------------------------------- runmeans
# the sizes the contract was written against, and the same with one more chromosome so that G is odd and no multiple of 16
RUNMEANS_SIZES = {"even": [1, 2, 3, 100, 101, 102, 257, 1, 3000, 17], "odd": [1, 2, 3, 100, 101, 102, 257, 1, 3000, 17, 5]}
_runmeans_ref = {}


def runmeans_case(layout, window):
    """(X, chr_start, restated result) at 67 cells: computed once, shared by the cell counts (the cells are independent)."""
    key = (layout, window)
    if key not in _runmeans_ref:
        cs = np.concatenate([[0], np.cumsum(RUNMEANS_SIZES[layout])]).astype(np.int32)
        X = np.random.default_rng(16).normal(0.0, 0.4, size=(int(cs[-1]), 67))
        _runmeans_ref[key] = (X, cs, swr.runmeans(X, cs, window))
    return _runmeans_ref[key]


@pytest.mark.parametrize("layout", ["even", "odd"])
@pytest.mark.parametrize("window", [1, 2, 7, 100, 101, 10001])
def test_runmeans_bit_equal_to_restatement(dev, layout, window):
    X, cs, want = runmeans_case(layout, window)
    assert (int(cs[-1]) % 2 == 1 and int(cs[-1]) % 16 != 0) == (layout == "odd")
    tab = sw.runmeans_windows(cs, window)
    for C in (1, 9, 67):
        same(back(dev.smooth_windows(on_dev(X[:, :C]), tab)), want[:, :C])


@pytest.mark.parametrize("window", [2, 100, 101])
def test_runmeans_bit_equal_to_k10_smoothing_launch(dev, window):
    X = np.random.default_rng(10).normal(0.0, 0.4, size=(1000, 6))
    x = on_dev(X)
    witness = dev.random_trees_matrix(x, np.arange(6), window_size=window, stages=_lib.RT_SMOOTH)
    got = dev.smooth_windows(x, sw.runmeans_windows([0, 1000], window))
    same(got.cpu().numpy(), witness.cpu().numpy())


# ---------------------------------------------------------------- coordinates
@pytest.mark.parametrize("w", [101, 5e4, 3e5, 1e7])
def test_coordinates_bit_equal_to_restatement(dev, w):
    start, stop = swr.layout60()
    cs = np.array([0, 60, 61, 63], dtype=np.int32)                  # + a chromosome of one gene and one of two
    start = np.concatenate([start, [5.0], [10.0, 900.0]])
    stop = np.concatenate([stop, [50.0], [700.0, 1500.0]])
    X = np.random.default_rng(63).normal(0.0, 0.4, size=(63, 9))
    got = back(dev.smooth_windows(on_dev(X), sw.coordinate_windows(cs, start, stop, w)))
    same(got, swr.coordinates(X, cs, start, stop, w))


def test_coordinates_hspike_layout_bit_equal_to_restatement(dev):
    pos = np.arange(1, 401, dtype=np.float64)
    X = np.random.default_rng(64).normal(0.0, 0.4, size=(400, 9))
    tab = sw.coordinate_windows([0, 400], pos, pos, 51)
    assert tab.widest == 201
    same(back(dev.smooth_windows(on_dev(X), tab)), swr.coordinates(X, [0, 400], pos, pos, 51))


# ---------------------------------------------------------------- a generic weighted table
@pytest.mark.parametrize("sizes,window", [([102, 300, 1500], 101), ([8, 40], 7)])
def test_generic_pyramid_table_matches_the_chain_stage(dev, sizes, window):
    cs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    X = np.random.default_rng(int(cs[-1])).normal(0.0, 0.1, size=(int(cs[-1]), 9))
    x = on_dev(X)
    got = back(dev.smooth_windows(x, swr.pyramid_windows(cs, window)))
    stage, _ = dev.smooth_chain(x, cs, [], window_length=window, stage_mask=_lib.ST_SMOOTH)
    err = np.abs(got - back(stage)).max()
    print(f"pyramid table vs ICNV_ST_SMOOTH, window {window}: max abs difference {err:.3e}")
    assert err <= 1e-11


# ---------------------------------------------------------------- layouts
def test_padded_input_and_output_give_the_same_bits(dev):
    X, cs, want = runmeans_case("odd", 101)
    X, want = X[:, :9], want[:, :9]
    G = X.shape[0]
    assert G % 16 != 0
    tab = sw.runmeans_windows(cs, 101)
    xp = dev.padded_matrix(9, G)
    assert xp.stride(0) != G
    xp.copy_(on_dev(X))
    outp = dev.padded_matrix(9, G)
    obase = outp._base
    obase.fill_(-7.0)
    got = dev.smooth_windows(xp, tab, out=outp)
    assert got.data_ptr() == outp.data_ptr()
    same(back(got), want)
    assert bool((obase[:, G:] == -7.0).all())                       # the padding is never written
    same(back(dev.smooth_windows(xp, tab)), want)                   # padded in, contiguous out
    same(back(dev.smooth_windows(on_dev(X), tab, out=outp)), want)  # contiguous in, padded out
    pos = np.arange(1, G + 1, dtype=np.float64)
    wtab = sw.coordinate_windows(cs, pos, pos, 20)                  # a weighted table through the same layouts
    same(back(dev.smooth_windows(xp, wtab, out=outp)), back(dev.smooth_windows(on_dev(X), wtab)))


def test_spilled_tiles_bit_equal_to_restatement(dev):
    """One chromosome of 20 000 genes, k = 10 001: no tile's span fits the LDS budget, every tile reads its rows from HBM."""
    X = np.random.default_rng(20).normal(0.0, 0.4, size=(20000, 3))
    tab = sw.runmeans_windows([0, 20000], 10001)
    dev.smooth_windows_stats(reset=True)
    got = back(dev.smooth_windows(on_dev(X), tab))
    st = dev.smooth_windows_stats()
    assert st["calls"] == 1 and st["tiles_spilled"] >= 1 and st["tiles_lds"] == 0, st
    same(got, swr.runmean_chr(X, 10001))


def test_mixed_lds_and_spilled_tiles(dev):
    """A short-window chromosome in front of a wide-window one: LDS tiles and spilled tiles in one call."""
    cs = np.array([0, 1500, 5500], dtype=np.int32)
    X = np.random.default_rng(21).normal(0.0, 0.4, size=(5500, 5))
    tab = sw.runmeans_windows(cs, 3001)
    dev.smooth_windows_stats(reset=True)
    got = back(dev.smooth_windows(on_dev(X), tab))
    st = dev.smooth_windows_stats()
    assert st["tiles_spilled"] >= 1 and st["tiles_lds"] >= 1, st
    same(got, swr.runmeans(X, cs, 3001))


# ---------------------------------------------------------------- errors
def _call_dev(L, x, out, G, C, lo, ln, w_off, w, den, ld_in=None, ld_out=None):
    lo = np.ascontiguousarray(lo, dtype=np.int32)
    ln = np.ascontiguousarray(ln, dtype=np.int32)
    den = np.ascontiguousarray(den, dtype=np.float64)
    ip, dp, i64p = ct.POINTER(ct.c_int32), ct.POINTER(ct.c_double), ct.POINTER(ct.c_int64)
    if w is not None:
        w_off = np.ascontiguousarray(w_off, dtype=np.int64)
        w = np.ascontiguousarray(w, dtype=np.float64)
    return L.icnv_smooth_windows_dev(ct.c_void_p(x), G if ld_in is None else ld_in, ct.c_void_p(out), G if ld_out is None else ld_out,
                                     G, C, lo.ctypes.data_as(ip), ln.ctypes.data_as(ip),
                                     w_off.ctypes.data_as(i64p) if w is not None else None,
                                     w.ctypes.data_as(dp) if w is not None else None, den.ctypes.data_as(dp),
                                     ct.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_every_refusal_leaves_the_output_untouched(dev):
    L = _lib.load()
    G, C = 40, 5
    x = on_dev(np.random.default_rng(1).normal(size=(G, C)))
    out = torch.full((C, G), -7.0, dtype=torch.float64, device="cuda")
    tab = sw.coordinate_windows([0, G], np.arange(1, G + 1.0), np.arange(1, G + 1.0), 5)
    good = dict(lo=tab.lo, ln=tab.len, w_off=tab.w_off, w=tab.w, den=tab.denom)

    def variant(**kw):
        v = {k: np.array(a, copy=True) for k, a in good.items()}
        for k, (i, val) in kw.items():
            v[k][i] = val
        return v

    bad_off = good["w_off"].copy()
    bad_off[3] = bad_off[2]                                           # row 2 has no room for its len weights: not monotone
    cases = {
        "lo < 0": variant(lo=(0, -1)),
        "len < 1": variant(ln=(4, 0)),
        "lo + len > G": variant(lo=(G - 1, G - 1)),
        "w_off": dict(good, w_off=bad_off),
        "denom zero": variant(den=(7, 0.0)),
        "denom inf": variant(den=(7, np.inf)),
        "denom nan": variant(den=(7, np.nan)),
    }
    for label, v in cases.items():
        rc = _call_dev(L, x.data_ptr(), out.data_ptr(), G, C, v["lo"], v["ln"], v["w_off"], v["w"], v["den"])
        assert rc == _lib.ERR_ARG, label
        assert bool((out == -7.0).all()), label
        t = sw.WindowTable(v["lo"], v["ln"], v["den"], v["w_off"], v["w"])
        with pytest.raises(IcnvError) as e:
            dev.smooth_windows(x, t, out=out)
        assert e.value.code == _lib.ERR_ARG and bool((out == -7.0).all()), label
    # in place, and a partial overlap: refused, the matrix keeps its values
    before = x.clone()
    assert _call_dev(L, x.data_ptr(), x.data_ptr(), G, C, **good) == _lib.ERR_ARG
    assert b"overlap" in L.icnv_last_error()
    with pytest.raises(IcnvError):
        dev.smooth_windows(x, tab, out=x)
    big = torch.full((2 * C, G), -7.0, dtype=torch.float64, device="cuda")
    big[:C] = x
    assert _call_dev(L, big.data_ptr(), big.data_ptr() + 8 * G * (C - 1), G, C, **good) == _lib.ERR_ARG
    assert bool((big[C:] == -7.0).all()) and torch.equal(x, before)
    assert _call_dev(L, x.data_ptr(), out.data_ptr(), G, C, **good, ld_in=G - 1) == _lib.ERR_ARG
    assert bool((out == -7.0).all())
    with pytest.raises(ValueError):
        dev.smooth_windows(x, sw.runmeans_windows([0, G + 1], 3), out=out)
    assert _call_dev(L, x.data_ptr(), out.data_ptr(), G, C, **good) == _lib.OK     # and the good table is accepted


@pytest.mark.parametrize("value", [np.nan, np.inf])
@pytest.mark.parametrize("weighted", [False, True])
def test_non_finite_input_is_refused(dev, value, weighted):
    G, C = 3000, 7
    X = np.random.default_rng(2).normal(size=(G, C))
    X[1234, 5] = value
    pos = np.arange(1, G + 1.0)
    tab = sw.coordinate_windows([0, G], pos, pos, 4) if weighted else sw.runmeans_windows([0, G], 101)
    with pytest.raises(IcnvError) as e:
        dev.smooth_windows(on_dev(X), tab)
    assert e.value.code == _lib.ERR_ARG and "not finite" in str(e.value)
    Xs = np.random.default_rng(2).normal(size=(20000, 2))             # and on the spilled path
    Xs[15000, 1] = value
    with pytest.raises(IcnvError) as e:
        dev.smooth_windows(on_dev(Xs), sw.runmeans_windows([0, 20000], 10001))
    assert e.value.code == _lib.ERR_ARG


# ---------------------------------------------------------------- ops wrappers and the chain
def make_obj(seed=7, with_hspike=True, interleave=True):
    """Three chromosomes whose genes are interleaved in the object's order (chr_layout() returns a permutation), references
    and observations, coordinates, and an hspike with start = stop = 1 .. n per chromosome."""
    rng = np.random.default_rng(seed)
    sizes = {"chrA": 150, "chrB": 61, "chrC": 1, "chrD": 90}
    chr_ = np.concatenate([[k] * n for k, n in sizes.items()])
    start = np.concatenate([np.sort(rng.integers(1, 40_000_000, size=n)) for n in sizes.values()]).astype(np.float64)
    stop = start + rng.integers(1_000, 400_000, size=start.size)
    if interleave:
        order = rng.permutation(chr_.size)
        order = np.concatenate([np.sort(order[:100]), np.sort(order[100:])])      # two interleaved runs, coordinates ascending in each
        chr_, start, stop = chr_[order], start[order], stop[order]
        for k in sizes:                                                            # within a chromosome the genes stay in coordinate order
            idx = np.nonzero(chr_ == k)[0]
            o = np.argsort(start[idx], kind="stable")
            start[idx], stop[idx] = start[idx][o], stop[idx][o]
    G, C = chr_.size, 30
    expr = np.log2(rng.gamma(2.0, 2.0, size=(G, C)) + 1.0)
    expr[:, 12:] += rng.normal(0.0, 0.3, size=(G, 1)) * (rng.random((G, 1)) < 0.3)
    hs = None
    if with_hspike:
        hchr = np.array(["chrA"] * 230 + ["chr_x"] * 120)
        pos = np.concatenate([np.arange(1, 231), np.arange(1, 121)]).astype(np.float64)
        hs = InfercnvObject(expr_data=np.log2(rng.gamma(2.0, 2.0, size=(350, 16)) + 1.0), gene_order=GeneOrder(hchr, pos, pos.copy()),
                            reference_grouped_cell_indices={"n": np.arange(8)}, observation_grouped_cell_indices={"t": np.arange(8, 16)})
    return InfercnvObject(expr_data=expr, gene_order=GeneOrder(chr_, start, stop),
                          reference_grouped_cell_indices={"n1": np.arange(6), "n2": np.arange(6, 12)},
                          observation_grouped_cell_indices={"t": np.arange(12, C)}, hspike=hs)


@pytest.mark.parametrize("method,window", [("runmeans", 101), ("runmeans", 8), ("coordinates", 5e6), ("coordinates", 3e5)])
def test_ops_wrappers_equal_the_restatement_per_chromosome(dev, method, window):
    obj = make_obj()
    assert obj.chr_layout()[0] is not None
    fn = ops.smooth_by_chromosome_runmeans if method == "runmeans" else ops.smooth_by_chromosome_coordinates
    got = fn(obj, window)
    same(got.expr_data, swr.on_object(obj, method, window))
    same(got.hspike.expr_data, swr.on_object(obj.hspike, method, window if method == "runmeans" else 51))
    same(obj.expr_data, make_obj().expr_data)                        # the input object is not modified


def test_ops_wrappers_window_one_returns_the_data(dev):
    obj = make_obj()
    same(ops.smooth_by_chromosome_runmeans(obj, 1).expr_data, obj.expr_data)
    got = ops.smooth_by_chromosome_coordinates(obj, 1)
    same(got.expr_data, obj.expr_data)
    same(got.hspike.expr_data, swr.on_object(obj.hspike, "coordinates", 51))     # the hspike's window is 51 whatever is passed


def _standalone(obj, method, window):
    """run()'s order, one wrapper per step (R/inferCNV_ops.R:771-1031)."""
    fn = ops.smooth_by_chromosome_runmeans if method == "runmeans" else ops.smooth_by_chromosome_coordinates
    o = ops.subtract_ref_expr_from_obs(obj)
    o = ops.apply_max_threshold_bounds(o, 3)
    o = fn(o, window)
    o = ops.center_cell_expr_across_chromosome(o, "median")
    o = ops.subtract_ref_expr_from_obs(o)
    o14 = ops.invert_log2(o)
    return o14, ops.clear_noise_via_ref_mean_sd(o14, 1.5)


def _oracle(obj, method, window):
    """The oracle's step functions composed around the restated smoother: (pre-denoise, denoised, (mu, s))."""
    refs = [np.asarray(v) for v in obj.reference_grouped_cell_indices.values()]
    x = onp.subtract_ref_expr_from_obs(np.asarray(obj.expr_data, dtype=np.float64), refs)
    x = onp.apply_max_threshold_bounds(x, 3.0)
    tmp = obj.copy()
    tmp.expr_data = x
    x = swr.on_object(tmp, method, window)
    x = onp.center_columns(x, "median")
    x = onp.subtract_ref_expr_from_obs(x, refs)
    pre = onp.invert_log2(x)
    ref_idx = np.concatenate(refs)
    mu, s = onp.clear_noise_params_via_ref_mean_sd(pre, ref_idx, 1.5)
    return pre, onp.clear_noise_bounds(pre, mu, s), (mu, s)


@pytest.mark.parametrize("method,window", [("runmeans", 101), ("coordinates", 5e6)])
def test_chain_with_smooth_method(dev, method, window):
    obj = make_obj()
    fused, hmm_in = ops.hip_smooth_chain(obj, window_length=window, smooth_method=method, return_hmm_input=True)
    o14, o22 = _standalone(obj, method, window)
    pre, den, (mu, s) = _oracle(obj, method, window)
    d = np.abs(hmm_in.expr_data - o14.expr_data).max()
    print(f"{method}: chain vs step functions, HMM input: {d:.3e}")
    assert d <= 1e-12
    check_denoise_flips(fused.expr_data, o22.expr_data, pre, mu, s, tol=1e-12, label=f"{method}: chain vs step functions")
    d = np.abs(hmm_in.expr_data - pre).max()
    print(f"{method}: chain vs oracle steps around the restated smoother, HMM input: {d:.3e}")
    assert d <= 1e-11
    check_denoise_flips(fused.expr_data, den, pre, mu, s, tol=1e-11, label=f"{method}: chain vs oracle")
    # the hspike mirrors steps 8 .. 14 with its own window
    hw = window if method == "runmeans" else 51
    hpre, _, _ = _oracle(obj.hspike, method, hw)
    assert np.abs(fused.hspike.expr_data - hpre).max() <= 1e-11
    assert np.abs(fused.hspike.expr_data - o14.hspike.expr_data).max() <= 1e-12

    # the device-resident twin, on the layout order
    perm, cs = obj.chr_layout()
    refs = [np.asarray(v, dtype=np.int32) for v in obj.reference_grouped_cell_indices.values()]
    table = sw.table_for(obj, method, window)
    out, dpre = dev.smooth_chain_windows(on_dev(obj.expr_data[perm]), cs, refs, table, want_pre_denoise=True)
    inv = np.empty_like(perm)
    inv[perm] = np.arange(perm.size)
    assert np.abs(back(dpre)[inv] - o14.expr_data).max() <= 1e-12
    check_denoise_flips(back(out)[inv], o22.expr_data, pre, mu, s, tol=1e-12, label=f"{method}: device twin vs step functions")
    assert np.abs(back(dpre)[inv] - pre).max() <= 1e-11
    check_denoise_flips(back(out)[inv], den, pre, mu, s, tol=1e-11, label=f"{method}: device twin vs oracle")


def test_default_smooth_method_is_the_fused_chain(dev):
    obj = make_obj()
    a, ah = ops.hip_smooth_chain(obj, return_hmm_input=True)
    b, bh = ops.hip_smooth_chain(obj, return_hmm_input=True, smooth_method="pyramidinal")
    same(a.expr_data, b.expr_data)
    same(ah.expr_data, bh.expr_data)
    same(a.hspike.expr_data, b.hspike.expr_data)
    with pytest.raises(ValueError):
        ops.hip_smooth_chain(obj, smooth_method="median")
