"""NA-aware median filter on the GPU (-m gpu, K19): icnv_median_filter_na[_dev], device.median_filter(na_aware=True) and
apply_median_filtering against R's NA result as restated in tests/median_na_restate.py.

One small layout: 331 genes in chromosomes of 1, 2, 9, 64, 65 and 190 genes (a one-gene chromosome; blocks that start and
end off a 64-bit word of the NA mask), 150 cells, tiles of 1, 2, 9, 40 and 70 cells with shuffled, interleaved indices and
28 cells in no tile; two data shapes (continuous values; ~90 % of the elements equal to one value with islands of
continuous values -- together they send outputs down the sparse, strip and border kernels); window_size 3, 7 and 15.

The finite expectation is computed ONCE per (data shape, window size) by the filter's existing checker
(oracle_c.median_filter) on the NaN-free base matrix and never changed: every case injects its NaNs into a copy of that
base, so the base is a cleaned matrix of every case, and the expectation is only looked at where the restatement says the
window holds no NA.
"""
import ctypes as ct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import oracle_c as oc  # noqa: E402
import median_na_restate as mr  # noqa: E402

CHR_SIZES = [1, 2, 9, 64, 65, 190]
TILE_SIZES = [1, 2, 9, 40, 70]
G, C = sum(CHR_SIZES), 150
WINDOWS = (3, 7, 15)
SHAPES = ("continuous", "denoised")
MU = 1.0124904741170890

NA_REAL = np.array([0x7FF00000000007A2], dtype=np.uint64).view(np.float64)[0]
NEG_QUIET = np.array([0xFFF8000000000000], dtype=np.uint64).view(np.float64)[0]
SIGNALLING = np.array([0x7FF0000000000001], dtype=np.uint64).view(np.float64)[0]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infercnv_amd import device
    torch.cuda.set_device(0)
    device.init(0)
    return device


def to_dev(x_gc):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x_gc, dtype=np.float64).T)).cuda()


def to_host(t_cg):
    return t_cg.cpu().numpy().T


@pytest.fixture(scope="module")
def layout():
    rng = np.random.default_rng(19)
    cs = np.concatenate([[0], np.cumsum(CHR_SIZES)]).astype(np.int32)
    perm = rng.permutation(C)
    off = np.concatenate([[0], np.cumsum(TILE_SIZES)])
    tiles = [perm[off[i]:off[i + 1]].astype(np.int32) for i in range(len(TILE_SIZES))]
    untiled = perm[off[-1]:]
    assert untiled.size == 28
    base = {}
    cont = rng.normal(1.0, 0.2, size=(G, C))
    base["continuous"] = cont
    den = np.full((G, C), MU)
    for _ in range(40):                                   # islands of continuous values: ~10 % of the elements
        g0, c0 = int(rng.integers(0, G - 4)), int(rng.integers(0, C - 4))
        g1, c1 = min(G, g0 + int(rng.integers(3, 30))), min(C, c0 + int(rng.integers(2, 12)))
        den[g0:g1, c0:c1] = rng.normal(1.0, 0.2, size=(g1 - g0, c1 - c0))
    den[:, tiles[4][10:30]] = np.where(rng.random((G, 20)) < 0.5, MU, cont[:, :20])   # ... and a stretch of tile cells half and half
    base["denoised"] = den
    return {"cs": cs, "tiles": tiles, "untiled": untiled, "base": base}


@pytest.fixture(scope="module")
def finite_ref(layout):
    """The plain filter's checker on the NaN-free bases: computed once, shared, never written."""
    ref = {}
    for shape in SHAPES:
        for w in WINDOWS:
            r = oc.median_filter(layout["base"][shape], layout["cs"], layout["tiles"], w)
            r.setflags(write=False)
            ref[shape, w] = r
    return ref


def run_na(dev, x, layout, w):
    out, n_na = dev.median_filter(to_dev(x), layout["cs"], layout["tiles"], w, na_aware=True, return_na_count=True)
    return to_host(out), n_na


@pytest.mark.parametrize("shape", SHAPES)
def test_no_nan_is_the_plain_entry(dev, layout, finite_ref, shape):
    x = layout["base"][shape]
    for w in WINDOWS:
        got, n_na = run_na(dev, x, layout, w)
        plain = to_host(dev.median_filter(to_dev(x), layout["cs"], layout["tiles"], w))
        assert n_na == 0
        assert np.array_equal(got.view(np.uint64), plain.view(np.uint64))
        mr.check_output(got, x, layout["cs"], layout["tiles"], w, finite_ref[shape, w])


def single_positions(layout):
    cs, tiles, T = layout["cs"], layout["tiles"], layout["tiles"][4]
    return {
        "block_corner": (int(cs[5]), int(T[0])),
        "chr_first_gene": (int(cs[4]), int(T[35])),
        "chr_last_gene": (int(cs[5]) - 1, int(T[35])),
        "tile_first_cell": (200, int(T[0])),
        "tile_last_cell": (200, int(T[-1])),
        "gene_63": (63, int(T[20])),
        "gene_64": (64, int(T[20])),
        "one_gene_chr": (0, int(T[10])),
        "one_cell_tile": (100, int(tiles[0][0])),
        "untiled_cell": (100, int(layout["untiled"][3])),
    }


@pytest.mark.parametrize("where", ["block_corner", "chr_first_gene", "chr_last_gene", "tile_first_cell", "tile_last_cell", "gene_63",
                                   "gene_64", "one_gene_chr", "one_cell_tile", "untiled_cell"])
def test_one_nan_stays_inside_its_block(dev, layout, finite_ref, where):
    g, c = single_positions(layout)[where]
    cs, tiles = layout["cs"], layout["tiles"]
    k = int(np.searchsorted(cs, g, side="right")) - 1
    for shape in SHAPES:
        x = layout["base"][shape].copy()
        x[g, c] = np.nan
        for w in WINDOWS:
            got, n_na = run_na(dev, x, layout, w)
            assert n_na == 1
            want_na = mr.check_output(got, x, cs, tiles, w, finite_ref[shape, w])
            if where == "untiled_cell":
                assert not want_na.any() and np.isnan(got).sum() == 1       # it poisons nothing
                continue
            tile = next(t for t in tiles if c in t)
            inside = np.zeros((G, C), dtype=bool)
            inside[cs[k]:cs[k + 1], tile] = True
            assert want_na[g, c] and not (want_na & ~inside).any()          # never across a chromosome or tile border
            assert np.array_equal(np.isnan(got), want_na)


def test_sparse_random_nan_keeps_most_outputs_finite(dev, layout, finite_ref):
    rng = np.random.default_rng(3)
    hit = rng.random((G, C)) < 0.002
    tiled = mr.tiled_cells(layout["tiles"], C)
    for w in WINDOWS:      # from the restatement alone, before any library output is looked at
        want_na = mr.na_outputs(hit, layout["cs"], layout["tiles"], w)
        assert (~want_na[:, tiled]).mean() >= 0.5, (w, (~want_na[:, tiled]).mean())
    for shape in SHAPES:
        x = layout["base"][shape].copy()
        x[hit] = np.nan
        for w in WINDOWS:
            got, n_na = run_na(dev, x, layout, w)
            assert n_na == int(hit.sum())
            mr.check_output(got, x, layout["cs"], layout["tiles"], w, finite_ref[shape, w])


@pytest.mark.parametrize("case", ["random_30_percent", "whole_cell", "whole_gene"])
def test_dense_nan_sets(dev, layout, finite_ref, case):
    rng = np.random.default_rng(len(case))
    hit = np.zeros((G, C), dtype=bool)
    if case == "random_30_percent":
        hit = rng.random((G, C)) < 0.3
    elif case == "whole_cell":
        hit[:, layout["tiles"][3][17]] = True
    else:
        hit[150, :] = True
    for shape in SHAPES:
        x = layout["base"][shape].copy()
        x[hit] = np.nan
        for w in WINDOWS:
            got, n_na = run_na(dev, x, layout, w)
            assert n_na == int(hit.sum())
            mr.check_output(got, x, layout["cs"], layout["tiles"], w, finite_ref[shape, w])


def test_nan_payloads(dev, layout, finite_ref):
    """NA_real_, a negative quiet NaN and a signalling pattern on input: every NA output of a tiled cell is NA_real_, the cells in
    no tile keep their payloads (both asserted bit by bit in check_output)."""
    rng = np.random.default_rng(5)
    x = layout["base"]["continuous"].copy()
    pick = rng.random((G, C))
    xb = x.view(np.uint64)
    for lo, v in ((0.000, NA_REAL), (0.002, NEG_QUIET), (0.004, SIGNALLING)):
        xb[(pick >= lo) & (pick < lo + 0.002)] = np.array([v]).view(np.uint64)[0]
    u = layout["untiled"]
    xb[10, u[0]], xb[11, u[1]], xb[12, u[2]] = (np.array([v]).view(np.uint64)[0] for v in (NA_REAL, NEG_QUIET, SIGNALLING))
    n_in = int(mr.is_na_bits(x).sum())
    assert n_in >= 3 * 50
    for w in WINDOWS:
        got, n_na = run_na(dev, x, layout, w)
        assert n_na == n_in
        mr.check_output(got, x, layout["cs"], layout["tiles"], w, finite_ref["continuous", w])
        gb = got.view(np.uint64)
        assert gb[12, u[2]] == np.uint64(0x7FF0000000000001) and gb[11, u[1]] == np.uint64(0xFFF8000000000000)


def test_infinities_and_huge_values_next_to_nan(dev, layout):
    """+-Inf and 1e300 are numbers: next to a NaN they poison nothing, and clean windows equal the plain entry (and the checker)."""
    rng = np.random.default_rng(6)
    base = layout["base"]["denoised"].copy()
    spots = [(70, layout["tiles"][4][k]) for k in (5, 6, 7)] + [(200 + k, layout["tiles"][3][12]) for k in range(3)]
    for (g, c), v in zip(spots, (np.inf, -np.inf, 1e300, np.inf, -np.inf, 1e300)):
        base[g, c] = v
    base[rng.random((G, C)) < 0.003] = np.inf
    base[250:262, layout["tiles"][4][40:52]] = np.inf      # 12 x 12 positions of one block: 5 x 5 windows whose median is +Inf
    x = base.copy()
    x[71, layout["tiles"][4][6]] = np.nan
    x[201, layout["tiles"][3][13]] = np.nan
    x[rng.random((G, C)) < 0.001] = np.nan
    for w in WINDOWS:
        ref = oc.median_filter(base, layout["cs"], layout["tiles"], w)
        plain = to_host(dev.median_filter(to_dev(base), layout["cs"], layout["tiles"], w))
        got, n_na = run_na(dev, x, layout, w)
        assert n_na == int(np.isnan(x).sum())
        want_na = mr.check_output(got, x, layout["cs"], layout["tiles"], w, ref)
        clean = ~want_na & mr.tiled_cells(layout["tiles"], C)[None, :]
        assert np.array_equal(got.view(np.uint64)[clean], plain.view(np.uint64)[clean])
        assert w != 3 or np.isposinf(got[clean]).any()


def test_surface_host_entry_wrapper_and_c_abi_agree(dev, layout, finite_ref):
    from infercnv_amd import _lib
    from infercnv_amd._lib import check, i32, pack_groups
    rng = np.random.default_rng(8)
    x = np.asfortranarray(layout["base"]["denoised"].copy())
    x[rng.random((G, C)) < 0.004] = np.nan
    L = _lib.load()
    cs, cp = i32(layout["cs"])
    idx, off = pack_groups(layout["tiles"])
    idx, ip = i32(idx)
    off, op = i32(off)
    for w in WINDOWS:
        # the device entry through the C ABI
        xd = to_dev(x)
        od = torch.empty_like(xd)
        n_dev = ct.c_int64(-1)
        check(L.icnv_median_filter_na_dev(ct.c_void_p(xd.data_ptr()), ct.c_void_p(od.data_ptr()), G, C, cp, cs.size - 1, ip, op,
                                          len(layout["tiles"]), w, ct.byref(n_dev), None))
        torch.cuda.synchronize()
        want = to_host(od)
        mr.check_output(want, x, layout["cs"], layout["tiles"], w, finite_ref["denoised", w])
        assert n_dev.value == int(np.isnan(x).sum())
        # the wrapper, with and without the counter
        got, n_wrap = run_na(dev, x, layout, w)
        got2 = to_host(dev.median_filter(to_dev(x), layout["cs"], layout["tiles"], w, na_aware=True))
        assert n_wrap == n_dev.value
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)) and np.array_equal(got2.view(np.uint64), want.view(np.uint64))
        # the host-buffer entry (a null counter is allowed)
        oh = np.empty_like(x, order="F")
        n_host = ct.c_int64(-1)
        check(L.icnv_median_filter_na(x.ctypes.data_as(ct.c_void_p), oh.ctypes.data_as(ct.c_void_p), G, C, cp, cs.size - 1, ip, op,
                                      len(layout["tiles"]), w, ct.byref(n_host)))
        assert n_host.value == n_dev.value
        assert np.array_equal(np.ascontiguousarray(oh).view(np.uint64), np.ascontiguousarray(want).view(np.uint64))
        oh2 = np.empty_like(x, order="F")
        check(L.icnv_median_filter_na(x.ctypes.data_as(ct.c_void_p), oh2.ctypes.data_as(ct.c_void_p), G, C, cp, cs.size - 1, ip, op,
                                      len(layout["tiles"]), w, None))
        assert np.array_equal(np.ascontiguousarray(oh2).view(np.uint64), np.ascontiguousarray(want).view(np.uint64))
    with pytest.raises(ValueError):
        dev.median_filter(to_dev(x), layout["cs"], layout["tiles"], 7, return_na_count=True)
    with pytest.raises(RuntimeError):      # the plain entry's refusals
        dev.median_filter(to_dev(x), layout["cs"], layout["tiles"], 17, na_aware=True)
    xd = to_dev(x)
    with pytest.raises(RuntimeError):
        dev.median_filter(xd, layout["cs"], layout["tiles"], 7, out=xd, na_aware=True)


def test_apply_median_filtering_gives_r_na(dev, layout, finite_ref):
    """The mirror takes the NA-aware entry when the object holds a NaN (R gives NA there; the plain entry returned finite
    numbers) and the plain one otherwise (what it returned before)."""
    from infercnv_amd import GeneOrder, InfercnvObject, noise_reduction
    from infercnv_amd import sharded
    tiles, cs = layout["tiles"], layout["cs"]
    levels = np.repeat(np.array(["chr%d" % (k + 1) for k in range(len(CHR_SIZES))]), CHR_SIZES)
    ref_cells = tiles[4]
    obs_cells = np.concatenate(tiles[:4])

    def make(x):
        # the tiles in the order apply_median_filtering walks them: the subclusters of the observation groups, then the reference groups
        return InfercnvObject(expr_data=x, gene_order=GeneOrder(chr=levels),
                              reference_grouped_cell_indices={"normal": ref_cells},
                              observation_grouped_cell_indices={"tumor": obs_cells},
                              tumor_subclusters={"subclusters": {"tumor": {"s%d" % i: tiles[i] for i in range(4)},
                                                                 "normal": {"normal_s1": ref_cells}}})
    base = layout["base"]["denoised"]
    plain = noise_reduction.apply_median_filtering(make(base.copy()))
    mr.check_output(plain.expr_data, base, cs, tiles, 7, finite_ref["denoised", 7])
    assert not np.isnan(plain.expr_data).any()
    x = base.copy()
    x[150, tiles[4][3]] = np.nan
    x[64, tiles[2][1]] = np.nan
    x[30, layout["untiled"][0]] = np.nan
    got = noise_reduction.apply_median_filtering(make(x))
    want_na = mr.check_output(got.expr_data, x, cs, tiles, 7, finite_ref["denoised", 7])
    assert want_na.sum() > 2 and np.isnan(got.expr_data).sum() == want_na.sum() + 1
    # the sharded wrapper passes na_aware through
    sh = sharded.ShardedMedianFilter().run(to_dev(x), cs, tiles, 7, na_aware=True)
    assert np.array_equal(to_host(sh).view(np.uint64), np.ascontiguousarray(got.expr_data).view(np.uint64))
