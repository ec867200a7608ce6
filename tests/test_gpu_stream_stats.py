"""The memory-bound kernels every run passes through (-m gpu): ingest.hip, stats_kernels.hip and the per-cell reductions and
elementwise kernels of chain_kernels.hip / viterbi_kernels.hip, at the shapes where they take another path, against
tests/stream_stats_restate.py (tied to the oracles by tests/test_stream_stats_host.py).

Every shape is the smallest that reaches its path: one element, one short of / exactly / one past a 256-gene tile, C % 4 in
{1, 2, 3} for the CSC kernels' four columns per block, more slices wanted than cells, the 1024-slice cap, a grid that wraps
(8 192 blocks; 4 x 8 192 columns for CSC; 4 096 blocks for the per-cell min / max; 16 x CU count blocks for the clamp), the
16-byte pair loops' boundaries at 768 / 1024 / 1792 / 2048 pairs with and without the odd-G leftover.

Every tolerance is one of: equality (integer or dyadic data, or the same IEEE operations in the same order), a bound derived
in stream_stats_restate (sum_bound, sd_bound, 1 ulp for an exact sum divided once in long double and rounded twice), or the
project's existing 1e-12 -- the comment at each assertion says which.
"""
import ctypes as ct
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import stream_stats_restate as ss  # noqa: E402

FORMS = ("dense", "csc")
FLAGS = ((0, 0), (1, 0), (0, 1), (1, 1))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infercnv_amd import device
    torch.cuda.set_device(0)
    device.init(0)
    return device


@pytest.fixture(scope="module")
def L(dev):
    from infercnv_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def n_cu(dev):
    return torch.cuda.get_device_properties(0).multi_processor_count


def to_dev(x_gc, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x_gc, dtype=dtype).T)).cuda()


def to_host(t_cg):
    return t_cg.cpu().numpy().T


def vp(t):
    return ct.c_void_p(t.data_ptr()) if t is not None else ct.c_void_p(0)


def same_bits(a, b):
    return np.array_equal(ss.bits(a), ss.bits(b))


def same_values(a, b):
    """Equal where finite, NaN in the same places (a NaN's payload is the hardware's business)."""
    return np.array_equal(a, b, equal_nan=True)


def make_counts(dev, form, x=None, csc=None, G=None):
    """DeviceCounts in either form from a dense (G, C) int32 matrix or from CSC arrays."""
    if form == "dense":
        if x is None:
            x = ss.csc_to_dense(*csc, G)
        return dev.DeviceCounts(x.shape[0], x.shape[1], dense=to_dev(x, np.int32))
    if csc is None:
        csc = ss.dense_to_csc(x, seed=x.shape[0])
        G = x.shape[0]
    colptr, rowidx, vals = csc
    return dev.DeviceCounts(G, len(colptr) - 1, colptr=torch.from_numpy(colptr).cuda(), rowidx=torch.from_numpy(rowidx).cuda(),
                            vals=torch.from_numpy(vals).cuda())


def csc_slice(csc, a, b):
    colptr, rowidx, vals = csc
    lo, hi = int(colptr[a]), int(colptr[b])
    return (colptr[a:b + 1] - lo).astype(np.int64), rowidx[lo:hi].copy(), vals[lo:hi].copy()


def apply_flags(L, counts, keep_idx, cs_t, factor, do_norm, do_log, out=None):
    """icnv_ingest_apply_dev with its two flags free (device.ingest_apply fixes them at 1, 1) -> (rc, (C, G_out) tensor)."""
    keep = torch.as_tensor(np.asarray(keep_idx, dtype=np.int32), device="cuda")
    if out is None:
        out = torch.full((counts.C, int(keep.numel())), -777.0, dtype=torch.float64, device="cuda")
    rc = L.icnv_ingest_apply_dev(ct.byref(counts.c), counts.G, counts.C, vp(keep), int(keep.numel()), vp(cs_t if do_norm else None),
                                 float(factor), int(do_norm), int(do_log), vp(out), None)
    torch.cuda.synchronize()
    return rc, out


def stats_of(dev, counts):
    st = dev.ingest_gene_stats(counts).cpu().numpy()
    return st[:counts.G].tolist(), st[counts.G:].tolist()


# ================================================================== A. ingest, dense int32 and CSC
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", ss.INGEST_SHAPES + (ss.INGEST_CSC_WRAP,), ids=lambda s: f"{s[0]}x{s[1]}")
def test_ingest_gene_stats_int64_sums_slices_and_wrap(dev, shape, form):
    """Sums and positive counts of ~90 % zero counts with INT32_MAX planted five times in a gene and three times in a cell:
    (300, 1030) reaches the 1024-slice cap with empty trailing slices, (4113, 37) wants more slices than there are cells,
    (5, 8195) and (4, 32771) are the wrap shapes of the later phases."""
    x, _ = ss.count_matrix(*shape, seed=shape[0])
    sums, pos = ss.gene_stats_int(x)
    got_s, got_n = stats_of(dev, make_counts(dev, form, x))
    assert got_s == [float(s) for s in sums]            # equality: integer sums below 2^53
    assert got_n == [float(n) for n in pos]             # equality: counts


@pytest.mark.parametrize("shape", ss.INGEST_SHAPES + (ss.INGEST_CSC_WRAP,), ids=lambda s: f"{s[0]}x{s[1]}")
def test_ingest_col_sums_and_apply_flags_wrap_8192_and_csc_wrap_32768(dev, L, shape):
    """Column sums over a keep mask that drops the first gene, the last gene and a run in the middle, and apply with all four
    flag combinations, dense and CSC and -- the header's claim -- icnv_normalize_log2_dev on the f64 copy of the kept rows.
    (5, 8195) wraps the dense kernels' 8 192-block grid, (4, 32771) the CSC kernels' 8 192 blocks of four columns."""
    G, C = shape
    x, info = ss.count_matrix(G, C, seed=G)
    keep = info["keep"]
    keep_idx = np.nonzero(keep)[0].astype(np.int32)
    want_cs = ss.col_sums_int(x, keep)
    f = 10000.0                                       # (the median as the factor is test_ingest_one_call_equals_its_phases_and_a_split's)
    kept_f64 = to_dev(x[keep])
    res = {}
    for form in FORMS:
        counts = make_counts(dev, form, x)
        cs_t = dev.ingest_col_sums(counts, keep_idx)
        assert cs_t.cpu().numpy().tolist() == [float(s) for s in want_cs], form        # equality: integer sums below 2^53
        for dn, dl in FLAGS:
            rc, out = apply_flags(L, counts, keep_idx, cs_t, f, dn, dl)
            assert rc == 0
            res[form, dn, dl] = to_host(out)
    for dn, dl in FLAGS:
        res["f64", dn, dl] = to_host(dev.normalize_log2(kept_f64, col_sums_t=cs_t, normalize_factor=f, do_normalize=bool(dn), do_log2=bool(dl)))
        assert same_bits(res["dense", dn, dl], res["csc", dn, dl]), (dn, dl)           # equality: the same operations on the same counts
        assert same_bits(res["dense", dn, dl], res["f64", dn, dl]), (dn, dl)           # equality: the header's bit-for-bit claim
    assert same_bits(res["dense", 0, 0], x[keep].astype(np.float64))                   # equality: (double)count
    norm = ss.apply_counts(x[keep], want_cs, f, True, False)
    assert same_values(res["dense", 1, 0], norm)                                       # equality: IEEE divide and multiply in R's order
    for dn in (0, 1):
        want = ss.apply_counts(x[keep], want_cs, f, bool(dn), True)
        got = res["dense", dn, 1]
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.abs(got[ok] - want[ok]).max(initial=0.0) < 1e-12                     # the project's existing 1e-12 for this entry
    zero = np.array(want_cs) == 0                                                      # zero-sum cells: 0 / 0 * f in all three routes
    assert info["c_zero"] is None or zero[info["c_zero"]]
    for route in ("dense", "csc", "f64"):
        for dl in (0, 1):
            assert np.isnan(res[route, 1, dl][:, zero]).all() and not np.isnan(res[route, 1, dl][:, ~zero]).any()
            assert (res[route, 0, dl][:, zero] == 0.0).all()                           # without the division: plain values
    if shape == (300, 1030):
        finite = norm[~np.isnan(norm)]
        got = res["dense", 1, 1][~np.isnan(norm)]
        worst = max(ss.ulp_distance(g, math.log2(v + 1.0)) for g, v in zip(got.tolist(), finite.tolist()))
        print(f"\nlog2: largest ulp distance from math.log2 over {finite.size} elements = {worst}; "
              f"largest |difference| from np.log2 = {np.abs(got - np.log2(finite + 1.0)).max():.3e} of the 1e-12 allowed")


@pytest.mark.parametrize("C", sorted(ss.CSC_CASES), ids=lambda c: f"csc_c_mod4_C{c}")
def test_csc_layouts_column_lengths_unsorted_explicit_zeros_dropped_column(dev, L, C):
    """131 genes, C in {1, 2, 3, 5, 7} (C % 4 != 0, C < 4): columns of 0, 1, 63, 64, 65 and 130 stored entries around the
    64-lane stride, shuffled inside the column, with explicitly stored zeros, and a column whose entries all lie in dropped
    genes -- there the NaN fill and the scatter of the CSC apply run together."""
    colptr, rowidx, vals, keep = ss.csc_layout(C)
    x = ss.csc_to_dense(colptr, rowidx, vals, ss.CSC_G)
    keep_idx = np.nonzero(keep)[0].astype(np.int32)
    sums, pos = ss.gene_stats_int(x)
    want_cs = ss.col_sums_int(x, keep)
    f = 1000.0
    res = {}
    for form in FORMS:
        counts = make_counts(dev, form, x=x if form == "dense" else None, csc=(colptr, rowidx, vals), G=ss.CSC_G)
        got_s, got_n = stats_of(dev, counts)
        assert got_s == [float(s) for s in sums] and got_n == [float(n) for n in pos], form   # equality; a stored zero is in no "cells > 0"
        cs_t = dev.ingest_col_sums(counts, keep_idx)
        assert cs_t.cpu().numpy().tolist() == [float(s) for s in want_cs], form               # equality: integer sums
        for dn, dl in FLAGS:
            rc, out = apply_flags(L, counts, keep_idx, cs_t, f, dn, dl)
            assert rc == 0
            res[form, dn, dl] = to_host(out)
    for dn, dl in FLAGS:
        assert same_bits(res["dense", dn, dl], res["csc", dn, dl]), (dn, dl)                  # equality: the same operations
    assert same_values(res["csc", 1, 0], ss.apply_counts(x[keep], want_cs, f, True, False))   # equality: IEEE divide and multiply
    assert same_bits(res["csc", 0, 0], x[keep].astype(np.float64))                            # equality: (double)count
    for c, kind in enumerate(ss.CSC_CASES[C]):
        assert want_cs[c] == 0 or kind not in ("dropped", 0)
        for dl in (0, 1):
            if want_cs[c] == 0:                                                               # fill and scatter together: 0 / 0 * f everywhere
                assert np.isnan(res["csc", 1, dl][:, c]).all() and (res["csc", 0, dl][:, c] == 0.0).all()
            else:
                assert not np.isnan(res["csc", 1, dl][:, c]).any()


def test_csc_nnz_zero_gives_the_all_nan_matrix_like_dense(dev):
    """nnz == 0, no filters, normalize_factor NaN: every column sum is 0, their median is 0, R's 0 / 0 * 0 is NaN."""
    G, C = ss.CSC_G, 5
    empty = (np.zeros(C + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32))
    res = {}
    for form in FORMS:
        counts = make_counts(dev, form, x=np.zeros((G, C), np.int32) if form == "dense" else None, csc=empty, G=G)
        st = dev.ingest_gene_stats(counts).cpu().numpy()
        assert (st == 0.0).all()
        expr, kept, f = dev.ingest_counts(counts)
        assert kept.tolist() == list(range(G)) and f == 0.0 and tuple(expr.shape) == (C, G)
        res[form] = to_host(expr)
        assert np.isnan(res[form]).all()
    assert same_bits(res["dense"], res["csc"])                                                # equality: identical from the dense form


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("C", (10, 11), ids=("even_C", "odd_C"))
def test_ingest_one_call_equals_its_phases_and_a_split(dev, L, C, form):
    """icnv_ingest_counts_dev against gene_stats -> select -> col_sums -> median -> apply (kept genes, factor, bits; even and odd
    C run both branches of the host median), and the cells split at column 3 -- not a multiple of the CSC kernels' four
    columns per block -- and in the middle: statistics add up, column sums concatenate, apply with the global factor gives
    the whole's slice."""
    G, cutoff, min_cells = 257, 0.25, 2
    x, _ = ss.count_matrix(G, C, seed=C)
    csc = ss.dense_to_csc(x, seed=C)
    counts = make_counts(dev, form, x=x, csc=csc, G=G)
    sums, pos = ss.gene_stats_int(x)
    assert ss.mean_gap(sums, C, cutoff) > 1e-9
    want_keep = ss.select_genes(sums, pos, C, cutoff, min_cells)
    assert 0 < want_keep.size < G
    expr, kept, f = dev.ingest_counts(counts, cutoff, min_cells)
    stats = dev.ingest_gene_stats(counts).cpu().numpy()
    kept2 = dev.ingest_select(stats, G, C, cutoff, min_cells)
    assert kept.tolist() == kept2.tolist() == want_keep.tolist()                      # equality: the filter decision
    cs_t = dev.ingest_col_sums(counts, kept2)
    want_cs = ss.col_sums_int(x[want_keep])
    assert cs_t.cpu().numpy().tolist() == [float(s) for s in want_cs]                 # equality: integer sums
    assert f == ss.r_median(want_cs)                                                  # equality: a selection, one exact halving
    whole = dev.ingest_apply(counts, kept2, cs_t, f)
    assert same_bits(to_host(expr), to_host(whole))                                   # equality: the same kernels on the same inputs
    want = ss.apply_counts(x[want_keep], want_cs, f)
    assert np.array_equal(np.isnan(to_host(whole)), np.isnan(want))
    assert np.nanmax(np.abs(to_host(whole) - want)) < 1e-12                           # the project's existing 1e-12 for this entry
    for cut in (3, C // 2):
        st_sum, cs_cat, parts = np.zeros(2 * G), [], []
        for a, b in ((0, cut), (cut, C)):
            shard = make_counts(dev, form, x=x[:, a:b], csc=csc_slice(csc, a, b), G=G)
            st_sum += dev.ingest_gene_stats(shard).cpu().numpy()
            cs_s = dev.ingest_col_sums(shard, kept2)
            cs_cat += cs_s.cpu().numpy().tolist()
            parts.append(to_host(dev.ingest_apply(shard, kept2, cs_s, f)))
        assert np.array_equal(st_sum, stats), cut                                     # equality: every split gives the same statistics
        assert cs_cat == cs_t.cpu().numpy().tolist(), cut                             # equality
        assert same_bits(np.concatenate(parts, axis=1), to_host(whole)), cut          # equality: per-element arithmetic


def test_ingest_refusals_return_err_arg_and_leave_outputs_untouched(dev, L):
    from infercnv_amd import _lib
    G, C = 131, 5
    colptr, rowidx, vals, keep = ss.csc_layout(C)
    x = ss.csc_to_dense(colptr, rowidx, vals, G)
    keep_idx = np.nonzero(keep)[0].astype(np.int32)
    good = {form: make_counts(dev, form, x=x, csc=(colptr, rowidx, vals), G=G) for form in FORMS}
    cs_t = dev.ingest_col_sums(good["dense"], keep_idx)

    def one_call(counts):
        kbuf = np.full(G, -5, dtype=np.int32)
        n, used = ct.c_int64(-5), ct.c_double(-5.0)
        out = torch.full((C * G,), -777.0, dtype=torch.float64, device="cuda")
        rc = L.icnv_ingest_counts_dev(ct.byref(counts.c), G, C, float("nan"), 0, float("nan"), kbuf.ctypes.data_as(ct.POINTER(ct.c_int32)),
                                      ct.byref(n), vp(out), ct.byref(used), None)
        torch.cuda.synchronize()
        untouched = (kbuf == -5).all() and n.value == -5 and used.value == -5.0 and bool((out == -777.0).all())
        return rc, untouched

    # a negative entry (R's NA_integer_ is INT_MIN), dense and CSC
    xn = x.copy()
    xn[70, 3] = np.iinfo(np.int32).min
    vn = vals.copy()
    vn[vn.size // 2] = -1
    for bad in (make_counts(dev, "dense", x=xn), make_counts(dev, "csc", csc=(colptr, rowidx, vn), G=G)):
        assert one_call(bad) == (_lib.ERR_ARG, True)
        stats = torch.empty(2 * G, dtype=torch.float64, device="cuda")
        assert L.icnv_ingest_gene_stats_dev(ct.byref(bad.c), G, C, vp(stats), None) == _lib.ERR_ARG
    # both forms given, neither form given: every phase refuses before it touches anything
    both = _lib.Counts(good["dense"].c.dense, good["csc"].c.colptr, good["csc"].c.rowidx, good["csc"].c.vals, good["csc"].c.nnz)
    neither = _lib.Counts(None, None, None, None, 0)
    for c in (both, neither):
        holder = type("H", (), {"c": c, "G": G, "C": C})
        assert one_call(holder) == (_lib.ERR_ARG, True)
        stats = torch.full((2 * G,), -777.0, dtype=torch.float64, device="cuda")
        assert L.icnv_ingest_gene_stats_dev(ct.byref(c), G, C, vp(stats), None) == _lib.ERR_ARG
        mask = torch.ones(G, dtype=torch.uint8, device="cuda")
        cs_o = torch.full((C,), -777.0, dtype=torch.float64, device="cuda")
        assert L.icnv_ingest_col_sums_dev(ct.byref(c), G, C, vp(mask), vp(cs_o), None) == _lib.ERR_ARG
        rc, out = apply_flags(L, holder, keep_idx, cs_t, 1.0, 1, 1)
        torch.cuda.synchronize()
        assert rc == _lib.ERR_ARG and bool((out == -777.0).all()) and bool((stats == -777.0).all()) and bool((cs_o == -777.0).all())
    # G_out > G, dense and CSC (the list is never read)
    for form in FORMS:
        out = torch.full((C, G + 1), -777.0, dtype=torch.float64, device="cuda")
        rc, out = apply_flags(L, good[form], np.zeros(G + 1, np.int32), cs_t, 1.0, 1, 1, out=out)
        assert rc == _lib.ERR_ARG and bool((out == -777.0).all()), form
    # a keep index out of range in the CSC apply
    for bad_idx in (G, -1):
        k = keep_idx.copy()
        k[5] = bad_idx
        rc, out = apply_flags(L, good["csc"], k, cs_t, 1.0, 1, 1)
        assert rc == _lib.ERR_ARG and bool((out == -777.0).all()), bad_idx
    rc, out = apply_flags(L, good["csc"], keep_idx, cs_t, 1.0, 1, 1)                  # ... and the library is still in order
    assert rc == 0 and not bool((out == -777.0).any())


# ================================================================== B. gene statistics, scaling and row selection on f64
def gene_stats(L, x):
    G, C = x.shape
    xd = to_dev(x)
    s = torch.full((G,), -777.0, dtype=torch.float64, device="cuda")
    n = torch.full((G,), -777, dtype=torch.int32, device="cuda")
    assert L.icnv_gene_stats_dev(vp(xd), G, C, vp(s), vp(n), None) == 0
    torch.cuda.synchronize()
    return s.cpu().numpy(), n.cpu().numpy()


@pytest.mark.parametrize("shape", ss.GENE_STATS_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gene_stats_f64_position_coded_fsum_bound_and_positive_counts(dev, L, shape):
    G, C = shape
    x = ss.position_coded(G, C)
    s, n = gene_stats(L, x)
    assert s.tolist() == [float(v) for v in ss.gene_stats_int(x.astype(np.int64))[0]]     # equality: integers below 2^53; a dropped or doubled element names itself
    assert n.tolist() == [C] * G
    x = np.random.default_rng(G).lognormal(0.5, 0.8, size=(G, C))
    s, n = gene_stats(L, x)
    want = ss.gene_sums_fsum(x)
    bound = np.array([ss.sum_bound(C, math.fsum(r)) for r in x.tolist()])                 # derived: C * 2^-53 * sum|x_g|, any summation order
    assert (np.abs(s - want) <= bound).all()
    assert n.tolist() == [C] * G
    rng = np.random.default_rng(G + 1)
    pool = np.array([np.nan, -0.0, 0.0, -1.5, np.inf, 5e-324, 2.2250738585072014e-308 / 4, 1.0, 3.25])
    x = pool[rng.integers(0, pool.size, size=(G, C))]
    s, n = gene_stats(L, x)
    assert n.tolist() == ss.positive_counts(x)                                            # equality: x > 0 & !is.na(x)


def scale_genes(L, x):
    G, C = x.shape
    xd = to_dev(x)
    out = torch.full((C, G), -777.0, dtype=torch.float64, device="cuda")
    assert L.icnv_scale_genes_dev(vp(xd), vp(out), G, C, None) == 0
    torch.cuda.synchronize()
    return to_host(out)


@pytest.mark.parametrize("shape", ss.SCALE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_scale_genes_tiles_slices_wrap_8192_and_constant_genes(dev, L, shape):
    G, C = shape
    const = ss.SCALE_CONSTANT[shape]
    x = ss.scale_input(G, C, seed=G, constant=const)
    got = scale_genes(L, x)
    want = ss.scale_rows(x)
    assert np.nonzero(np.isnan(got).any(axis=1))[0].tolist() == sorted(const)             # a planted constant gene gives NaN, nothing else does
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want).any(axis=1)                                                      # (the host test: only the planted genes are exempt)
    if ok.any():
        assert np.abs(got[ok] - want[ok]).max() < 1e-12                                   # the project's existing 1e-12


def test_scale_genes_single_cell_is_nan_and_integer_triples_are_exact(dev, L):
    assert np.isnan(scale_genes(L, ss.scale_input(300, 1))).all()                         # C = 1: 0 / sqrt(0 / 1), as scale.default
    m, d = np.arange(3, 303, dtype=np.float64), 1.0 + np.arange(300, dtype=np.float64) % 7
    x = np.stack([m - d, m, m + d], axis=1)
    assert same_bits(scale_genes(L, x), np.tile([-1.0, 0.0, 1.0], (300, 1)))              # equality: mean m, sum of squares 2 d^2, scale d, all exact


def select_genes(L, x, keep):
    G, C = x.shape
    xd = to_dev(x)
    k = np.ascontiguousarray(keep, dtype=np.int32)
    out = torch.full((C, k.size), -777.0, dtype=torch.float64, device="cuda")
    assert L.icnv_select_genes_dev(vp(xd), G, C, k.ctypes.data_as(ct.POINTER(ct.c_int32)), k.size, vp(out), None) == 0
    torch.cuda.synchronize()
    return to_host(out)


def payload_matrix(G, C, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(G, C))
    u = x.view(np.uint64)
    where = rng.random((G, C)) < 0.05
    u[where] = np.uint64(0x7FF8000000000000) | rng.integers(1, 2 ** 32, size=int(where.sum())).astype(np.uint64)   # NaNs that carry a payload
    x[rng.random((G, C)) < 0.05] = -0.0
    return x


@pytest.mark.parametrize("case", ("identity", "reversed", "duplicates", "single", "g_out_255", "g_out_256", "g_out_257", "g_out_700", "wrap_8192"))
def test_select_genes_keep_lists_and_wrap_8192(dev, L, case):
    G, C = (6, 8195) if case == "wrap_8192" else (700, 37)
    x = payload_matrix(G, C, seed=len(case))
    rng = np.random.default_rng(3)
    keep = {"identity": np.arange(G), "reversed": np.arange(G)[::-1], "duplicates": np.array([5, 5, 699, 0, 5, 699, 130]),
            "single": np.array([431]), "g_out_255": rng.permutation(G)[:255], "g_out_256": rng.permutation(G)[:256],
            "g_out_257": rng.permutation(G)[:257], "g_out_700": rng.permutation(G), "wrap_8192": np.array([5, 0, 3, 3, 1])}[case]
    assert same_bits(select_genes(L, x, keep), x[keep])                                   # equality as uint64: NaN payloads and -0.0 count


# ================================================================== C. per-cell reductions
REDUCE_SHAPES = tuple((G, C) for G in ss.REDUCE_G for C in ss.REDUCE_C) + (ss.WRAP_8192,)


@pytest.mark.parametrize("shape", REDUCE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_col_sums_and_normalize_log2_tiles_and_wrap_8192(dev, shape):
    G, C = shape
    x = ss.position_coded(G, C)
    got = dev.col_sums(to_dev(x)).cpu().numpy()
    assert got.tolist() == [float(s) for s in ss.col_sums_int(x.astype(np.int64))]        # equality: integers below 2^53
    x = np.random.default_rng(G * 100 + C).lognormal(0.5, 0.8, size=(G, C))
    xd = to_dev(x)
    cs_t = dev.col_sums(xd)
    got = cs_t.cpu().numpy()
    want = ss.col_sums_fsum(x)
    assert (np.abs(got - want) <= np.array([ss.sum_bound(G, s) for s in want])).all()     # derived: G * 2^-53 * sum|x| (x > 0), any order
    f = ss.r_median(got)
    y10 = to_host(dev.normalize_log2(xd, col_sums_t=cs_t, normalize_factor=f, do_log2=False))
    assert same_bits(y10, ss.apply_counts(x, got, f, True, False))                        # equality: IEEE divide and multiply in R's order
    assert same_bits(to_host(dev.normalize_log2(xd, do_normalize=False, do_log2=False)), x)
    for dn in (False, True):
        y = to_host(dev.normalize_log2(xd, col_sums_t=cs_t, normalize_factor=f, do_normalize=dn, do_log2=True))
        assert np.abs(y - ss.apply_counts(x, got, f, dn, True)).max() < 1e-12             # the project's existing 1e-12 for this entry


BOUNDS_SHAPES = tuple((G, C) for G in ss.REDUCE_G for C in (1, 32)) + ((5, 8192), (3, 16384))


@pytest.mark.parametrize("shape", BOUNDS_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_average_bounds_exact_on_dyadic_values_nan_skipped_and_wrap_4096(dev, shape):
    """Multiples of 2^-20 below 2^10 and C a power of two: the long-double mean of the per-cell minima and maxima is exact, so
    the result must EQUAL the exact mean; 8 192 and 16 384 cells wrap the kernel's 4 096-block grid.  NaNs scattered in are
    skipped like quantile(na.rm = TRUE) does."""
    G, C = shape
    x = ss.dyadic(G, C, seed=G + C)
    assert dev.average_bounds(to_dev(x)) == ss.average_bounds(x)                          # equality: exact means
    if G > 1:
        rng = np.random.default_rng(G + C)
        y = x.copy()
        mask = rng.random((G, C)) < 0.3
        amin = int(np.argmin(x[:, 0]))
        keep_row = rng.integers(0, G, C)
        keep_row[0] = (amin + 1) % G
        mask[keep_row, np.arange(C)] = False                                              # (every cell keeps a value)
        mask[amin, 0] = True                                                              # the first cell's minimum is one of the skipped
        y[mask] = np.nan
        want = ss.average_bounds(y)
        assert not math.isnan(want[0]) and want != ss.average_bounds(x)
        assert dev.average_bounds(to_dev(y)) == want                                      # equality: exact means of the values that are not NaN


@pytest.mark.parametrize("shape", ((1, 1), (257, 32), (3, 16384)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_average_bounds_all_nan_cell_is_na_and_remove_outliers_passes_it_on(dev, shape):
    """R: quantile(na.rm = TRUE) of a cell of nothing but NaN is NA and so is the mean over the cells, for both bounds.
    The kernel leaves lo = +Inf, hi = -Inf for such a cell; the host's mean() turns that into NaN in its refinement pass
    (Inf - Inf), for one cell and for many.  With NA bounds R's two assignments assign nothing: icnv_remove_outliers_dev
    passes the NaN bounds on and copies the matrix (include/icnv.h)."""
    G, C = shape
    x = ss.dyadic(G, C, seed=7)
    x[:, C // 2] = np.nan
    if G > 1:
        x[1, 0] = np.nan
    lo, hi = dev.average_bounds(to_dev(x))
    assert math.isnan(lo) and math.isnan(hi)
    assert all(math.isnan(v) for v in ss.average_bounds(x))
    out, used = dev.remove_outliers(to_dev(x))
    assert math.isnan(used[0]) and math.isnan(used[1]) and same_bits(to_host(out), x)     # equality: nothing is assigned


@pytest.mark.parametrize("G", ss.MOMENTS_G, ids=lambda g: f"pair_loop_boundaries_G{g}")
def test_cells_moments_partial_all_genes_pair_loops_exact(dev, G):
    """block_cell_reduce_kernel's all-genes path on integers |v| <= 2^15: np = G / 2 pairs crosses the 1-wide / 4-wide / 8-wide
    loop boundaries at 768, 1024, 1792 and 2048 pairs; an odd G leaves one element over and starts the odd cells on an 8-byte
    boundary.  Seven listed cells of nine: unsorted, one listed twice, odd and even indices."""
    x = ss.moments_matrix(G, seed=G)
    xd = to_dev(x)
    cells = np.array(ss.MOMENTS_CELLS, dtype=np.int32)
    s, n = dev.cells_moments_partial(xd, cells, 0)
    assert (s, n) == (float(ss.int_moments(x, cells)), float(cells.size * G))             # equality: integers below 2^53
    for mean in (0.0, -3.0, 1217.0):
        s, n = dev.cells_moments_partial(xd, cells, 1, mean)
        assert (s, n) == (float(ss.int_moments(x, cells, int(mean))), float(cells.size * G))   # equality: integers below 2^53
    for phase in (0, 1):
        assert dev.cells_moments_partial(xd, np.zeros(0, np.int32), phase, 5.0) == (0.0, 0.0)  # n_cells = 0 contributes zeros


@pytest.fixture(scope="module")
def list_matrix(dev):
    x = ss.grid_values((ss.LIST_G, 9), seed=11)
    return x, to_dev(x)


def block_mean_sd(L, xd, G, C, genes, cells):
    out = (ct.c_double * 2)(-777.0, -777.0)
    g = np.ascontiguousarray(genes, dtype=np.int32)
    c = np.ascontiguousarray(cells, dtype=np.int32)
    assert L.icnv_block_mean_sd_dev(vp(xd), G, C, g.ctypes.data_as(ct.POINTER(ct.c_int32)), g.size, c.ctypes.data_as(ct.POINTER(ct.c_int32)),
                                    c.size, out, None) == 0
    return out[0], out[1]


@pytest.mark.parametrize("n_genes", ss.LIST_N_GENES, ids=lambda n: f"listed_{n}")
def test_block_mean_sd_gene_list_four_wide_loop(dev, L, list_matrix, n_genes):
    """The listed-genes path: its 4-wide loop runs from 769 genes on (j + 768 < n_genes); unsorted lists with repeats."""
    x, xd = list_matrix
    genes, cells = ss.gene_list(n_genes, seed=n_genes), np.array(ss.LIST_CELLS)
    vals = x[np.ix_(genes, cells)].ravel(order="F").tolist()
    want_mean, want_sd = ss.exact_mean_sd(vals, 24)
    mean, sd = block_mean_sd(L, xd, ss.LIST_G, 9, genes, cells)
    assert ss.ulp_distance(mean, want_mean) <= 1                                          # derived: exact sum (2^-24 grid), one long-double division rounded twice
    assert abs(sd - want_sd) <= ss.sd_bound(len(vals)) * want_sd                          # derived: sd_bound, (N + 8) * 2^-53 relative
    if n_genes == 1:
        mean, sd = block_mean_sd(L, xd, ss.LIST_G, 9, genes, [6])
        assert mean == x[genes[0], 6] and math.isnan(sd)                                  # one gene x one cell: sd() of one value is NA


@pytest.mark.parametrize("G", (3587, 10001), ids=lambda g: f"G{g}")
def test_cells_mean_sd_real_valued_all_genes(dev, G):
    """cells_mean_sd (the i3 HMM's mean and sd) on real-valued data through the 8-wide pair loop with the odd-G leftover.  The
    values lie on a 2^-24 grid around 1, so that the sum is exact and the mean's 1-ulp bound is the division's alone."""
    x = ss.grid_values((G, 9), seed=G)
    cells = np.array(ss.MOMENTS_CELLS, dtype=np.int32)
    want_mean, want_sd = ss.exact_mean_sd(x[:, cells].ravel(order="F").tolist(), 24)
    mean, sd = dev.cells_mean_sd(to_dev(x), cells)
    assert ss.ulp_distance(mean, want_mean) <= 1                                          # derived: exact sum, one long-double division rounded twice
    assert abs(sd - want_sd) <= ss.sd_bound(G * cells.size) * want_sd                     # derived: sd_bound


# ================================================================== D. elementwise kernels past one grid
BIG = (1031, 1019)


def test_remove_outliers_both_bounds_wraps_16_blocks_per_cu(dev, n_cu):
    G, C = BIG
    assert G * C > 16 * 256 * n_cu                                                        # more elements than one grid of the clamp holds
    rng = np.random.default_rng(16)
    x = rng.normal(0.0, 1.0, size=BIG)
    x[rng.random(BIG) < 0.01] = np.nan
    x[rng.random(BIG) < 0.01] = -0.0
    x[-1, -1], x[0, 0], x[-2, -1] = 9.0, -9.0, np.nan
    for lo, hi in ((-0.5, 0.75), (0.0, 0.0)):
        out, used = dev.remove_outliers(to_dev(x), lo, hi)
        assert used == (lo, hi)
        assert same_bits(to_host(out), ss.remove_outliers(x, lo, hi))                     # equality: R's two assignments; NaN passes, -0.0 is kept


@pytest.mark.parametrize("K", (3, 6))
def test_states_to_proxy_every_byte_value_class(dev, K):
    G, C = BIG
    rng = np.random.default_rng(K)
    st = rng.choice(np.array([0, 1, 2, 3, 4, 5, 6, 7, 255], dtype=np.uint8), size=BIG)
    st[-1, -1], st[0, 0], st[5, 5] = 255, 0, 7
    got = to_host(dev.states_to_proxy(to_dev(st, np.uint8), K))
    want = ss.states_to_proxy(st, K)
    assert same_values(got, want)                                                         # equality: a table
    assert np.isnan(got[np.isin(st, [0, 7, 255] + ([4, 5, 6] if K == 3 else []))]).all() and np.isnan(got).sum() == np.isnan(want).sum()


def test_gather_values_wraps_8192_blocks(dev, L):
    n = 8192 * 256 + 5
    x = payload_matrix(37, 11, seed=2)
    xd = to_dev(x)
    flat = x.ravel(order="F")
    off = np.random.default_rng(4).integers(0, flat.size, size=n).astype(np.int64)
    off[:4] = [0, flat.size - 1, 0, 0]
    off[-5:] = [flat.size - 1, 0, 17, 17, flat.size - 1]                                  # the five elements past the grid: first, last, repeats
    out = np.full(n, -777.0)
    assert L.icnv_gather_values_dev(vp(xd), flat.size, off.ctypes.data_as(ct.POINTER(ct.c_int64)), n,
                                    out.ctypes.data_as(ct.POINTER(ct.c_double)), None) == 0
    assert same_bits(out, flat[off])                                                      # equality: a gather
