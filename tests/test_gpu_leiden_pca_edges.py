"""The kernels of the PCA route of the Leiden subclustering (DESIGN K18; infercnv_amd/csrc/leiden_pca_kernels.hip) at their
edge shapes, each through its own device wrapper on synthetic mean / sd / V -- no trend fit, no eigh: block and tile edges,
one-stage and hundred-stage contractions, packed batches whose grids exceed a problem's own, permuted lists with a repeat,
the clips met with equality and by one ulp, padded matrices with NaN in the padding, empty and complete SNN graphs,
k = 1 and k = 128, and the refusals of a caller's CSR beyond the first problem and the first 256 rows.  The references
are tests/leiden_pca_restate.py and, for the Gram matrix, exact integer products; tests/test_leiden_pca_host.py shows on the
restatement alone that the inputs are the edge cases they are meant to be."""
import ctypes as ct

import numpy as np
import pytest

import leiden_pca_restate as pr
import leiden_restate as lr
from test_leiden_pca_host import GRAM_F, GRAM_N, RULER8, RULER9, gram_int_input, plant_scale_clips, shift_block, vstd_clip_case

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PAD = 64                                    # sentinel elements either side of a guarded output
SENT_F, SENT_I = -7.25e300, -0x5A5A5A5B


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infercnv_amd import device
    torch.cuda.set_device(0)
    device.init(0)
    return device


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(n, dtype):
    """(buffer, view): n elements with PAD sentinels either side."""
    buf = torch.full((n + 2 * PAD,), SENT_F if dtype.is_floating_point else SENT_I, dtype=dtype, device="cuda")
    return buf, buf[PAD:PAD + n]


def intact(buf):
    b = buf.cpu().numpy()
    s = np.asarray(SENT_F if b.dtype.kind == "f" else SENT_I, dtype=b.dtype)
    return bool(np.all(b[:PAD] == s) and np.all(b[-PAD:] == s))


def lists(dev, problems):
    """The HOST index lists of the C ABI: ((array, pointer) of gene_idx, gene_off, cell_idx, cell_off)."""
    from infercnv_amd import _lib
    gi, go = _lib.pack_groups([g for g, _ in problems])
    ci, co = _lib.pack_groups([c for _, c in problems])
    return _lib.i32(gi), _lib.i32(go), _lib.i32(ci), _lib.i32(co)


def expr(G, C, seed):
    """genes x cells."""
    return np.random.default_rng(seed).normal(1.0, 0.3, size=(G, C))


def padded_with_nan(X, extra=3):
    """The (cells, genes) device matrix as full[:, :G] of a wider tensor whose padding columns hold NaN."""
    G, C = X.shape
    full = torch.full((C, G + extra), float("nan"), dtype=torch.float64, device="cuda")
    full[:, :G] = cuda(X.T)
    return full[:, :G]


# ---------------------------------------------------------------------------------------------------- v_std
def synth_mean_sd(X, problems, seed, zero_every=50):
    """Any doubles will do for the kernel: a mean near the block's, an sd well below the spread (the sqrt(n) clip binds at
    small n), sd = 0 on some genes."""
    rng = np.random.default_rng(seed)
    means, sds = [], []
    for g, c in problems:
        sub = X[np.ix_(g, c)]
        means.append(sub.mean(axis=1) + rng.normal(0.0, 0.05, size=len(g)))
        sd = rng.uniform(0.05, 0.4, size=len(g))
        sd[zero_every - 1::zero_every] = 0.0
        sds.append(sd)
    return means, sds


def vstd_want(X, problems, means, sds):
    return np.concatenate([pr.v_std(X[np.ix_(g, c)], m, s) for (g, c), m, s in zip(problems, means, sds)])


def check_vstd(dev, x, X, problems, means, sds):
    got = dev.lpca_vstd(x, problems, cuda(np.concatenate(means)), cuda(np.concatenate(sds))).cpu().numpy()
    want = vstd_want(X, problems, means, sds)
    assert np.isfinite(got).all() and np.array_equal(got, want)
    return got, want


@pytest.mark.parametrize("n", [2, 3, 4])
def test_vstd_small_n_and_gene_counts_on_block_edges(dev, n):
    X = expr(300, 9, 100 + n)
    x = cuda(X.T)
    cells = np.arange(n) + 3
    clipped = 0
    for Gc in (1, 255, 256, 257):
        problems = [(np.arange(Gc) + 7, cells)]
        means, sds = synth_mean_sd(X, problems, Gc)
        check_vstd(dev, x, X, problems, means, sds)
        d = (X[np.ix_(*problems[0])] - means[0][:, None]) / np.where(sds[0] == 0, 1.0, sds[0])[:, None]
        clipped += int(np.count_nonzero(d > np.sqrt(float(n))))
    assert clipped > 100                                            # the clip binds all over these inputs
    # one batch of different gene counts and cell lists: lanes past a problem's genes, blocks past its last one
    problems = [(np.arange(1) + 299, cells), (np.arange(257), np.arange(n)), (np.arange(255) + 40, cells + 1),
                (np.arange(256) + 44, np.arange(n)[::-1] + 2)]
    means, sds = synth_mean_sd(X, problems, 9)
    got, _ = check_vstd(dev, x, X, problems, means, sds)
    assert np.count_nonzero(got == 0.0) == sum(len(g) // 50 for g, _ in problems)     # the sd = 0 genes and no other


def test_vstd_permuted_lists_with_a_repeat(dev):
    rng = np.random.default_rng(21)
    X = expr(300, 40, 22)
    genes, cells = rng.permutation(300)[:70], rng.permutation(40)[:9]
    genes[40], cells[7] = genes[5], cells[2]
    other = (rng.permutation(300)[:33], rng.permutation(40)[:4])
    problems = [(genes, cells), other]
    means, sds = synth_mean_sd(X, problems, 23)
    got, want = check_vstd(dev, cuda(X.T), X, problems, means, sds)
    rev = [(genes, cells[::-1].copy()), other]                      # the list order is the summation order
    assert not np.array_equal(vstd_want(X, rev, means, sds), want)
    check_vstd(dev, cuda(X.T), X, rev, means, sds)


def test_vstd_clip_met_with_equality_and_by_one_ulp(dev):
    X, mean, sd = vstd_clip_case()
    problems = [(np.arange(5), np.arange(4))]
    got, want = check_vstd(dev, cuda(X.T), X, problems, [mean], [sd])
    X2 = X.copy()
    X2[1, 2], X2[4, 3] = 1.0, 2.0
    assert np.array_equal(got, pr.v_std(X2, mean, sd))              # d one ulp above sqrt(n) and d = 30 both count as 2
    assert got[3] == 0.0 and got[2] > 1000.0 ** 2 / 3               # sd = 0; a large negative d is not clipped


def test_vstd_padded_matrix_and_guarded_output(dev):
    from infercnv_amd import _lib
    X = expr(70, 12, 31)
    problems = [(np.arange(33) + 20, np.arange(4) + 8), (np.arange(70), np.arange(12)), (np.arange(1), np.arange(2) + 10)]
    means, sds = synth_mean_sd(X, problems, 32, zero_every=16)
    xp = padded_with_nan(X)
    assert xp.stride(0) == 73 and bool(torch.isnan(xp.as_strided((12, 73), (73, 1))[:, 70:]).all())
    _, want = check_vstd(dev, xp, X, problems, means, sds)
    (gi, gp), (go, gop), (ci, cp), (co, cop) = lists(dev, problems)
    m, s = cuda(np.concatenate(means)), cuda(np.concatenate(sds))
    buf, out = guarded(want.size, torch.float64)
    _lib.check(_lib.load().icnv_lpca_vstd_dev(dev._ptr(xp), 70, 12, 73, gp, gop, cp, cop, 3, dev._ptr(m), dev._ptr(s), dev._ptr(out),
                                             dev._stream()))
    assert np.array_equal(out.cpu().numpy(), want) and intact(buf)


# ---------------------------------------------------------------------------------------------------- scale
def synth_scale(X, problems, seed):
    """Per problem (mean, var) of any doubles, the clips of plant_scale_clips planted into X (the problems' genes differ)."""
    rng = np.random.default_rng(seed)
    means, vs = [], []
    for g, c in problems:
        sub = X[np.ix_(g, c)]
        mean, var = sub.mean(axis=1) + rng.normal(0.0, 0.05, size=len(g)), rng.uniform(0.0005, 0.3, size=len(g))
        plant_scale_clips(X, mean, var, g, c)
        means.append(mean)
        vs.append(var)
    return means, vs


def check_scale(dev, x, X, problems, means, vs):
    """Every block at the offset lpca_z_layout gives: bit-equal to pr.scale, the padding column zero."""
    sd = cuda(np.concatenate([np.sqrt(v) for v in vs]))
    got = dev.lpca_scale(x, problems, cuda(np.concatenate(means)), sd).cpu().numpy()
    off, ldz = dev.lpca_z_layout([len(g) for g, _ in problems], [len(c) for _, c in problems])
    assert got.size == off[-1]
    wants = []
    for p, ((g, c), m, v) in enumerate(zip(problems, means, vs)):
        Z = got[off[p]:off[p + 1]].reshape(len(g), int(ldz[p]))
        want = pr.scale(X[np.ix_(g, c)], m, v)
        assert np.array_equal(Z[:, :len(c)], want) and not Z[:, len(c):].any() and ldz[p] == len(c) + len(c) % 2
        assert want[0, 0] == 10.0 and want[0, 1] == 10.0 and want.max() == 10.0
        if len(g) > 2:
            assert want[1, 0] == 10.0 and want[1, 1] == -2002.0 and not want[2].any()
        wants.append(want)
    return got, wants


@pytest.mark.parametrize("n", [2, 31, 32, 33, 63, 64, 65])
def test_scale_tile_edges(dev, n):
    X0 = expr(40, 70, 200 + n)
    for F in (1, 31, 32, 33):
        X = X0.copy()
        problems = [(np.arange(F) + 3, np.arange(n) + 2)]
        means, vs = synth_scale(X, problems, F)
        check_scale(dev, cuda(X.T), X, problems, means, vs)


def test_scale_batch_of_the_smallest_and_the_largest_shape_padded_and_guarded(dev):
    from infercnv_amd import _lib
    rng = np.random.default_rng(41)
    X = expr(80, 70, 42)
    problems = [(np.array([70]), np.array([69, 3])), (rng.permutation(33), rng.permutation(70)[:65]),
                (np.arange(32) + 33, np.arange(33) + 30), (np.arange(4) + 72, np.arange(2))]
    means, vs = synth_scale(X, problems, 43)
    got, _ = check_scale(dev, cuda(X.T), X, problems, means, vs)
    xp = padded_with_nan(X, extra=5)
    got_p, _ = check_scale(dev, xp, X, problems, means, vs)
    assert np.array_equal(got, got_p)
    (gi, gp), (go, gop), (ci, cp), (co, cop) = lists(dev, problems)
    m, s = cuda(np.concatenate(means)), cuda(np.concatenate([np.sqrt(v) for v in vs]))
    buf, out = guarded(got.size, torch.float64)
    _lib.check(_lib.load().icnv_lpca_scale_dev(dev._ptr(xp), 80, 70, 85, gp, gop, cp, cop, len(problems), dev._ptr(m), dev._ptr(s),
                                              dev._ptr(out), dev._stream()))
    assert np.array_equal(out.cpu().numpy(), got) and intact(buf)


# ---------------------------------------------------------------------------------------------------- Gram
def pack_z(blocks):
    """(F, n) blocks as icnv_lpca_scale_dev packs them: rows of ldz = n + (n & 1) doubles, the padding element 0."""
    out = []
    for Z in blocks:
        F, n = Z.shape
        P = np.zeros((F, n + (n & 1)))
        P[:, :n] = Z
        out.append(P.ravel())
    return np.concatenate(out)


@pytest.mark.parametrize("n", GRAM_N)
def test_gram_of_eighths_is_the_exact_integer_product(dev, n):
    """Z in eighths within [-2, 2]: every product and every partial sum in any order is exact (test_leiden_pca_host.py), so M
    is the int64 product / 64 to the bit -- a tile, stage or segment read or written at the wrong place cannot hide."""
    for F in GRAM_F:
        K, Z = gram_int_input(F, n, 7)
        M = dev.lpca_gram(cuda(pack_z([Z])), [F], [n]).cpu().numpy().reshape(F, F)
        assert np.array_equal(M, (K @ K.T) / 64.0), (F, n)
        assert np.array_equal(M, M.T)


def test_gram_batch_whose_tile_grid_exceeds_a_problems_own(dev):
    from infercnv_amd import _lib
    Fs, ns = [1, 129, 64], [33, 30, 64]                              # nt_max = 3: 9 tile slots, problems 0 and 2 own one
    KZ = [gram_int_input(F, n, 11) for F, n in zip(Fs, ns)]
    z = cuda(pack_z([Z for _, Z in KZ]))
    M = dev.lpca_gram(z, Fs, ns).cpu().numpy()
    m0 = 0
    for (K, _), F in zip(KZ, Fs):
        assert np.array_equal(M[m0:m0 + F * F].reshape(F, F), (K @ K.T) / 64.0)
        m0 += F * F
    assert M.size == m0
    buf, out = guarded(m0, torch.float64)
    (nf, nfp), (nc, ncp) = _lib.i32(Fs), _lib.i32(ns)
    _lib.check(_lib.load().icnv_lpca_gram_dev(dev._ptr(z), nfp, ncp, 3, dev._ptr(out), dev._stream()))
    assert np.array_equal(out.cpu().numpy(), M) and intact(buf)


@pytest.mark.parametrize("F,n", [(65, 33), (129, 4097)])
def test_gram_of_reals_within_the_contracts_bound(dev, F, n):
    """|M - ref| <= gamma_n sum |z_a z_b| (include/icnv.h), ref and the sum in extended precision: 64-bit significands, whose
    own error of about n 2^-64 sum |z_a z_b| is 2^-11 of the bound."""
    assert np.finfo(np.longdouble).nmant >= 63
    rng = np.random.default_rng([F, n])
    Z = 2.0 * rng.normal(size=(F, n))
    Z[rng.integers(0, F, 12), rng.integers(0, n, 12)] = 10.0         # a few entries at the clip
    M = dev.lpca_gram(cuda(pack_z([Z])), [F], [n]).cpu().numpy().reshape(F, F)
    assert np.array_equal(M, M.T)
    Zl = Z.astype(np.longdouble)
    ref = Zl @ Zl.T
    u = np.longdouble(2.0) ** -53
    bound = (n * u / (1 - n * u)) * (np.abs(Zl) @ np.abs(Zl).T)
    err = np.abs(M.astype(np.longdouble) - ref)
    ratio = float(np.max(err / bound))
    print(f"gram F={F} n={n}: max err / bound = {ratio:.4f}")
    assert np.all(err <= bound)


# ---------------------------------------------------------------------------------------------------- projection
def check_project(dev, Zs, Vs, e_ld):
    n_feat, n_cells, npcs = [Z.shape[0] for Z in Zs], [Z.shape[1] for Z in Zs], [V.shape[1] for V in Vs]
    v = cuda(np.concatenate([V.ravel() for V in Vs]))
    E = dev.lpca_project(cuda(pack_z(Zs)), v, n_feat, n_cells, npcs, e_ld).cpu().numpy()
    assert E.shape == (sum(n_cells), e_ld)
    r0 = 0
    for Z, V in zip(Zs, Vs):
        n, c = Z.shape[1], V.shape[1]
        assert np.array_equal(E[r0:r0 + n, :c], pr.project(Z, V)) and not E[r0:r0 + n, c:].any()
        r0 += n
    return E


@pytest.mark.parametrize("F", [1, 2, 2000])
def test_projection_cell_block_edges_and_few_components(dev, F):
    rng = np.random.default_rng(300 + F)
    for n in (1, 255, 256, 257, 513):
        Z = rng.normal(size=(F, n))
        V = rng.normal(size=(F, 10))
        for npcs in (1, 9, 10):
            check_project(dev, [Z], [np.ascontiguousarray(V[:, :npcs])], 10)


def test_projection_of_64_components_and_a_packed_batch(dev):
    from infercnv_amd import _lib
    rng = np.random.default_rng(51)
    check_project(dev, [rng.normal(size=(70, 257))], [rng.normal(size=(70, 64))], 64)
    Zs = [rng.normal(size=(2, 255)), rng.normal(size=(70, 1)), rng.normal(size=(37, 513))]
    Vs = [rng.normal(size=(2, 1)), rng.normal(size=(70, 10)), rng.normal(size=(37, 4))]
    E = check_project(dev, Zs, Vs, 10)
    z, v = cuda(pack_z(Zs)), cuda(np.concatenate([V.ravel() for V in Vs]))
    (nf, nfp), (nc, ncp), (npc, npp) = _lib.i32([2, 70, 37]), _lib.i32([255, 1, 513]), _lib.i32([1, 10, 4])
    buf, out = guarded(E.size, torch.float64)
    _lib.check(_lib.load().icnv_lpca_project_dev(dev._ptr(z), dev._ptr(v), nfp, ncp, npp, 3, dev._ptr(out), 10, dev._stream()))
    assert np.array_equal(out.cpu().numpy().reshape(E.shape), E) and intact(buf)


# ---------------------------------------------------------------------------------------------------- kNN as the route calls it
def embedding(n, seed):
    """An (n, 10) matrix with identical rows (n >= 3: rows 0 and n - 1, and a run of three at n = 65)."""
    E = np.random.default_rng(seed).normal(size=(n, 10))
    if n >= 3:
        E[n - 1] = E[0]
    if n >= 65:
        E[40] = E[41] = E[17]
    return E


@pytest.mark.parametrize("npcs", [1, 2, 9])
def test_knn_over_the_first_components_of_an_embedding(dev, npcs):
    from infercnv_amd import _lib
    Es = [embedding(n, 60 + n) for n in (2, 3, 65)]
    E = np.concatenate(Es)
    e = cuda(E)
    comps = np.arange(npcs, dtype=np.int32)
    rows = np.concatenate([[0], np.cumsum([len(x) for x in Es])])
    for p, (Ep, k) in enumerate(zip(Es, (2, 3, 8))):                # every problem alone, k up to n
        nn, _ = dev.knn(e, [(comps, np.arange(rows[p], rows[p + 1], dtype=np.int32))], k)
        want = pr.knn(Ep[:, :npcs], k)
        assert np.array_equal(nn.cpu().numpy(), want)
        if len(Ep) >= 3:
            assert want[len(Ep) - 1, 0] == 0 and want[0, 1] == len(Ep) - 1     # identical rows: the tie goes by position
    problems = [(np.arange(c, dtype=np.int32), np.arange(rows[p], rows[p + 1], dtype=np.int32)) for p, c in enumerate((npcs, 1, 9))]
    nn, dist = dev.knn(e, problems, 2)                                # one batch, a component count per problem, one k
    want = np.concatenate([pr.knn(Ep[:, :c], 2) for Ep, c in zip(Es, (npcs, 1, 9))])
    assert np.array_equal(nn.cpu().numpy(), want)
    (gi, gp), (go, gop), (ci, cp), (co, cop) = lists(dev, problems)
    bi, oi = guarded(70 * 2, torch.int32)
    bd, od = guarded(70 * 2, torch.float64)
    _lib.check(_lib.load().icnv_knn_dev(dev._ptr(e), 10, 70, gp, gop, cp, cop, 3, 2, dev._ptr(oi), dev._ptr(od), dev._stream()))
    assert np.array_equal(oi.cpu().numpy().reshape(70, 2), want) and np.array_equal(od.cpu().numpy(), dist.cpu().numpy().ravel())
    assert intact(bi) and intact(bd)


# ---------------------------------------------------------------------------------------------------- SNN
def snn_want(nns):
    """pr.snn of every block as one CSR over the batch."""
    offs, parts, e0 = [], [[], [], [], []], 0
    for nn in nns:
        off, col, shared, weight, loop = pr.snn(nn)
        offs.append(off[:-1] + e0)
        for lst, a in zip(parts, (col, shared, weight, loop)):
            lst.append(a)
        e0 += col.size
    offs.append(np.array([e0], dtype=np.int64))
    return [np.concatenate(offs)] + [np.concatenate(p) for p in parts]


def check_snn(dev, nns):
    got = [a.cpu().numpy() for a in dev.snn_jaccard(cuda(np.concatenate(nns)), [len(nn) for nn in nns])]
    for g, w in zip(got, snn_want(nns)):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    return got


def test_snn_empty_graphs(dev):
    """Every row keeps nothing: nnz = 0 and the fill pass has nothing to launch; then the same block between two others."""
    from test_gpu_leiden_pca import hub_block
    for n in (100, 89):
        got = check_snn(dev, [shift_block(n, RULER9)])
        assert got[1].size == 0 and not got[0].any() and got[4].all()
    got = check_snn(dev, [hub_block(21, 9, 1), shift_block(100, RULER9), hub_block(70, 9, 2)])
    assert got[0][21] == got[0][121] > 0 and got[1].size > got[0][21]
    for nn in (np.array([[0]]), np.array([[0], [1], [2]])):           # k = 1, every node its own neighbour
        got = check_snn(dev, [nn.astype(np.int32)])
        assert got[1].size == 0


def test_snn_prune_rule_at_equality_complete_graph_and_k_of_1_and_128(dev):
    got = check_snn(dev, [shift_block(100, RULER8)])
    assert np.array_equal(np.diff(got[0]), np.full(100, 56)) and np.all(got[2] == 1)
    got = check_snn(dev, [shift_block(5, range(5))])                  # n = k
    assert got[1].size == 20 and np.all(got[2] == 5) and np.all(got[3] == 1 << 24)
    got = check_snn(dev, [np.array([[1], [1], [0]], dtype=np.int32)])  # k = 1: d = 2 k - s = 1
    assert got[1].tolist() == [1, 0] and got[3].tolist() == [1 << 24] * 2
    got = check_snn(dev, [shift_block(128, range(128))])              # k = 128 = LEIDEN_MAX_K
    assert got[1].size == 16256 and np.all(got[2] == 128)
    got = check_snn(dev, [shift_block(129, range(128))])
    assert got[1].size == 16512 and np.all(got[2] == 127)


@pytest.mark.parametrize("n", [63, 64, 65, 66, 129, 130])
def test_snn_hub_rows_around_one_and_two_wavefronts(dev, n):
    """Node 0 is in every row: its transposed list has n entries, its kept row n - 1."""
    from test_gpu_leiden_pca import hub_block
    nn = hub_block(n, 8, n)
    got = check_snn(dev, [nn])
    assert got[0][1] - got[0][0] == n - 1
    if n == 130:                                                      # the atomics' order must not show
        again = [a.cpu().numpy() for a in dev.snn_jaccard(cuda(nn), [n])]
        assert all(np.array_equal(a, b) for a, b in zip(got, again))


def test_snn_batch_of_300_tiny_problems_and_guarded_outputs(dev):
    from infercnv_amd import _lib
    rng = np.random.default_rng(71)
    nns = [rng.integers(0, 1 + p % 7, size=(1 + p % 7, 1)).astype(np.int32) for p in range(300)]
    got = check_snn(dev, nns)
    assert got[1].size > 300
    L = _lib.load()
    t = cuda(np.concatenate(nns))
    tn, nnz = t.shape[0], got[1].size
    off, offp = _lib.i32(np.concatenate([[0], np.cumsum([len(nn) for nn in nns])]))
    h, cnt = ct.c_void_p(0), ct.c_int64(-1)
    _lib.check(L.icnv_snn_begin_dev(dev._ptr(t), 1, offp, 300, ct.byref(h), ct.byref(cnt), dev._stream()))
    try:
        assert cnt.value == nnz
        bufs = [guarded(m, dt) for m, dt in ((tn + 1, torch.int64), (nnz, torch.int32), (nnz, torch.int32), (nnz, torch.int64),
                                             (tn, torch.int32))]
        _lib.check(L.icnv_snn_fill_dev(h, *[dev._ptr(v) for _, v in bufs], dev._stream()))
    finally:
        L.icnv_snn_end(h)
    for (buf, view), g in zip(bufs, got):
        assert np.array_equal(view.cpu().numpy(), g) and intact(buf)


def test_snn_refuses_a_row_that_repeats_an_entry(dev):
    """N(i) is a set (include/icnv.h): ICNV_ERR_ARG from the device check, no handle, nnz untouched.  Such rows are sent only
    to a library that carries the check: the rows kernel is not defined on them."""
    from infercnv_amd import IcnvError, _lib
    from test_gpu_leiden_pca import hub_block
    with open(_lib.LIB_PATH, "rb") as f:
        assert b"snn: an nn_idx row repeats an entry" in f.read(), "this library has no check for repeated entries"
    L = _lib.load()
    big = shift_block(300, RULER8)
    big[270, 5] = big[270, 3]
    own = shift_block(300, RULER8)
    own[299, 7] = own[299, 0]                                         # the node itself, twice
    for nns in ([hub_block(21, 8, 3), big], [own], [np.array([[0, 0], [1, 0]], dtype=np.int32)]):
        t = cuda(np.concatenate(nns))
        with pytest.raises(IcnvError) as e:
            dev.snn_jaccard(t, [len(nn) for nn in nns])
        assert e.value.code == _lib.ERR_ARG and "repeats an entry" in str(e.value)
        with pytest.raises(ValueError, match="repeats an entry"):
            pr.snn(nns[-1])
        off, offp = _lib.i32(np.concatenate([[0], np.cumsum([len(nn) for nn in nns])]))
        h, cnt = ct.c_void_p(0), ct.c_int64(-1)
        rc = L.icnv_snn_begin_dev(dev._ptr(t), t.shape[1], offp, len(nns), ct.byref(h), ct.byref(cnt), dev._stream())
        assert rc == _lib.ERR_ARG and h.value is None and cnt.value == -1
    check_snn(dev, [hub_block(21, 8, 3), shift_block(300, RULER8)])   # the same batch without the repeat


def test_k11_graph_is_defined_on_a_repeated_entry(dev):
    """K11's contract is on membership (edge {i, j} iff j is in row i or i in row j): a repeated entry changes nothing."""
    nn = shift_block(70, RULER8)
    nn[33, 5] = nn[33, 3]
    nn[69, 7] = nn[69, 0]
    got = [a.cpu().numpy() for a in dev.snn_graph(cuda(nn), [70])]
    for g, w in zip(got, lr.snn_graph(nn)):
        assert np.array_equal(g, w)


# ---------------------------------------------------------------------------------------------------- a caller's CSR
@pytest.fixture(scope="module")
def two_graphs():
    """Two valid graphs as one CSR: 21 nodes, then 300 nodes with 56 entries a row."""
    from test_gpu_leiden_pca import hub_block
    off, col, shared, weight, loop = snn_want([hub_block(21, 5, 4), shift_block(300, RULER8)])
    return dict(row_off=off, col=col, weight=weight, loop=loop, sizes=[21, 300])


def run_graph(dev, g, **changed):
    a = {k: cuda(changed.get(k, g[k])) for k in ("row_off", "col", "weight", "loop")}
    return dev.leiden_graph(a["row_off"], a["col"], a["weight"], a["loop"], g["sizes"], "CPM", 0.05 * pr.ONE, 0.01, 2, 3, [5, 6])


def test_leiden_graph_accepts_the_valid_batch_and_guards_its_output(dev, two_graphs):
    from infercnv_amd import _lib
    g = two_graphs
    memb, ncl = run_graph(dev, g)
    memb = memb.cpu().numpy()
    r0 = 0
    for p, n in enumerate(g["sizes"]):
        o = g["row_off"][r0:r0 + n + 1]
        sl = slice(int(o[0]), int(o[-1]))
        want, K = pr.leiden_graph(o - o[0], g["col"][sl], g["weight"][sl], g["loop"][r0:r0 + n], lr.CPM, 0.05 * pr.ONE, 0.01, 2, seed=3,
                                  token=5 + p)
        assert int(ncl[p]) == K and np.array_equal(memb[r0:r0 + n], want)
        r0 += n
    a = [cuda(g[k]) for k in ("row_off", "col", "weight", "loop")]
    buf, out = guarded(321, torch.int32)
    (off, offp), (res, rp) = _lib.i32([0, 21, 321]), _lib.f64([0.05 * pr.ONE] * 2)
    tok = np.array([5, 6], dtype=np.uint64)
    got_ncl = np.zeros(2, dtype=np.int32)
    _lib.check(_lib.load().icnv_leiden_graph_dev(*[dev._ptr(t) for t in a], pr.ONE, offp, 2, _lib.LEIDEN_CPM, rp, 0.01, 2, 3,
                                                tok.ctypes.data_as(ct.POINTER(ct.c_uint64)), dev._ptr(out),
                                                got_ncl.ctypes.data_as(_lib._ip), dev._stream()))
    assert np.array_equal(out.cpu().numpy(), memb) and np.array_equal(got_ncl, ncl) and intact(buf)


@pytest.mark.parametrize("defect", ["own node", "equal neighbours", "descending pair", "weight above 2^62"])
def test_leiden_graph_refuses_a_defect_in_the_second_problem_past_row_256(dev, two_graphs, defect):
    from infercnv_amd import IcnvError, _lib
    g = two_graphs
    col, weight = g["col"].copy(), g["weight"].copy()
    row = {"own node": 270, "equal neighbours": 280, "descending pair": 290, "weight above 2^62": 299}[defect]
    t0, t1 = int(g["row_off"][21 + row]), int(g["row_off"][21 + row + 1])
    assert row >= 256 and t1 - t0 == 56
    if defect == "own node":
        t = t0 + int(np.searchsorted(col[t0:t1], row))              # the first column above the node ...
        assert t0 < t < t1 and col[t - 1] < row < col[t]
        col[t] = row                                                  # ... becomes the node: the row stays ascending
        assert np.all(np.diff(col[t0:t1]) > 0)
    elif defect == "equal neighbours":
        col[t0 + 31] = col[t0 + 30]
    elif defect == "descending pair":
        col[t0 + 30], col[t0 + 31] = col[t0 + 31], col[t0 + 30]
    else:
        weight[t1 - 1] = (1 << 62) + 1
    with pytest.raises(IcnvError) as e:
        run_graph(dev, g, col=col, weight=weight)
    assert e.value.code == _lib.ERR_ARG
