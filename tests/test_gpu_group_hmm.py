"""The kernels every group-level HMM call goes through (-m gpu) -- group_partial_sums_kernel<false / true>,
group_means_finish_kernel, reduce_moments_kernel, i3_params_kernel, broadcast_states_kernel<KEEP>, state_consensus_kernel,
states_to_proxy_kernel of viterbi_kernels.hip -- at their edge shapes, against tests/group_hmm_restate.py (tied to independent
references by tests/test_group_hmm_host.py).

Shapes: G in {1, 255, 256, 257, 512, 513} (one gene; one short of, exactly and one past a 256-gene tile; two tiles and the
16-byte broadcast; three tiles), groups of 1, 2, 3, 63, 64, 65 and 129 cells (below, at and above the 64 slices; odd and even
for the two-cell loops and their tail), and every call at the highest split count (64: few groups) and at split count 1
(filler groups of one cell until tiles * n_grp >= 2048).

Every tolerance is equality (bits of a correctly rounded mean; integer moments; tables) or a bound derived where it is used.
"""
import functools
import math
import statistics

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import group_hmm_restate as gh  # noqa: E402
import oracle_np as onp  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infercnv_amd import device
    torch.cuda.set_device(0)
    device.init(0)
    return device


def to_dev(x_gc, dtype=np.float64):
    return torch.from_numpy(np.array(np.asarray(x_gc, dtype=dtype).T, order="C")).cuda()   # (a copy: the cached inputs are read-only)


def to_host(t_cg):
    return t_cg.cpu().numpy().T


def fillers_for_one_slice(G, n_groups):
    """How many one-cell groups to add so that group_means_nsplit gives 1."""
    tiles = (G + 255) // 256
    n = -(-2048 // tiles) - n_groups
    assert gh.nsplit(G, n_groups + n) == 1 and gh.nsplit(G, n_groups) == 64
    return n


# ================================================================== a. correctly rounded group means
MEANS_G = (1, 255, 256, 257, 513)


@functools.lru_cache(maxsize=None)
def means_case(G):
    n_fill = fillers_for_one_slice(G, len(gh.MEAN_SIZES))
    groups, rest = gh.mean_groups(seed=G, extra=n_fill)
    C = sum(gh.MEAN_SIZES) + n_fill
    x = gh.means_matrix(G, groups, C, seed=G)
    want = gh.exact_group_means(x, groups)
    x.setflags(write=False)
    want.setflags(write=False)
    return x, groups, [np.array([c], dtype=np.int32) for c in rest], want


def assert_same_bits(got, want):
    diff = gh.bits(got) != gh.bits(want)
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:5].tolist())


@pytest.mark.parametrize("G", MEANS_G, ids=lambda g: f"G{g}")
def test_group_means_correctly_rounded_at_every_split_count(dev, G):
    """The kernel comment's contract: the correctly rounded mean, whatever the split of a group's cells into slices and
    whatever their order.  Inputs on which double-double arithmetic can keep that promise: sum |x| / |sum x| below 2^40 for
    every (gene, group) -- the cap -- and, since a mean may sit arbitrarily close to a rounding boundary, no mean closer to
    one than the arithmetic's own loss (gh.dd_margin_needed, derived there); both are checked here on the CPU first."""
    x, groups, fillers, want = means_case(G)
    for g in range(G):
        for cells in groups:
            assert gh.cancellation_ratio(x[g, cells]) < 2.0 ** 40                          # the cancellation cap
            assert gh.gene_group_ok(x[g, cells])                                           # the cap again, and the margin where one is needed
    xd = to_dev(x)
    calls = [groups, groups + fillers]                                                     # 64 slices (most of them empty for the small groups); one slice
    if G == 513:
        calls.insert(1, groups + fillers[:33])
        assert gh.nsplit(G, 40) == 18
    rng = np.random.default_rng(G)
    for call in calls:
        for shuffle in (False, True):
            listed = [rng.permutation(c) if shuffle else c for c in call]
            got = to_host(dev.group_means(xd, listed))
            assert_same_bits(got[:, :len(groups)], want)                                   # equality: one correctly rounded result
            if len(call) > len(groups):
                assert_same_bits(got[:, len(groups):], x[:, np.concatenate(call[len(groups):])])   # a group of one cell: the cell


# ================================================================== b. non-finite inputs
def test_group_means_non_finite_inputs_follow_rowmeans(dev):
    """The third accumulator (the plain sum) and plain / n: NaN for a NaN or both infinities, the signed infinity otherwise,
    in groups of odd and even size, at 64 slices and at one; every other (gene, group) keeps its bits."""
    G = 257
    x0, groups, fillers, want0 = means_case(G)
    x = x0.copy()
    by_size = {len(c): c for c in groups}
    inf, nan = math.inf, math.nan
    plants = [  # (gene, group size, positions in the group's list, values)
        (0, 65, (64,), (nan,)), (1, 64, (0,), (inf,)), (2, 3, (1,), (-inf,)), (3, 129, (0, 2), (inf, -inf)), (4, 129, (0, 1), (inf, -inf)),
        (5, 129, (5, 100), (-inf, inf)), (6, 2, (0, 1), (nan, inf)), (7, 1, (0,), (inf,)), (8, 1, (0,), (nan,)), (9, 64, (10, 63), (-inf, -inf)),
        (255, 65, (3,), (inf,)), (256, 63, (62,), (-inf,)), (256, 129, (128,), (nan,)), (10, 2, (1,), (-inf,)), (11, 63, (0, 31), (inf, nan))]
    for gene, size, where, vals in plants:
        x[gene, by_size[size][list(where)]] = vals
    genes = sorted({p[0] for p in plants})
    want = want0.copy()
    want[genes] = gh.exact_group_means(x[genes], groups)
    assert np.isnan(want).sum() == 8 and np.isposinf(want).sum() == 3 and np.isneginf(want).sum() == 4
    xd = to_dev(x)
    for call in (groups, groups + fillers):
        got = to_host(dev.group_means(xd, call))[:, :len(groups)]
        assert np.array_equal(np.isnan(got), np.isnan(want))
        finite_or_inf = ~np.isnan(want)
        assert_same_bits(got[finite_or_inf], want[finite_or_inf])                          # equality: the infinities' signs and every untouched mean


# ================================================================== c-f. the plan: moments, parameters, states, broadcast
# (cells, how the group's cells are flagged as reference cells)
LAYOUT = ((1, "all"), (2, "all"), (3, "mixed, tail flagged"), (64, "none"), (65, "mixed, tail not flagged"), (129, "mixed, tail flagged"),
          (64, "mixed"), (65, "all"), (1, "none"), (129, "mixed, tail not flagged"))
LOOSE = 5                                                                                  # cells in no group
PLAN_G = (1, 257, 512)
PLAN_CASES = [(G, fill) for G in PLAN_G for fill in (False, True)]
Z = abs(statistics.NormalDist().inv_cdf(0.05))


@functools.lru_cache(maxsize=None)
def plan_layout(G, fill):
    """Groups, reference cells and loose cells over a permutation of the cells.  `fill` adds one-cell groups until the plan's
    split count is 1; every seventh of them is a reference cell (a group of one reference cell), the others are not."""
    sizes = [s for s, _ in LAYOUT]
    n_fill = fillers_for_one_slice(G, len(LAYOUT)) if fill else 0
    C = sum(sizes) + LOOSE + n_fill
    rng = np.random.default_rng([G, int(fill)])
    perm = rng.permutation(C).astype(np.int32)
    groups, ref, at = [], [], 0
    for size, how in LAYOUT:
        cells = perm[at:at + size]
        at += size
        if how == "all":
            flag = np.ones(size, dtype=bool)
        elif how == "none":
            flag = np.zeros(size, dtype=bool)
        else:
            flag = rng.random(size) < 0.5
            flag[0], flag[1] = True, False                                                 # mixed whatever the draw
            if "tail" in how:
                flag[-1] = "not" not in how
        groups.append(cells)
        ref.extend(cells[flag].tolist())
    loose = perm[at:at + LOOSE]
    at += LOOSE
    for i in range(n_fill):
        groups.append(perm[at + i:at + i + 1])
        if i % 7 == 0:
            ref.append(int(perm[at + i]))
    ref = rng.permutation(np.array(ref, dtype=np.int32))
    chr_start = np.array([0, G] if G == 1 else [0, 100, G], dtype=np.int32)
    assert len(groups) * (chr_start.size - 1) <= 8192                                      # the plan's limit on (group, chromosome) sequences
    ns = gh.nsplit(G, len(groups))
    assert ns == (1 if fill else 64)
    largest_slice = max(-(-len(c) // ns) for c in groups)
    return C, groups, ref, loose, chr_start, largest_slice


@functools.lru_cache(maxsize=None)
def plan_data(G, fill, real):
    C, groups, ref, _, _, _ = plan_layout(G, fill)
    if real:
        x = 1.0 + 0.1 * np.random.default_rng([G, int(fill), 1]).standard_normal((G, C))
    else:
        x = gh.integer_matrix(G, C, seed=G + int(fill))
        if G > 1:   # a gained and a lost stretch in some groups, so that the states differ: still integers, -8 .. 11
            for q, cells in enumerate(groups[:len(LAYOUT)]):
                if q % 3 == 1:
                    x[30:80, cells] += 5.0
                elif q % 3 == 2:
                    x[150:220, cells] -= 5.0
    x.setflags(write=False)
    return x, gh.exact_moments(x, ref)


@pytest.mark.parametrize("G,fill", PLAN_CASES)
def test_plan_moments_exact_on_integers_for_every_group_kind(dev, G, fill):
    """group_partial_sums_kernel<true>: the loops for groups without, of only, and with some reference cells, and the odd
    cell behind them, on small integers (gh.integer_matrix, some stretches shifted by 5): S1, S2 and n are integers below 2^53
    and every partial sum is exact in any order."""
    C, groups, ref, loose, cs, _ = plan_layout(G, fill)
    x, (S1, S2, n, _, _) = plan_data(G, fill, False)
    assert n == ref.size * G and S2 < 2 ** 53 and S1.denominator == 1 and S2.denominator == 1
    xd = to_dev(x)
    plan = dev.GroupHMMPlan(G, C, cs, groups, ref)
    try:
        first = plan.i3_partial(xd).cpu().tolist()
        assert first == [float(S1), float(S2), float(ref.size * G)], (first, float(S1), float(S2))   # equality: exact integers
        second = plan.i3_partial(xd).cpu().tolist()
        assert second == first                                                             # nothing stale, nothing added twice
    finally:
        plan.close()


@pytest.mark.parametrize("G,fill", PLAN_CASES)
def test_plan_moments_bounded_on_real_values(dev, G, fill):
    """The same layouts on 1 + 0.1 N(0, 1).  x - 1 is exact for x in [0.5, 2] (Sterbenz), so a lane's S1 is a recursive sum of at
    most L exact terms, L the largest slice of any group: at most (L - 1) u sum |d| over the lane's terms (first order).  The lanes
    are then added in six shuffle steps and two additions from LDS, each losing at most u times the sum of the |d| below it:
    8 u sum |d| over everything.  The workgroups' values are added in double-double (u^2) and the pair is rounded once: u.  That
    is (L + 8) u sum |d|; the issue's L + 16 leaves room for the second-order terms.  S2 adds one rounding per term, the
    product inside the fma (the fma rounds d * d + s2 once, the first one rounds d * d): L + 17."""
    C, groups, ref, loose, cs, L = plan_layout(G, fill)
    x, (S1, S2, n, A1, A2) = plan_data(G, fill, True)
    assert x.min() >= 0.5 and x.max() <= 2.0 and L == (129 if fill else 3)
    plan = dev.GroupHMMPlan(G, C, cs, groups, ref)
    try:
        m3 = plan.i3_partial(to_dev(x)).cpu().tolist()
    finally:
        plan.close()
    e1, e2 = abs(m3[0] - float(S1)), abs(m3[1] - float(S2))
    b1, b2 = (L + 16) * gh.U * A1, (L + 17) * gh.U * A2
    print(f"G={G} fill={fill}: |S1 err| {e1:.3e} (bound {b1:.3e}), |S2 err| {e2:.3e} (bound {b2:.3e})")
    # (float(S1) is itself rounded: half an ulp of S1, far below u * A1 / 2; covered by the slack)
    assert e1 <= b1 and e2 <= b2 and m3[2] == ref.size * G


@pytest.mark.parametrize("delta_abs", (None, 3.0), ids=("delta_from_z", "delta_given"))
@pytest.mark.parametrize("G,fill", PLAN_CASES)
def test_plan_i3_parameters_states_and_broadcast(dev, G, fill, delta_abs):
    """On the integer plans S1, S2 and n reach i3_params_kernel exact, so its results are held to the mathematics:
      mu = 1 + S1 / n: one division, one addition, u (|mu - 1| + |mu|) <= 2^-52 max(1, |mu|) for |mu - 1| <= |mu|;
      sigma: S1^2 exact (below 2^53), S1^2 / n one rounding, amplified by (kappa - 1) in the subtraction, which rounds once, as
      does the division by n - 1: (kappa + 1) u on the variance, half of it on sigma, plus the square root's u:
      ((kappa + 1) / 2 + 1) u <= (kappa + 2) u;
      delta = sigma z, one multiplication of the kernel's own sigma, or delta_abs itself.
    The states then equal viterbi_groups' under the plan's own parameters (its group means and broadcast, bit for bit), every
    member cell has its group's states, every loose cell 255, and nothing of a caller's buffer survives."""
    C, groups, ref, loose, cs, _ = plan_layout(G, fill)
    x, (S1, S2, n, _, _) = plan_data(G, fill, False)
    kappa = gh.sigma_condition(S1, S2, n)
    assert 1.0 <= kappa <= 4.0                                                             # the cap that keeps the sigma bound meaningful
    mu_w, sigma_w, delta_w, _ = gh.i3_params(S1, S2, n, Z, delta_abs)
    assert abs(mu_w - 1.0) <= abs(mu_w)
    xd = to_dev(x)
    Pi3, d3 = onp.get_HMM_i3(1e-6)
    states = torch.full((C, G), 0x77, dtype=torch.uint8, device=xd.device)
    plan = dev.GroupHMMPlan(G, C, cs, groups, ref)
    try:
        plan.i3_partial(xd)
        out = plan.i3_finish(np.log(Pi3), np.log(d3), Z, delta_abs=delta_abs, states=states)
        mu, sigma, delta = plan.i3_params()
    finally:
        plan.close()
    assert out is states
    assert abs(mu - mu_w) <= 2.0 ** -52 * max(1.0, abs(mu_w)), (mu, mu_w)
    assert abs(sigma - sigma_w) <= (kappa + 2.0) * gh.U * sigma_w, (sigma, sigma_w, kappa)
    assert delta == (sigma * Z if delta_abs is None else delta_abs)                        # equality: the same single multiplication
    want, _ = dev.viterbi_groups(xd, cs, groups, np.array([mu - delta, mu, mu + delta]), [sigma] * len(groups), np.log(Pi3), np.log(d3))
    assert torch.equal(states, want), int((states != want).sum())
    st = to_host(states)
    assert (st[:, loose] == 255).all()
    member = np.concatenate(groups)
    assert np.isin(st[:, member], (1, 2, 3)).all()                                         # the sentinel is gone from every byte
    for cells in groups:
        assert (st[:, cells] == st[:, cells[:1]]).all()                                    # one column per group
    if G > 1:
        assert len(np.unique(st[:, member])) >= 2                                         # the Viterbi had something to decide


@pytest.mark.parametrize("G", (257, 512), ids=("G257_bytes", "G512_16_byte_words"))
def test_state_consensus_overwrite_keeps_cells_in_no_group(dev, G):
    """broadcast_states_kernel<true> behind state_consensus(overwrite=True): member cells get the consensus, the others keep
    their states; both copy loops."""
    C, groups, _, loose, _, _ = plan_layout(G, False)
    rng = np.random.default_rng(G)
    st = rng.choice(np.array([1, 2, 3, 4, 5, 6, 255], dtype=np.uint8), size=(G, C))
    want = gh.consensus(st, groups)
    cons, out = dev.state_consensus(to_dev(st, np.uint8), groups, overwrite=True)
    assert np.array_equal(to_host(cons), want)
    got = to_host(out)
    assert np.array_equal(got[:, loose], st[:, loose]) and loose.size == LOOSE
    for q, cells in enumerate(groups):
        assert (got[:, cells] == want[:, q:q + 1]).all()


# ================================================================== g. consensus ties and limits
# (the group's states, the winner by R's rule): ties go to the smallest value present, -1 (255) before every state
CONSENSUS_GROUPS = (
    ([255] * 255, 255),                                   # all -1
    ([255, 1], 255),                                      # -1 ties with state 1
    ([4] * 128 + [3] * 128, 3),                           # states 3 and 4 tie
    ([6, 5, 4, 3, 2, 1] * 42 + [255] * 3, 1),             # 255 cells: a six-way tie above three -1
    ([5], 5),                                             # one cell
    ([6] * 129 + [1] * 128, 6),                           # 257 cells: a strict majority of the last state
    ([255] * 128 + [2] * 128, 255),                       # 256 cells: -1 ties with a state
    ([1] * 127 + [255] * 128, 255),                       # -1 wins outright
    ([6, 6], 6),
    ([2, 1, 2, 1, 6, 6], 1),                              # a three-way tie without -1
)


@pytest.mark.parametrize("G", (1, 257))
def test_state_consensus_ties_invalid_state_and_group_sizes(dev, G):
    sizes = [len(v) for v, _ in CONSENSUS_GROUPS]
    assert {1, 2, 255, 256, 257} <= set(sizes)
    C = sum(sizes)
    perm = np.random.default_rng(G).permutation(C).astype(np.int32)
    st = np.empty((G, C), dtype=np.uint8)
    groups, at = [], 0
    for vals, _ in CONSENSUS_GROUPS:
        cells = perm[at:at + len(vals)]
        at += len(vals)
        groups.append(cells)
        for g in range(G):
            st[g, cells] = np.roll(vals, 7 * g)                                            # the same multiset in another order on every gene
    want = np.repeat(np.array([[w for _, w in CONSENSUS_GROUPS]], dtype=np.uint8), G, axis=0)
    assert np.array_equal(gh.consensus(st, groups), want)
    assert np.array_equal(to_host(dev.state_consensus(to_dev(st, np.uint8), groups)), want)


def test_state_consensus_group_count_limit(dev):
    from infercnv_amd import _lib
    rng = np.random.default_rng(9)
    st = rng.choice(np.array([1, 2, 3, 4, 5, 6, 255], dtype=np.uint8), size=(1, 65536))
    std = to_dev(st, np.uint8)
    cons = dev.state_consensus(std, [np.array([c], dtype=np.int32) for c in range(65535)])
    assert np.array_equal(to_host(cons)[0], st[0, :65535])                                 # a group of one cell: the cell's state
    with pytest.raises(_lib.IcnvError) as e:
        dev.state_consensus(std, [np.array([c], dtype=np.int32) for c in range(65536)])
    assert e.value.code == _lib.ERR_UNSUPPORTED


# ================================================================== h. proxy values
@pytest.mark.parametrize("K", (3, 6))
def test_states_to_proxy_every_byte_the_tables_name_or_not(dev, K):
    G, C = 37, 29                                                                          # 1073 bytes: four blocks and a part of a fifth
    st = np.resize(np.array([0, 1, 2, 3, 4, 5, 6, 7, 255], dtype=np.uint8), G * C).reshape(G, C)
    st = np.random.default_rng(K).permuted(st, axis=1)
    got = to_host(dev.states_to_proxy(to_dev(st, np.uint8), K))
    want = gh.proxy(st, K)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)])
    assert np.isnan(got[np.isin(st, (0, 7, 255) + ((4, 5, 6) if K == 3 else ()))]).all()
    assert sorted(set(got[~np.isnan(got)].tolist())) == sorted(gh.PROXY[K].values())
