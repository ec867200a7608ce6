"""Steps 18-19 per cell on the GPU (DESIGN K25): the packed sampler of regions with a handful of undecided cells bit-equal to
the restatement of tests/bayes_restate.py and counted by the library's own statistics, the one-launch rectangle rewrite
against a NumPy loop, and the table route of bayes_net / cnv_regions against the dict route -- objects, probabilities,
filtered states and files."""
import numpy as np
import pytest

import bayes_restate as br

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MU6 = np.array([0.1, 0.5, 1.0, 1.5, 2.0, 3.0])
TAU6 = 1.0 / np.array([0.2, 0.25, 0.3, 0.3, 0.35, 0.4]) ** 2
MU3 = np.array([0.5, 1.0, 1.5])
TAU3 = np.full(3, 1.0 / 0.2 ** 2)


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


# ---- the packed sampler -------------------------------------------------------------------------------------------------
# (cells, undecided cells) of every region: packed when it has cells and at most 8 of them are undecided
SHAPES = [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2), (8, 0), (8, 7), (8, 8), (9, 1), (9, 8), (9, 9), (40, 0), (40, 7), (40, 8),
          (40, 9), (40, 40)]
N_PACKED = sum(1 for n, u in SHAPES if n > 0 and u <= 8)


def planted_L(K, shapes, seed):
    """L built directly: a row with ONE non-zero entry is decided, a row with several and an all-zero row are undecided."""
    rng = np.random.default_rng(seed)
    rows, off = [], [0]
    for n, u in shapes:
        block = np.zeros((n, K))
        und = rng.permutation(n)[:u]
        for i in range(n):
            if i in und:
                if rng.random() < 0.2:
                    continue                                            # all zero: undecided too
                nz = rng.choice(K, size=int(rng.integers(2, K + 1)), replace=False)
                block[i, nz] = rng.uniform(0.05, 1.0, size=nz.size)
                block[i, nz[0]] = 1.0
            else:
                block[i, rng.integers(K)] = 1.0
        assert (((block > 0).sum(axis=1) != 1).sum()) == u
        rows.append(block)
        off.append(off[-1] + n)
    return np.concatenate(rows), np.array(off, dtype=np.int64)


def gpu_sample(dev, L, off, tokens, sched, seed, want_samples=True):
    ts, smp, fr = dev.bayes_sample(torch.from_numpy(L).cuda(), off, tokens, *sched, seed=seed, want_samples=want_samples)
    return ts.cpu().numpy(), (smp.cpu().numpy() if smp is not None else None), fr.cpu().numpy()


@pytest.fixture(scope="module")
def packed_case():
    out = {}
    for K in (3, 6):
        L, off = planted_L(K, SHAPES, K)
        tokens = [br.fnv1a64(f"chr{r}-region_{r + 1}") for r in range(len(SHAPES))]
        assert {n for n, _ in SHAPES} == {0, 1, 2, 8, 9, 40} and {u for n, u in SHAPES if n and u <= 8} >= {0, 1, 7, 8}
        assert any(u == 9 for _, u in SHAPES) and (N_PACKED * K) % 8 != 0   # a last wavefront that is not full
        out[K] = (L, off, tokens, br.sample(L, off, tokens, K, 3, 2, 6, seed=K))
    return out


@pytest.mark.parametrize("want_samples", [True, False])
@pytest.mark.parametrize("K", [3, 6])
def test_packed_regions_bit_equal_and_counted(dev, packed_case, K, want_samples):
    L, off, tokens, (rts, rsmp, rfr) = packed_case[K]
    dev.bayes_stats(reset=True)
    ts, smp, fr = gpu_sample(dev, L, off, tokens, (3, 2, 6), K, want_samples)
    st = dev.bayes_stats()
    assert st["regions_packed"] == N_PACKED                              # the class ran: not the old path under another name
    assert st["regions_lds"] == len(SHAPES) and st["regions_streamed"] == 0 and st["undecided_rows"] == sum(u for _, u in SHAPES)
    same(ts, rts)
    assert (smp is None) == (not want_samples)
    if want_samples:
        same(smp, rsmp)
    assert np.array_equal(fr, rfr) and (fr.sum(axis=1) == K * 6).all()
    assert np.isnan(ts[0]).all() and not np.isnan(ts[1:]).any()          # the region without cells keeps its NaN


def test_packed_default_schedule(dev):
    """500 + 200 discarded and 1 000 kept iterations on three one-cell regions."""
    L = np.array([[1.0, 0.5, 0.2], [0.3, 1.0, 0.9], [0.0, 1.0, 0.0]])
    off = np.arange(4, dtype=np.int64)
    tokens = [br.fnv1a64(f"chr7-region_{o}") for o in (3, 10, 999)]
    dev.bayes_stats(reset=True)
    ts, smp, fr = gpu_sample(dev, L, off, tokens, (500, 200, 1000), 1)
    assert dev.bayes_stats()["regions_packed"] == 3
    rts, rsmp, rfr = br.sample(L, off, tokens, 3, 500, 200, 1000, seed=1)
    same(ts, rts)
    same(smp, rsmp)
    assert np.array_equal(fr, rfr)


def test_packed_thousand_regions_against_the_lds_path(dev, monkeypatch):
    """1 030 regions of 0-3 cells: more than one workgroup of the packed kernel, against ICNV_BAYES_PACKED=0 -- the path that
    test_gpu_bayes.test_thousand_regions holds to the restatement."""
    rng = np.random.default_rng(17)
    shapes = [(n, int(rng.integers(0, n + 1))) for n in rng.integers(0, 4, size=1030)]
    with_cells = sum(1 for n, _ in shapes if n)
    assert len({n for n, _ in shapes}) == 4 and with_cells * 3 > 256 // 8
    L, off = planted_L(3, shapes, 18)
    tokens = [br.fnv1a64(f"chr{r % 22 + 1}-region_{r + 1}") for r in range(len(shapes))]
    dev.bayes_stats(reset=True)
    a = gpu_sample(dev, L, off, tokens, (1, 1, 2), 3)
    assert dev.bayes_stats(reset=True)["regions_packed"] == with_cells
    monkeypatch.setenv("ICNV_BAYES_PACKED", "0")
    b = gpu_sample(dev, L, off, tokens, (1, 1, 2), 3)
    st = dev.bayes_stats(reset=True)
    monkeypatch.delenv("ICNV_BAYES_PACKED")
    assert st["regions_packed"] == 0 and st["regions_lds"] == len(shapes)
    same(a[0], b[0])
    same(a[1], b[1])
    assert np.array_equal(a[2], b[2])


def test_packed_with_every_cell_undecided(dev, packed_case, monkeypatch):
    """ICNV_BAYES_DECIDED=0: the same output, and the regions of at most 8 CELLS are the packed ones."""
    L, off, tokens, (rts, rsmp, rfr) = packed_case[6]
    monkeypatch.setenv("ICNV_BAYES_DECIDED", "0")
    dev.bayes_stats(reset=True)
    ts, smp, fr = gpu_sample(dev, L, off, tokens, (3, 2, 6), 6)
    st = dev.bayes_stats(reset=True)
    monkeypatch.delenv("ICNV_BAYES_DECIDED")
    assert st["undecided_rows"] == st["rows"] == L.shape[0]
    assert st["regions_packed"] == sum(1 for n, _ in SHAPES if 0 < n <= 8)
    same(ts, rts)
    same(smp, rsmp)
    assert np.array_equal(fr, rfr)


# ---- fill_regions ---------------------------------------------------------------------------------------------------------
G_FILL, C_FILL = 121, 70
#                genes            cells                                   value
FILL_REGIONS = [((0, 1), [5], 3), ((1, 63), list(range(64, -1, -1)), 4), ((57, 64), [65], 5), ((10, 65), [66], 6),
                ((0, 121), [67], 2), ((3, 6), [], 1), ((0, 121), [69, 68], 0), ((100, 21), [0, 9], 1)]


def fill_arrays(regions):
    off = np.concatenate([[0], np.cumsum([len(c) for _, c, _ in regions])]).astype(np.int64)
    idx = np.array([c for _, cells, _ in regions for c in cells], dtype=np.int32)
    return (np.array([g for (g, _), _, _ in regions], dtype=np.int32), np.array([n for (_, n), _, _ in regions], dtype=np.int32), off, idx,
            np.array([v for _, _, v in regions], dtype=np.uint8))


def fill_by_loop(states, regions):
    want = states.copy()
    for (g0, ng), cells, v in regions:
        for c in cells:
            if v:
                want[c, g0:g0 + ng] = v
    return want


@pytest.mark.parametrize("one_cell", [False, True])
@pytest.mark.parametrize("ld", [128, 121])
def test_fill_regions_against_a_loop(dev, ld, one_cell):
    regions = [r for r in FILL_REGIONS if len(r[1]) == 1] + [((0, 121), [68], 0)] if one_cell else FILL_REGIONS
    assert {len(c) for _, c, _ in FILL_REGIONS} >= {0, 1, 65} and {n for (_, n), _, _ in FILL_REGIONS} >= {1, 63, 64, 65, G_FILL}
    assert any(v == 0 for _, _, v in regions) and (not one_cell or all(len(c) == 1 for _, c, _ in regions))
    touched = np.zeros((C_FILL, G_FILL), dtype=np.int32)
    for (g0, ng), cells, _ in regions:
        touched[cells, g0:g0 + ng] += 1
    assert touched.max() == 1                                            # the rectangles are disjoint
    rng = np.random.default_rng(ld)
    full = torch.full((C_FILL, ld), 77, dtype=torch.uint8, device="cuda")
    start = rng.integers(7, 10, size=(C_FILL, G_FILL)).astype(np.uint8)
    full[:, :G_FILL] = torch.from_numpy(start).cuda()
    states = full[:, :G_FILL]
    arrays = fill_arrays(regions)
    assert dev.fill_regions(states, *arrays) is states
    got = full.cpu().numpy()
    assert np.array_equal(got[:, :G_FILL], fill_by_loop(start, regions)) and (got[:, G_FILL:] == 77).all()
    # the same from arrays that already are on the device
    again = torch.from_numpy(start).cuda()
    on_dev = [torch.from_numpy(a).cuda() for a in arrays]
    dev.fill_regions(again, *on_dev)
    assert np.array_equal(again.cpu().numpy(), got[:, :G_FILL])


@pytest.mark.parametrize("fault", ["gene_end", "gene_negative", "gene_count", "cell_high", "cell_negative", "offsets"])
def test_fill_regions_refuses_before_it_writes(dev, fault):
    g0, ng, off, idx, val = fill_arrays(FILL_REGIONS)
    if fault == "gene_end":
        g0[3] = G_FILL - ng[3] + 1
    elif fault == "gene_negative":
        g0[0] = -1
    elif fault == "gene_count":
        ng[2] = 0
    elif fault == "cell_high":
        idx[-1] = C_FILL
    elif fault == "cell_negative":
        idx[3] = -1
    else:
        off[2] = off[3] + 1
    start = np.random.default_rng(1).integers(7, 10, size=(C_FILL, G_FILL)).astype(np.uint8)
    states = torch.from_numpy(start).cuda()
    with pytest.raises(ValueError):
        dev.fill_regions(states, g0, ng, off, idx, val)
    assert np.array_equal(states.cpu().numpy(), start)


# ---- the two routes -------------------------------------------------------------------------------------------------------
CHR_SIZES = (("chrA", 1), ("chrB", 2), ("chrC", 57), ("chrD", 60))
SCHED = (4, 3, 40)


def routes_object(hmm_type, torn=False, seed=0):
    """40 cells -- 8 reference, 32 observation cells in two groups of two subclusters -- x 120 genes in chromosomes of 1, 2, 57
    and 60 genes.  Planted HMM calls: A (chrC genes 5-24, group g1) a gain whose data sit at the neutral mean; B (chrD genes
    70-99, every observation cell) a call whose data sit at another state's mean; C (chrC genes 40-55, group g2) a loss whose
    data agree with it; short runs of single cells, calls on the two small chromosomes, all-neutral cells and one byte outside
    the states.  torn: chrC comes in two blocks with chrD between them, so the object needs chr_layout()'s gather."""
    from infercnv_amd.infercnv_object import GeneOrder, InfercnvObject
    rng = np.random.default_rng(seed)
    i6 = hmm_type == "i6"
    mu, sd = (MU6, 1.0 / np.sqrt(TAU6)) if i6 else (MU3, 1.0 / np.sqrt(TAU3))
    normal, gain, gain2, loss = (3, 4, 5, 2) if i6 else (2, 3, 3, 1)
    G, C = 120, 40
    g1, g2 = np.arange(8, 24), np.arange(24, 40)
    states = np.full((G, C), normal, dtype=np.int8)
    expr = rng.normal(mu[normal - 1], sd[normal - 1], size=(G, C))
    states[5:25, g1] = gain2                                             # A: the data stay neutral
    b_state, b_data = (gain, gain2) if i6 else (loss, gain)              # B: called one state, the data sit at another
    states[70:100, 8:] = b_state
    expr[70:100, 8:] = rng.normal(mu[b_data - 1], sd[b_data - 1], size=(30, 32))
    states[40:56, g2] = loss                                             # C: call and data agree
    expr[40:56, 24:] = rng.normal(mu[loss - 1], sd[loss - 1], size=(16, 16))
    states[0, 9] = 1
    states[1:3, [10, 30, 31]] = 6 if i6 else 3
    states[30:33, 12] = loss
    states[110:119, 26] = gain
    states[45:47, 35] = normal                                           # splits C for one cell
    states[:, [15, 39]] = normal                                         # all-neutral observation cells
    states[80, 20] = -1                                                  # a byte outside the states
    assert (states[:, :8] == normal).all() and (states == -1).sum() == 1
    chrs = np.concatenate([np.repeat(n, k) for n, k in CHR_SIZES])
    pos = np.concatenate([np.arange(k) * 1000 + 1 for _, k in CHR_SIZES])
    rows = np.arange(G)
    if torn:
        rows = np.concatenate([np.arange(3, 33), np.arange(60, 120), np.arange(33, 60), np.arange(0, 3)])
    obj = InfercnvObject(expr_data=expr[rows], gene_order=GeneOrder(chr=chrs[rows], start=pos[rows], stop=pos[rows] + 500),
                         reference_grouped_cell_indices={"normal": np.arange(8)},
                         observation_grouped_cell_indices={"g1": g1, "g2": g2},
                         tumor_subclusters={"subclusters": {"normal": {"normal.s1": np.arange(8)},
                                                            "g1": {"g1.s1": np.arange(8, 16), "g1.s2": np.arange(23, 15, -1)},
                                                            "g2": {"g2.s1": np.arange(24, 34), "g2.s2": np.arange(34, 40)}}},
                         gene_names=np.array([f"g{i}" for i in range(G)])[rows], cell_names=np.array([f"c{i}" for i in range(C)]))
    assert (obj.chr_layout()[0] is not None) == torn
    return obj, states[rows]


def compare_routes(obj, states, hmm_type, by, tmp_path, thr, device_states=None):
    from infercnv_amd import bayes_net, cnv_regions
    normal = 3 if hmm_type == "i6" else 2
    mu, tau = (MU6, TAU6) if hmm_type == "i6" else (MU3, TAU3)
    st_obj = obj.copy()
    st_obj.expr_data = states.astype(np.float64)
    cnv_regions.generate_cnv_region_reports(st_obj, "17_HMM_pred", str(tmp_path), ignore_neutral_state=normal, by=by)
    res = {}
    for route in ("dict", "table"):
        m = bayes_net.inferCNVBayesNet(obj, states, hmm_type, by=by, seed=4, n_adapt=SCHED[0], n_burn=SCHED[1], n_keep=SCHED[2],
                                       mu=mu, sig=tau, out_dir=str(tmp_path / route), route=route)
        f, new_states = bayes_net.filterHighPNormals(m, states if device_states is None else device_states, thr)
        cnv_regions.adjust_genes_regions_report(f, "17_HMM_pred", "adjusted." + route, str(tmp_path))
        res[route] = (m, f, new_states)
    (md, fd, sd), (mt, ft, stt) = res["dict"], res["table"]
    assert md.table is None and isinstance(mt.table, bayes_net.RegionTable) and ft.table.source is mt.table
    assert not isinstance(mt.cell_gene, list) and len(md.cnv_regions) > 0
    for a, b in ((md, mt), (fd, ft)):
        assert list(b.cnv_regions) == a.cnv_regions and len(b.cell_gene) == len(a.cell_gene) == len(b.cell_probabilities)
        for x, y in zip(a.cell_gene, b.cell_gene):
            assert x["cnv_regions"] == y["cnv_regions"] and x["State"] == y["State"] and type(y["State"]) is int
            assert np.array_equal(x["Genes"], y["Genes"]) and np.array_equal(x["Cells"], y["Cells"])
            assert x["Genes"].dtype == y["Genes"].dtype and x["Cells"].dtype == y["Cells"].dtype
        same(a.cnv_means, b.cnv_means)
        for x, y in zip(a.cell_probabilities, b.cell_probabilities):
            same(x, y)
        assert list(b.cnv_probabilities) == a.cnv_probabilities == [None] * len(a.cell_gene)
    assert np.array_equal(md.group_id, mt.group_id) and md.group_id.dtype == mt.group_id.dtype
    if device_states is None:
        assert stt.dtype == sd.dtype == states.dtype and np.array_equal(sd, stt)
    else:
        assert stt.is_cuda and stt.dtype == device_states.dtype and torch.equal(sd, stt)
    # the fixture has removed, reassigned and kept regions
    old = [cg["State"] for cg, p in zip(md.cell_gene, md.cnv_means[normal - 1]) if not p > thr]
    removed, moved = len(md.cell_gene) - len(old), sum(1 for o, cg in zip(old, fd.cell_gene) if o != cg["State"])
    assert len(old) == len(fd.cell_gene) and removed > 0 and moved > 0 and len(old) - moved > 0, (removed, moved, len(old) - moved)
    name = "CNV_State_Probabilities.dat"
    assert (tmp_path / "dict" / name).read_bytes() == (tmp_path / "table" / name).read_bytes()
    for suffix in (".pred_cnv_genes.dat", ".pred_cnv_regions.dat"):
        want = (tmp_path / ("adjusted.dict" + suffix)).read_bytes()
        assert (tmp_path / ("adjusted.table" + suffix)).read_bytes() == want and want.count(b"\n") > 1
    return res


@pytest.mark.parametrize("by", ["cell", "subcluster", "consensus"])
@pytest.mark.parametrize("hmm_type,thr", [("i6", 0.2), ("i3", 0.35)])
def test_table_route_equals_dict_route(dev, tmp_path, hmm_type, thr, by):
    obj, states = routes_object(hmm_type)
    res = compare_routes(obj, states, hmm_type, by, tmp_path, thr)
    if by == "cell":
        mt = res["table"][0]
        assert (np.diff(mt.table.cell_off) == 1).all() and (mt.table.state == -1).sum() == 1
        assert len(mt.table) > 32 and len(set(mt.cnv_regions)) == len(mt.table)


def test_table_route_states_on_the_device(dev, tmp_path):
    obj, states = routes_object("i6")
    for sub, dtype in (("u8", torch.uint8), ("i32", torch.int32)):
        dev_states = torch.from_numpy(np.ascontiguousarray(np.where(states < 0, 7, states).T)).cuda().to(dtype)
        keep = dev_states.clone()
        (tmp_path / sub).mkdir()
        compare_routes(obj, states, "i6", "cell", tmp_path / sub, 0.2, device_states=dev_states)
        assert torch.equal(dev_states, keep)                             # the input is left alone


def test_table_route_with_a_gene_gather(dev, tmp_path):
    obj, states = routes_object("i6", torn=True)
    res = compare_routes(obj, states, "i6", "cell", tmp_path, 0.2)
    t = res["table"][0].table
    assert t.perm is not None and (t.row_first != t.gene_first).any()


def test_table_route_refuses_remove_cells(dev):
    from infercnv_amd import bayes_net
    obj, states = routes_object("i6")
    with pytest.raises(ValueError, match="removeCells"):
        bayes_net.inferCNVBayesNet(obj, states, "i6", by="cell", postMcmcMethod="removeCells", mu=MU6, sig=TAU6, route="table")


# ---- run() ------------------------------------------------------------------------------------------------------------------
class Hook:
    def __init__(self):
        self.seen = {}

    def __call__(self, step, label, obj):
        self.seen[step] = obj


def counts_object(seed=3):
    """The routes object's shape with counts that carry its planted gains and losses, for run() from step 1."""
    from infercnv_amd.infercnv_object import InfercnvObject
    obj, states = routes_object("i6", seed=seed)
    rng = np.random.default_rng(seed)
    factor = np.array([0.0, 0.05, 0.5, 1.0, 1.5, 2.0, 3.0])[np.where(states < 0, 3, states)]
    base = rng.uniform(20.0, 60.0, size=(states.shape[0], 1))
    counts = rng.poisson(base * factor).astype(np.float64)
    return InfercnvObject(expr_data=counts, count_data=counts.copy(), gene_order=obj.gene_order,
                          reference_grouped_cell_indices=obj.reference_grouped_cell_indices,
                          observation_grouped_cell_indices=obj.observation_grouped_cell_indices,
                          gene_names=obj.gene_names, cell_names=obj.cell_names)


def test_run_cells_mode_takes_the_table_route(dev, tmp_path):
    from infercnv_amd import bayes_net, cnv_regions, run
    hook = Hook()
    out = tmp_path / "run"
    run(counts_object(), cutoff=1, out_dir=str(out), HMM=True, HMM_type="i6", analysis_mode="cells", denoise=True, BayesMaxPNormal=0.2,
        no_plot=True, seed=7, on_step=hook, up_to_step=19)
    assert {17, 18, 19} <= set(hook.seen)
    m = hook.seen[18]
    assert isinstance(m.table, bayes_net.RegionTable) and len(m.table) > 0 and m.args["by"] == "cell"
    token, states = "HMMi6.hmm_mode-cells", hook.seen[17].expr_data
    # the hand composition on the dict route, from the objects run() itself passed on
    hand = tmp_path / "hand"
    cnv_regions.generate_cnv_region_reports(hook.seen[17], f"17_HMM_pred{token}", str(hand), ignore_neutral_state=3, by="cell")
    md = bayes_net.inferCNVBayesNet(m.infercnv_obj, states, HMM_type="i6", by="cell", seed=7, out_dir=str(hand / "bayes"))
    assert md.table is None and md.cnv_regions == list(m.cnv_regions)
    same(md.cnv_means, m.cnv_means)
    fd, kept = bayes_net.filterHighPNormals(md, states, 0.2)
    assert np.array_equal(hook.seen[19].expr_data, kept) and len(md.cell_gene) > 0
    cnv_regions.adjust_genes_regions_report(fd, f"17_HMM_pred{token}", f"HMM_CNV_predictions.{token}.Pnorm_0.2", str(hand))
    for suffix in ("pred_cnv_genes.dat", "pred_cnv_regions.dat"):
        for prefix in (f"17_HMM_pred{token}", f"HMM_CNV_predictions.{token}.Pnorm_0.2"):
            name = f"{prefix}.{suffix}"
            assert (out / name).read_bytes() == (hand / name).read_bytes(), name
    # written when a region was removed, on either route
    got, want = out / f"BayesNetOutput.{token}" / "CNV_State_Probabilities.dat", hand / "bayes" / "CNV_State_Probabilities.dat"
    assert got.exists() == want.exists() == (len(fd.cell_gene) < len(md.cell_gene))
    if want.exists():
        assert got.read_bytes() == want.read_bytes()
