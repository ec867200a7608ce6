"""The CNV region reports written on the GPU (icnv_cnv_report_*, cnv_regions.generate_cnv_region_reports, DESIGN K24) against
the sequential restatement (tests/cnv_reports_restate.py) and the kept host writer, byte for byte in all four files."""
import ctypes as ct
import glob
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cnv_reports_restate as rr  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infercnv_amd import device
    torch.cuda.set_device(0)
    device.init(0)
    return device


def check_files(obj, by, ignore, tmp_path):
    """All four files of the device writer against the restatement and against the host writer; returns the device's."""
    from infercnv_amd import cnv_regions
    res = cnv_regions.generate_cnv_region_reports(obj, "dev", str(tmp_path), ignore_neutral_state=ignore, by=by)
    assert cnv_regions.LAST_REPORT_STATS.get("device_writer") is True and cnv_regions.LAST_REPORT_STATS["by"] == by
    cnv_regions._generate_cnv_region_reports_host(obj, "host", str(tmp_path), ignore_neutral_state=ignore, by=by)
    got, host, want = rr.read_files(tmp_path, "dev"), rr.read_files(tmp_path, "host"), rr.report_files(obj, by, ignore)
    for s in rr.SUFFIXES:
        assert got[s] == want[s], (by, ignore, s, "restatement")
        assert got[s] == host[s], (by, ignore, s, "host writer")
    return res, got


# ---- the edge object ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("by", ["consensus", "subcluster", "cell"])
@pytest.mark.parametrize("ignore", [None, 3, 2])
def test_edge_object(dev, tmp_path, by, ignore):
    _, got = check_files(rr.edge_object(), by, ignore, tmp_path)
    body = got[".pred_cnv_regions.dat"].split(b"\n")[1:-1]
    assert body and not any(l.split(b"\t")[3] == b"chr1" for l in body)          # the one-gene chromosome yields nothing
    if by == "cell" and ignore is None:
        first = [l.split(b"\t") for l in body][:3]
        assert [f[1] for f in first[:2]] == [b"chr2-region_1", b"chr3-region_2"]     # ... and does not advance the counter
        genes = got[".pred_cnv_genes.dat"].split(b"\n")[1:-1]
        assert sum(1 for l in genes if l.split(b"\t")[0] == b"c2" and l.split(b"\t")[2] == b"6") == 1   # a run of one gene


@pytest.mark.parametrize("by", ["consensus", "subcluster", "cell"])
def test_all_neutral_gives_header_only(dev, tmp_path, by):
    _, got = check_files(rr.edge_object(all_neutral=True), by, 3, tmp_path)
    assert got[".pred_cnv_regions.dat"] == b"cell_group_name\tcnv_name\tstate\tchr\tstart\tend\n"
    assert got[".pred_cnv_genes.dat"] == b"cell_group_name\tgene_region_name\tstate\tgene\tchr\tstart\tend\n"


@pytest.mark.parametrize("ignore", [None, 3])
def test_bytes_outside_the_states_print_as_minus_one(dev, tmp_path, ignore):
    _, got = check_files(rr.edge_object(odd_bytes=True), "cell", ignore, tmp_path)
    lines = [l.split(b"\t") for l in got[".pred_cnv_genes.dat"].split(b"\n")[1:-1]]
    minus = {(l[0], l[3]) for l in lines if l[2] == b"-1"}
    assert minus == {(b"c1", b"g12"), (b"c1", b"g13"), (b"c5", b"g14"), (b"c9", b"g30")}   # bytes 0, 7, 255 (-1) and 7


def test_no_subclusters_falls_to_the_groups(dev, tmp_path):
    obj = rr.edge_object()
    obj.tumor_subclusters = None
    check_files(obj, "cell", 3, tmp_path)


# ---- widths ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide():
    return rr.width_object()


@pytest.mark.parametrize("by,ignore", [("cell", 3), ("cell", None), ("subcluster", 3)])
def test_widths(dev, wide, tmp_path, by, ignore):
    _, got = check_files(wide, by, ignore, tmp_path)
    if by == "cell":
        ordinals = {int(l.split(b"\t")[1].rsplit(b"_", 1)[1]) for l in got[".pred_cnv_regions.dat"].split(b"\n")[1:-1]}
        assert min(ordinals) < 10 and max(ordinals) > 1000                               # crossing 9/10, 99/100, 999/1000
        assert any(l.startswith("zelle_äö€_50\t".encode()) for l in got[".pred_cnv_genes.dat"].split(b"\n"))
    if ignore is None:
        body = got[".pred_cnv_genes.dat"]
        for p in rr.WIDTH_POSITIONS:
            assert (b"\t%d\t" % p) in body and (b"\t%d\n" % p) in body
        assert (b"\t" + b"G" * 3000 + b"\t") in body


def test_gene_order_not_contiguous_by_chromosome(dev, tmp_path):
    obj = rr.width_object(seed=5, C=16, G=600, scramble=True)
    assert obj.chr_layout()[0] is not None                                               # the perm route
    check_files(obj, "cell", 3, tmp_path)
    check_files(obj, "consensus", None, tmp_path)


# ---- the device entry, driven directly ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def direct(dev, wide):
    """The by-cell records of the 64 x 3 000 object without the neutral state, the tables, and the restatement's lines."""
    from infercnv_amd import cnv_regions
    obj = wide
    st = cnv_regions._states_u8(obj)
    groups = cnv_regions._cell_groups(obj, "cell")
    _, chr_start = obj.chr_layout()
    rec, _ = dev.cnv_runs(torch.from_numpy(st.T).cuda(), chr_start, neutral=3, col_idx=np.concatenate([g for _, g in groups]))
    chrs = np.asarray(obj.gene_order.chr)
    tables = cnv_regions._report_tables([n for n, _ in groups], chrs[chr_start[:-1]], obj.genes(), "utf-8")
    pos = (np.asarray(obj.gene_order.start, dtype=np.int64), np.asarray(obj.gene_order.stop, dtype=np.int64))
    region_lines, gene_lines = rr.report_lines(obj, "cell", 3)
    want = {"regions": [l.encode() for l in region_lines], "genes": [("".join(ls)).encode() for ls in gene_lines]}
    return rec, tables, pos, want


def chunks(plan, cap, pad=1):
    """Every chunk of `cap` bytes, each into a fresh poisoned buffer with `pad` sentinel bytes on either side."""
    parts, offsets, rec = [], [0], 0
    while rec < plan.n_records:
        buf = torch.full((cap + 2 * pad,), 0xA5, dtype=torch.uint8, device="cuda")
        done, nbytes, off = plan.format_into(buf[pad:pad + cap], rec)
        host = buf.cpu().numpy()
        assert done >= 1 and off[0] == 0 and off[-1] == nbytes <= cap
        assert (host[:pad] == 0xA5).all() and (host[pad + nbytes:] == 0xA5).all()       # nothing outside out[0 .. n_bytes)
        parts.append(host[pad:pad + nbytes].tobytes())
        offsets += [offsets[-1] + int(o) for o in off[1:]]
        rec += done
    return b"".join(parts), offsets, len(parts)


@pytest.mark.parametrize("kind", ["genes", "regions"])
def test_chunks_concatenate_to_the_one_chunk_text(dev, direct, kind):
    rec, tables, pos, want = direct
    text = b"".join(want[kind])
    sums = np.concatenate([[0], np.cumsum([len(l) for l in want[kind]])]).tolist()
    with dev.CnvReportPlan(kind, rec, *tables, *pos) as plan:
        assert plan.n_records == len(want[kind]) and plan.total_bytes == len(text)
        largest = max(len(l) for l in want[kind])
        assert plan.max_record_bytes == largest and largest <= 64 << 10
        one, off, n = chunks(plan, plan.total_bytes, pad=16)                              # an aligned `out`
        assert n == 1 and one == text and off == sums
        for cap in (64 << 10, largest, largest + 1):
            got, off, n = chunks(plan, cap)                                               # `out` one byte off a 16-byte word
            assert got == text and off == sums, (kind, cap)
            assert n > 1 or plan.total_bytes <= cap
    assert dev.cnv_report(kind, rec, *tables, *pos, capacity=100_000) == text


def test_a_capacity_below_the_first_record_is_refused(dev, direct):
    from infercnv_amd import _lib
    rec, tables, pos, want = direct
    L = _lib.load()
    with dev.CnvReportPlan("genes", rec, *tables, *pos) as plan:
        buf = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda")
        done, nbytes = ct.c_int64(-7), ct.c_int64(-7)
        for rec0, cap in ((0, len(want["genes"][0]) - 1), (5, len(want["genes"][5]) - 1), (0, 0)):
            rc = L.icnv_cnv_report_format_dev(plan._h, rec0, ct.c_void_p(buf.data_ptr()), cap, None, ct.byref(done), ct.byref(nbytes), None)
            assert rc == _lib.ERR_ARG and (done.value, nbytes.value) == (-7, -7)
        torch.cuda.synchronize()
        assert bool((buf == 0xA5).all())
        # the first record exactly: one record
        cap = len(want["genes"][0])
        d, n, off = plan.format_into(buf[:cap], 0)
        assert (d, n) == (1, cap) and buf[:cap].cpu().numpy().tobytes() == want["genes"][0] and bool((buf[cap:] == 0xA5).all())


# ---- refusals before any launch ----------------------------------------------------------------------------------------
def begin(L, kind, rec, n, stride, tables, pos, G=None, null=()):
    i64p = ct.POINTER(ct.c_int64)
    h = ct.c_void_p()
    (gb, go), (cb, co), (nb, no) = tables
    args = {"plan": ct.byref(h), "records": ct.c_void_p(rec.data_ptr()), "gb": ct.c_void_p(gb.ctypes.data), "go": go.ctypes.data_as(i64p),
            "cb": ct.c_void_p(cb.ctypes.data), "co": co.ctypes.data_as(i64p), "nb": ct.c_void_p(nb.ctypes.data), "no": no.ctypes.data_as(i64p),
            "start": pos[0].ctypes.data_as(i64p), "end": pos[1].ctypes.data_as(i64p)}
    for k in null:
        args[k] = None
    rc = L.icnv_cnv_report_begin_dev(args["plan"], kind, args["records"], stride, n, args["gb"], args["go"], go.size - 1, args["cb"], args["co"],
                                     co.size - 1, args["nb"], args["no"], args["start"], args["end"], no.size - 1 if G is None else G, None, None)
    if rc == 0:
        L.icnv_cnv_report_end(h)
    return rc


def test_refusals(dev, direct):
    from infercnv_amd import _lib
    L = _lib.load()
    rec, tables, pos, _ = direct
    rec = rec.contiguous()
    n = rec.shape[1]
    before = dev.cnv_report_stats()
    assert begin(L, 0, rec, n, n, tables, pos) == _lib.OK
    for null in ("plan", "records", "go", "co", "no", "gb", "cb", "nb", "start", "end"):
        assert begin(L, 0, rec, n, n, tables, pos, null=(null,)) == _lib.ERR_ARG, null
    assert begin(L, 2, rec, n, n, tables, pos) == _lib.ERR_ARG                          # unknown kind
    assert begin(L, 0, rec, n, n - 1, tables, pos) == _lib.ERR_ARG                      # capacity below the count

    def with_record(field, value, r=7):
        bad = rec.clone()
        bad[field, r] = value
        return begin(L, 0, bad, n, n, tables, pos)

    n_groups, n_chr, G = (t[1].size - 1 for t in tables)
    first, last = int(rec[2, 7]), int(rec[3, 7])
    assert with_record(2, last + 1) == _lib.ERR_ARG and b"gene_first > gene_last" in L.icnv_last_error()
    for field, value in ((0, -1), (0, n_groups), (1, -1), (1, n_chr), (2, -1), (3, G), (4, 256), (4, -1)):
        assert with_record(field, value) == _lib.ERR_ARG, (field, value)
    assert with_record(3, first) == _lib.OK                                             # a run of one gene is fine

    def with_offsets(which, edit):
        t = [list(x) for x in tables]
        off = t[which][1].copy()
        edit(off)
        t[which][1] = off
        return begin(L, 1, rec, n, n, [tuple(x) for x in t], pos)

    for which in range(3):
        assert with_offsets(which, lambda off: off.__setitem__(0, 1)) == _lib.ERR_ARG                 # do not start at 0
        assert with_offsets(which, lambda off: off.__setitem__(1, off[2] + 1)) == _lib.ERR_ARG        # descend
    with dev.CnvReportPlan("genes", rec, *tables, *pos) as plan:
        done, nbytes = ct.c_int64(), ct.c_int64()
        out = torch.full((1 << 16,), 0xA5, dtype=torch.uint8, device="cuda")
        p = ct.c_void_p(out.data_ptr())
        assert L.icnv_cnv_report_format_dev(plan._h, 0, p, 2 ** 31, None, ct.byref(done), ct.byref(nbytes), None) == _lib.ERR_UNSUPPORTED
        assert L.icnv_cnv_report_format_dev(plan._h, 0, None, 1 << 16, None, ct.byref(done), ct.byref(nbytes), None) == _lib.ERR_ARG
        assert L.icnv_cnv_report_format_dev(plan._h, 0, p, 1 << 16, None, None, ct.byref(nbytes), None) == _lib.ERR_ARG
        assert L.icnv_cnv_report_format_dev(plan._h, 0, p, 1 << 16, None, ct.byref(done), None, None) == _lib.ERR_ARG
        assert L.icnv_cnv_report_format_dev(None, 0, p, 1 << 16, None, ct.byref(done), ct.byref(nbytes), None) == _lib.ERR_ARG
        for rec0 in (-1, n):
            assert L.icnv_cnv_report_format_dev(plan._h, rec0, p, 1 << 16, None, ct.byref(done), ct.byref(nbytes), None) == _lib.ERR_ARG
        torch.cuda.synchronize()
        assert bool((out == 0xA5).all())
    assert dev.cnv_report_stats() == before                                             # a refused call counts nowhere


def test_host_buffer_flavour(dev, direct):
    from infercnv_amd import _lib
    L = _lib.load()
    rec, tables, pos, want = direct
    host = np.ascontiguousarray(rec.cpu().numpy())
    n = host.shape[1]
    i64p = ct.POINTER(ct.c_int64)
    (gb, go), (cb, co), (nb, no) = tables
    h, totals = ct.c_void_p(), (ct.c_int64 * 3)()
    assert L.icnv_cnv_report_begin(ct.byref(h), 1, host.ctypes.data_as(ct.c_void_p), n, n, ct.c_void_p(gb.ctypes.data), go.ctypes.data_as(i64p),
                                   go.size - 1, ct.c_void_p(cb.ctypes.data), co.ctypes.data_as(i64p), co.size - 1, ct.c_void_p(nb.ctypes.data),
                                   no.ctypes.data_as(i64p), pos[0].ctypes.data_as(i64p), pos[1].ctypes.data_as(i64p), no.size - 1, totals) == _lib.OK
    text = b"".join(want["regions"])
    assert tuple(totals) == (len(text), n, max(len(l) for l in want["regions"]))
    out = np.full(len(text) + 8, 0xA5, dtype=np.uint8)
    done, nbytes = ct.c_int64(), ct.c_int64()
    assert L.icnv_cnv_report_format(h, 0, out.ctypes.data_as(ct.c_void_p), len(text) + 8, None, ct.byref(done), ct.byref(nbytes)) == _lib.OK
    L.icnv_cnv_report_end(h)
    assert (done.value, nbytes.value) == (n, len(text)) and out[:len(text)].tobytes() == text and (out[len(text):] == 0xA5).all()


# ---- the return value --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("by", ["consensus", "subcluster", "cell"])
def test_return_value_equals_get_predicted_cnv_regions(dev, tmp_path, by):
    from collections.abc import Sequence
    from infercnv_amd import cnv_regions
    obj = rr.edge_object(odd_bytes=(by == "cell"))
    got = cnv_regions.generate_cnv_region_reports(obj, "r", str(tmp_path), ignore_neutral_state=3, by=by)
    want = cnv_regions.get_predicted_CNV_regions(obj, by)
    assert isinstance(got, Sequence) and not isinstance(got, list) and len(got) == len(want) == {"consensus": 3, "subcluster": 3, "cell": 12}[by]
    n = 0
    for g, w in zip(got, want):                                                          # iteration
        n += 1
        assert g["cell_group_name"] == w["cell_group_name"] and list(g["cells"]) == list(w["cells"])
        assert [rn for rn, _ in g["gene_regions"]] == [rn for rn, _ in w["gene_regions"]]
        for (_, a), (_, b) in zip(g["gene_regions"], w["gene_regions"]):
            assert a["state"] == b["state"] and type(a["state"]) is type(b["state"]) and a["chr"] == b["chr"]
            for k in ("gene", "start", "end"):
                assert np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype
        assert g["cnv_ranges"] == w["cnv_ranges"]
    assert n == len(want)
    assert got[-1]["cell_group_name"] == want[-1]["cell_group_name"] and [x["cell_group_name"] for x in got[1:3]] == [x["cell_group_name"] for x in want[1:3]]
    with pytest.raises(IndexError):
        got[len(want)]
    with pytest.raises(TypeError):
        got[0] = {}


# ---- end to end --------------------------------------------------------------------------------------------------------
def test_run_writes_its_reports_on_the_device(dev, golden_dir, tmp_path):
    """run() on the reference's 20-cell example object, by cell: the report files equal the restatement's on the HMM states
    of step 17, and the library's counters show that the device writer wrote them."""
    from infercnv_amd import GeneOrder, InfercnvObject, run
    d = np.load(os.path.join(golden_dir, "infercnv_object_example.npz"))
    chr_names = d["chr_levels"][d["chr_codes"] - d["chr_codes"].min()]
    obj = InfercnvObject(expr_data=d["count_data"].copy(), count_data=d["count_data"].copy(), gene_order=GeneOrder(chr_names, d["gene_start"], d["gene_stop"]),
                         reference_grouped_cell_indices={"normal": d["ref_normal"]}, observation_grouped_cell_indices={"tumor": d["obs_tumor"]})
    seen = {}
    dev.cnv_report_stats(reset=True)
    run(obj, out_dir=str(tmp_path), cutoff=1, cluster_by_groups=True, denoise=True, analysis_mode="cells", HMM=True, BayesMaxPNormal=0,
        no_plot=True, on_step=lambda step, label, o: seen.__setitem__(step, o))
    stats = dev.cnv_report_stats()
    hmm_obj = seen[17]
    paths = glob.glob(os.path.join(str(tmp_path), "17_HMM_pred*.pred_cnv_genes.dat"))
    assert len(paths) == 1
    prefix = os.path.basename(paths[0])[:-len(".pred_cnv_genes.dat")]
    got, want = rr.read_files(tmp_path, prefix), rr.report_files(hmm_obj, "cell", 3)
    for s in rr.SUFFIXES:
        assert got[s] == want[s], s
    n_lines = sum(got[s].count(b"\n") - 1 for s in (".pred_cnv_regions.dat", ".pred_cnv_genes.dat"))
    n_bytes = sum(len(got[s]) - got[s].index(b"\n") - 1 for s in (".pred_cnv_regions.dat", ".pred_cnv_genes.dat"))
    print(f"[run] device writer: {stats}")
    assert got[".cell_groupings"].count(b"\n") == 21
    assert stats["lines"] == n_lines and stats["bytes"] == n_bytes and (stats["calls"] >= 2 if n_lines else stats["calls"] == 0)
    assert n_lines > 0
