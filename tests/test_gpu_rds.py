"""K27 on the GPU (-m gpu): icnv_xdr_encode_dev / icnv_xdr_decode_dev against NumPy's big-endian column-major bytes at the
shapes where the kernels can go wrong (one element, one row, one column, tiles cut in both directions, several tiles), in
both layouts, with and without padded rows, whole and in segments that cut tiles and columns; the refusals; the device route
of save_infercnv_obj against the host route byte for byte; the device load; run() with rds_checkpoints."""
import ctypes as ct
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_rds_host import NA_REAL, OTHER_NAN, assert_same_object, bits, example_object, tree  # noqa: E402

SHAPES = [(1, 1), (1, 70), (70, 1), (33, 65), (64, 64), (257, 129)]
SEGMENTS = (1, 7, 1000)
SPECIALS = np.array([NA_REAL, OTHER_NAN, 0.0, -0.0, np.inf, -np.inf, 5e-324, -2.2250738585072009e-308])


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infercnv_amd import device
    torch.cuda.set_device(0)
    device.init(0)
    return device


def matrix(rows, cols):
    """R's rows x cols matrix with the special values spread over it, and its stream: big-endian, column after column."""
    rng = np.random.default_rng(rows * 1000 + cols)
    x = rng.normal(size=(rows, cols))
    flat = x.reshape(-1)
    at = rng.permutation(flat.size)[:SPECIALS.size]
    flat[at] = SPECIALS[:at.size]
    return x, np.asfortranarray(x).astype(">f8").tobytes(order="F")


def on_device(x, layout, pad, fill=None):
    """x as the device matrix of the layout, its rows pad elements longer than they need to be; (view, base)."""
    src = np.ascontiguousarray(x.T) if layout == "cols" else x
    base = torch.full((src.shape[0], src.shape[1] + pad), -7.0 if fill is None else fill, dtype=torch.float64, device="cuda")
    view = base[:, :src.shape[1]]
    if fill is None:
        view.copy_(torch.from_numpy(src))
    return view, base


def raw_call(fn, mat, es, rows, cols, ld, layout, e0, e1, stream_ptr):
    """One call of the C entry point (the segment loops make hundreds of thousands of them)."""
    return fn(ct.c_void_p(mat), es, rows, cols, ld, layout, e0, e1, ct.c_void_p(stream_ptr), None)


def encode_segments(L, t, layout, rows, cols, seg, es=8):
    n = rows * cols
    out = torch.zeros(n * es, dtype=torch.uint8, device="cuda")
    ld = t.stride(0) if t.dim() == 2 and t.shape[0] > 1 else (rows if layout == 0 else cols)
    for e0 in range(0, n, seg):
        assert raw_call(L.icnv_xdr_encode_dev, t.data_ptr(), es, rows, cols, ld, layout, e0, min(n, e0 + seg), out.data_ptr() + e0 * es) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy().tobytes()


def decode_segments(L, stream, t, layout, rows, cols, seg, es=8):
    n = rows * cols
    ld = t.stride(0) if t.dim() == 2 and t.shape[0] > 1 else (rows if layout == 0 else cols)
    for e0 in range(0, n, seg):
        assert raw_call(L.icnv_xdr_decode_dev, stream.data_ptr() + e0 * es, es, rows, cols, ld, layout, e0, min(n, e0 + seg), t.data_ptr()) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("layout", ["cols", "rows"])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_encode_and_decode(dev, rows, cols, layout, pad):
    from infercnv_amd import _lib
    L = _lib.load()
    x, want = matrix(rows, cols)
    code = dev.XDR_LAYOUTS[layout]
    t, base = on_device(x, layout, pad)
    before = base.clone()
    got = dev.xdr_encode(t, layout=layout)
    assert got.dtype == torch.uint8 and got.cpu().numpy().tobytes() == want
    for seg in SEGMENTS:                                   # the concatenation of the segments is the whole
        assert encode_segments(L, t, code, rows, cols, seg) == want, f"segments of {seg}"
    assert torch.equal(base.view(torch.int64), before.view(torch.int64))          # encode reads only

    stream = torch.from_numpy(np.frombuffer(want, dtype=np.uint8).copy()).cuda()
    src_bits = np.ascontiguousarray(x.T if layout == "cols" else x).view(np.uint64)
    for seg in (rows * cols,) + SEGMENTS:
        out, out_base = on_device(x, layout, pad, fill=-3.0)
        if seg == rows * cols:
            dev.xdr_decode(stream, out, layout=layout)
            torch.cuda.synchronize()
        else:
            decode_segments(L, stream, out, code, rows, cols, seg)
        assert np.array_equal(out.cpu().numpy().view(np.uint64), src_bits), f"decode in segments of {seg}"
        if pad:
            assert bool((out_base[:, out.shape[1]:] == -3.0).all())                # the padding is never written
    # decode of encode is the identity
    back, _ = on_device(x, layout, pad, fill=0.0)
    dev.xdr_decode(dev.xdr_encode(t, layout=layout), back, layout=layout)
    assert torch.equal(back.contiguous().view(torch.int64), t.contiguous().view(torch.int64))


def test_partial_segment_leaves_the_rest(dev):
    """A decode writes the elements of its segment and nothing else, in both layouts."""
    rows, cols = 33, 65
    x, want = matrix(rows, cols)
    e0, e1 = 40, 1900
    stream = torch.from_numpy(np.frombuffer(want[e0 * 8:e1 * 8], dtype=np.uint8).copy()).cuda()
    inside = np.zeros(rows * cols, dtype=bool)
    inside[e0:e1] = True
    inside = inside.reshape(cols, rows)                    # the stream's own order
    for layout in ("cols", "rows"):
        out, _ = on_device(x, layout, 3, fill=-3.0)
        dev.xdr_decode(stream, out, layout=layout, e0=e0, e1=e1)
        got = out.cpu().numpy()
        got = got if layout == "cols" else got.T
        assert np.array_equal(got[inside].view(np.uint64), x.T[inside].view(np.uint64)) and bool((got[~inside] == -3.0).all())


@pytest.mark.parametrize("n", [1, 63, 65, 1000])
def test_int32_vectors(dev, n):
    from infercnv_amd import _lib
    L = _lib.load()
    rng = np.random.default_rng(n)
    v = rng.integers(-2 ** 31, 2 ** 31, size=n, dtype=np.int64).astype(np.int32)
    v[rng.integers(0, n)] = -2 ** 31                       # NA_integer_
    want = v.astype(">i4").tobytes()
    t = torch.from_numpy(v).cuda()
    assert dev.xdr_encode(t).cpu().numpy().tobytes() == want
    stream = torch.from_numpy(np.frombuffer(want, dtype=np.uint8).copy()).cuda()
    for seg in SEGMENTS:
        assert encode_segments(L, t, 0, n, 1, seg, es=4) == want
        out = torch.zeros(n, dtype=torch.int32, device="cuda")
        decode_segments(L, stream, out, 0, n, 1, seg, es=4)
        assert np.array_equal(out.cpu().numpy(), v)
    assert np.array_equal(dev.xdr_decode(stream, torch.zeros(n, dtype=torch.int32, device="cuda")).cpu().numpy(), v)
    # an int32 matrix through the transposing kernel
    if n == 1000:
        m = v.reshape(40, 25)
        got = dev.xdr_encode(torch.from_numpy(m).cuda(), layout="rows").cpu().numpy().tobytes()
        assert got == np.asfortranarray(m).astype(">i4").tobytes(order="F")


def test_argument_refusals(dev):
    from infercnv_amd import _lib
    L = _lib.load()
    src = torch.zeros(64, dtype=torch.float64, device="cuda")
    dst = torch.zeros(64 * 8, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    dev.timing_enable(True)
    dev.timing_reset()
    good = dict(es=8, rows=8, cols=8, ld=8, layout=0, e0=0, e1=64)
    bad = [dict(es=2), dict(es=16), dict(layout=2), dict(rows=0), dict(cols=-1), dict(ld=7), dict(layout=1, ld=7), dict(e0=-1),
           dict(e0=5, e1=4), dict(e1=65), dict(rows=2 ** 40, cols=2 ** 40, ld=2 ** 40)]
    try:
        for fn in (L.icnv_xdr_encode_dev, L.icnv_xdr_decode_dev):
            mat, stream = (src, dst) if fn is L.icnv_xdr_encode_dev else (dst, src)
            for change in bad:
                a = {**good, **change}
                rc = fn(ct.c_void_p(mat.data_ptr()), a["es"], a["rows"], a["cols"], a["ld"], a["layout"], a["e0"], a["e1"],
                        ct.c_void_p(stream.data_ptr()), None)
                assert rc == _lib.ERR_ARG, change
                assert L.icnv_last_error()
            a = good
            assert fn(None, 8, 8, 8, 8, 0, 0, 64, ct.c_void_p(stream.data_ptr()), None) == _lib.ERR_ARG
            assert fn(ct.c_void_p(mat.data_ptr()), 8, 8, 8, 8, 0, 0, 64, None, None) == _lib.ERR_ARG
            assert fn(ct.c_void_p(mat.data_ptr() + 4), 8, 8, 8, 8, 0, 0, 60, ct.c_void_p(stream.data_ptr()), None) == _lib.ERR_ARG
        assert dev.timing_get("xdr_encode")[1] == 0 and dev.timing_get("xdr_decode")[1] == 0      # nothing was launched
        with pytest.raises(_lib.IcnvError) as err:
            dev.xdr_encode(src.view(8, 8), e0=3, e1=65)
        assert err.value.code == _lib.ERR_ARG
        with pytest.raises(ValueError):
            dev.xdr_encode(src.view(8, 8), out=dst[:100])
        assert dev.timing_get("xdr_encode")[1] == 0
        dev.xdr_encode(src.view(8, 8))
        torch.cuda.synchronize()
        assert dev.timing_get("xdr_encode")[1] == 1                                                 # the hook does count launches
    finally:
        dev.timing_enable(False)
    assert bool((dst == 0).all())


# ---- the routes of save_infercnv_obj / load_infercnv_obj -------------------------------------------------------------------
def object_257x129():
    from infercnv_amd import GeneOrder, InfercnvObject
    G, C = 257, 129
    x, _ = matrix(G, C)
    rng = np.random.default_rng(5)
    cells = np.array([f"cell_{i}" for i in range(C)])
    obs, ref = np.arange(40, C), np.arange(0, 40)
    return InfercnvObject(
        expr_data=x, count_data=rng.poisson(1.0, size=(G, C)).astype(np.int32),
        gene_order=GeneOrder(np.repeat(["chr1", "chr2", "chr3"], [100, 100, 57]), np.arange(G) * 10 + 1, np.arange(G) * 10 + 9),
        reference_grouped_cell_indices={"ref": ref}, observation_grouped_cell_indices={"obs": obs},
        tumor_subclusters={"hc": {"obs": [tree(50, cells[40:90]), None], "ref": tree(40, cells[ref])},
                           "subclusters": {"obs": {"obs_s1": obs[:50], "obs_s2": obs[50:]}, "ref": {"ref_s1": ref}}},
        options={"cutoff": 0.1, "HMM": False, "out_dir": "o", "noise_filter": None, "k_nn": 20},
        gene_names=np.array([f"g{i}" for i in range(G)]), cell_names=cells)


def test_route_equality_and_device_load(dev, tmp_path, monkeypatch):
    from infercnv_amd import load_infercnv_obj, rds, save_infercnv_obj
    obj = object_257x129()
    save_infercnv_obj(obj, tmp_path / "host.rds", device=False)
    want = (tmp_path / "host.rds").read_bytes()
    assert save_infercnv_obj(obj, tmp_path / "default.rds") == [] and (tmp_path / "default.rds").read_bytes() == want   # below the threshold
    monkeypatch.setattr(rds, "DEVICE_THRESHOLD", 0)
    stats = save_infercnv_obj(obj, tmp_path / "device.rds")
    assert len(stats) > 10 and (tmp_path / "device.rds").read_bytes() == want
    x_dev = torch.from_numpy(np.ascontiguousarray(obj.expr_data.T)).cuda()
    blind = obj.copy()
    blind.expr_data = None                                  # with x_dev the host matrix is not looked at
    save_infercnv_obj(blind, tmp_path / "x_dev.rds", x_dev=x_dev)
    assert (tmp_path / "x_dev.rds").read_bytes() == want
    padded = dev.padded_matrix(129, 257)
    padded.copy_(x_dev)
    save_infercnv_obj(blind, tmp_path / "x_dev_ld.rds", x_dev=padded)
    assert (tmp_path / "x_dev_ld.rds").read_bytes() == want
    monkeypatch.setattr(rds, "CHUNK_BYTES", 40_000)         # 265 KB of expr.data: seven chunks, cut inside columns
    stats = save_infercnv_obj(obj, tmp_path / "chunks.rds")
    assert max(s["chunks"] for s in stats) >= 7 and (tmp_path / "chunks.rds").read_bytes() == want
    stats = save_infercnv_obj(blind, tmp_path / "chunks_x_dev.rds", x_dev=x_dev)
    assert max(s["chunks"] for s in stats) >= 7 and (tmp_path / "chunks_x_dev.rds").read_bytes() == want

    # load: the device route returns the host route's bits (several chunks, then one)
    host = load_infercnv_obj(tmp_path / "host.rds")
    assert_same_object(obj, host)
    for chunk in (40_000, 64 << 20):
        monkeypatch.setattr(rds, "CHUNK_BYTES", chunk)
        got, got_dev = load_infercnv_obj(tmp_path / "host.rds", return_device=True)
        assert got.expr_data is None and got_dev.is_cuda and tuple(got_dev.shape) == (129, 257) and got_dev.dtype == torch.float64
        assert np.array_equal(got_dev.cpu().numpy().T.copy().view(np.uint64), bits(host.expr_data))
        got.expr_data = host.expr_data
        assert_same_object(host, got)
    monkeypatch.setattr(rds, "DEVICE_THRESHOLD", 1 << 30)   # below the threshold: decoded on the host, uploaded
    got, got_dev = load_infercnv_obj(tmp_path / "host.rds", return_device=True)
    assert np.array_equal(got_dev.cpu().numpy().T.copy().view(np.uint64), bits(host.expr_data))


def test_run_with_rds_checkpoints(dev, tmp_path, golden_dir):
    """A tiny run(): R's file names are left behind, and every file loads back equal to the object on_step received."""
    from infercnv_amd import load_infercnv_obj, run
    from infercnv_amd.pipeline import checkpoint_file_names, rds_checkpoints
    _, obj = example_object(golden_dir)
    obj.tumor_subclusters, obj.options = None, {}
    obj.expr_data = obj.count_data.copy()
    call = dict(cutoff=1, cluster_by_groups=True, denoise=True, HMM=False, no_plot=True)
    save = rds_checkpoints(str(tmp_path), **call)
    seen = {}

    def hook(step, label, o):
        seen[step] = o
        save(step, label, o)

    final = run(obj, out_dir=str(tmp_path), on_step=hook, **call)
    names = checkpoint_file_names(**call)
    assert sorted(seen) == [1, 2, 3, 4, 8, 9, 10, 11, 12, 14, 15, 22]
    files = {f for f in os.listdir(tmp_path) if f.endswith("_obj")}
    assert files == {names[s] for s in seen} | {"preliminary.infercnv_obj", "run.final.infercnv_obj"}
    assert names[15] == "15_tumor_subclusters.leiden.infercnv_obj" and names[22] == "22_denoise.leiden.NF_NA.SD_1.5.NL_FALSE.infercnv_obj"
    for s, o in seen.items():
        assert_same_object(o, load_infercnv_obj(tmp_path / names[s]))
    assert_same_object(seen[15], load_infercnv_obj(tmp_path / "preliminary.infercnv_obj"))
    assert_same_object(final, load_infercnv_obj(tmp_path / "run.final.infercnv_obj"))
