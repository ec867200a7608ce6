"""The host drivers the plain and the column-selected text readers share (DESIGN K21, K22, K26): device.parse_table_into and
device.parse_triplets_into, with and without a column map, on in-memory chunks.  Under the identity map the selected entry must
give what the plain entry gives over the same bytes: the output bits, the label ranges, the row or entry counts and the deltas
of table_parse_stats.  The shapes are the smallest at which the shared driver takes another path."""
import numpy as np
import pytest

from table_parse_cases import TIES

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from infercnv_amd import _lib                           # noqa: E402

COUNTERS = ("rows", "fields", "host_parsed", "bytes", "collect_rounds", "calls")
SENTINEL = -7.25
FIELDS = ("0", "7", "13", "2.5", "1e3", "-4", "0.125", "12345.678", "+6", "3.", ".5", "1e-3")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infercnv_amd import device
    torch.cuda.set_device(0)
    device.init(0)
    return device


def identity(n):
    return torch.arange(n, dtype=torch.int32, device="cuda")


def parse(dev, body, n_cols, col_map=None, ld=None, row0=0, max_rows=None, with_host=True):
    """One call of parse_table_into over `body`: (the whole of out as bits, rows, label ranges, the counters' deltas)."""
    host = np.frombuffer(body, dtype=np.uint8).copy()
    max_rows = max_rows or body.count(b"\n") + 1
    out = torch.full((n_cols, ld or max_rows), SENTINEL, dtype=torch.float64, device="cuda")
    before = dev.table_parse_stats()
    n, ranges = dev.parse_table_into(torch.from_numpy(host).cuda(), host if with_host else None, host.size, "\t", out, row0, max_rows,
                                     col_map=col_map)
    after = dev.table_parse_stats()
    return out.cpu().numpy().view(np.int64), n, ranges.tolist(), {k: after[k] - before[k] for k in COUNTERS}


def both(dev, body, n_cols, **kw):
    """The plain entry and the selected entry with the identity map: equal in everything; returns the plain result."""
    plain = parse(dev, body, n_cols, **kw)
    selected = parse(dev, body, n_cols, col_map=identity(n_cols), **kw)
    assert np.array_equal(plain[0], selected[0])
    assert plain[1:] == selected[1:]
    return plain


def table(n_rows, n_cols, seed):
    pick = np.random.default_rng(seed).integers(0, len(FIELDS), size=(n_rows, n_cols))
    body = "".join("\t".join([f"g{i}"] + [FIELDS[k] for k in pick[i]]) + "\n" for i in range(n_rows)).encode()
    return body, np.array([[float(FIELDS[k]) for k in row] for row in pick])


def as_bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


# ---------------------------------------------------------------------------------------------------------------- dense tables
def test_one_row_of_one_column(dev):
    bits, n, ranges, delta = both(dev, b"g\t5\n", 1, max_rows=1)
    assert n == 1 and ranges == [[0, 1]] and np.array_equal(bits, as_bits([[5.0]]))
    assert delta == {"rows": 1, "fields": 1, "host_parsed": 0, "bytes": 4, "collect_rounds": 0, "calls": 1}


def test_one_past_the_transpose_tile_and_a_reversed_map(dev):
    body, want = table(65, 65, seed=65)
    bits, n, ranges, delta = both(dev, body, 65, max_rows=65)
    assert n == 65 and np.array_equal(bits, as_bits(want.T))
    assert delta == {"rows": 65, "fields": 65 * 65, "host_parsed": 0, "bytes": len(body), "collect_rounds": 0, "calls": 1}
    reverse = list(range(64, -1, -1))
    got = parse(dev, body, 65, col_map=torch.tensor(reverse, dtype=torch.int32, device="cuda"), max_rows=65)
    plain = torch.from_numpy(bits.view(np.float64)).cuda()
    assert np.array_equal(got[0], dev.gather_matrix(plain, cells=reverse).cpu().numpy().view(np.int64))
    assert got[1:] == (n, ranges, delta)


@pytest.mark.parametrize("open_end", [False, True])
@pytest.mark.parametrize("n_bytes", [4095, 4096, 4097])
def test_chunk_sizes_around_one_segment(dev, n_bytes, open_end):
    """Position n is a position, so 4096 bytes are two segments.  The last row begins below 4060 and ends with the chunk: in
    4097 bytes it straddles the segments.  open_end: it has no line end and its last field is empty."""
    full = (n_bytes - 40) // 12
    tail = b"\t1\t2\t" if open_end else b"\t1\t2\t3\n"
    body = b"".join(b"r%04d\t4\t5\t6\n" % i for i in range(full))
    body += b"L" * (n_bytes - len(body) - len(tail)) + tail
    assert len(body) == n_bytes and 12 * full < 4060
    bits, n, ranges, delta = both(dev, body, 3)
    assert n == full + 1 and ranges[-1] == [12 * full, n_bytes - len(tail)]
    vals = bits.view(np.float64)
    assert np.array_equal(vals[:, :full], np.repeat([[4.0], [5.0], [6.0]], full, axis=1))
    assert vals[0, full] == 1.0 and vals[1, full] == 2.0 and (np.isnan(vals[2, full]) if open_end else vals[2, full] == 3.0)
    assert delta == {"rows": n, "fields": 3 * n, "host_parsed": 0, "bytes": n_bytes, "collect_rounds": 0, "calls": 1}


def test_blank_lines_only(dev):
    bits, n, ranges, delta = both(dev, b"\n\r\n\n", 2, max_rows=3)
    assert n == 0 and ranges == [] and np.array_equal(bits, as_bits(np.full((2, 3), SENTINEL)))
    assert delta == {"rows": 0, "fields": 0, "host_parsed": 0, "bytes": 4, "collect_rounds": 0, "calls": 1}


def test_rows_land_at_row0_of_a_wider_matrix(dev):
    body, want = table(4, 3, seed=4)
    bits, n, ranges, delta = both(dev, body, 3, ld=16, row0=3, max_rows=5)
    expect = np.full((3, 16), SENTINEL)
    expect[:, 3:7] = want.T
    assert n == 4 and np.array_equal(bits, as_bits(expect))
    starts = [0] + [i + 1 for i in range(len(body) - 1) if body[i:i + 1] == b"\n"]
    assert ranges == [[p, p + 2] for p in starts]                  # the labels g0 .. g3
    assert delta == {"rows": 4, "fields": 12, "host_parsed": 0, "bytes": len(body), "collect_rounds": 0, "calls": 1}


def test_the_library_fetches_the_text_for_an_uncertified_field(dev):
    body = ("a\t1\t2\nb\t%s\t3\n" % TIES[0]).encode()
    with_copy = both(dev, body, 2)
    fetched = both(dev, body, 2, with_host=False)
    assert np.array_equal(fetched[0], with_copy[0]) and fetched[1:] == with_copy[1:]
    assert fetched[3]["host_parsed"] == 1 and fetched[0].view(np.float64)[0, 1] == float(TIES[0])


# ---------------------------------------------------------------------------------------------------------------- triplets
def triplets(dev, body, G, C, size, offset, selected):
    host = np.frombuffer(body, dtype=np.uint8).copy()
    arrays = [torch.full((size,), -77, dtype=torch.int32, device="cuda") for _ in range(3)]
    kw = {"col_map": identity(C), "n_cols_out": C} if selected else {}
    got = dev.parse_triplets_into(torch.from_numpy(host).cuda(), host, host.size, _lib.MM_INTEGER, G, C, *arrays, offset, **kw)
    return got, [a.tolist() for a in arrays]


def test_the_identity_map_keeps_every_triplet(dev):
    rng = np.random.default_rng(22)
    ent = np.stack([rng.integers(1, 40, 700), rng.integers(1, 30, 700), rng.integers(0, 1000, 700)], axis=1)
    body = "".join("%d %d %d\n" % tuple(e) for e in ent).encode()
    assert len(body) > 4096
    n, plain = triplets(dev, body, 39, 29, 702, 1, selected=False)
    (kept, seen), selected = triplets(dev, body, 39, 29, 702, 1, selected=True)
    assert n == kept == seen == 700 and plain == selected
    assert plain[0] == [-77] + (ent[:, 0] - 1).tolist() + [-77] and plain[1] == [-77] + (ent[:, 1] - 1).tolist() + [-77]
    assert plain[2] == [-77] + ent[:, 2].tolist() + [-77]


@pytest.mark.parametrize("capacity", [0, 2])
def test_blank_triplet_lines_only(dev, capacity):
    n, plain = triplets(dev, b"\n\r\n\n", 5, 5, 2, 2 - capacity, selected=False)
    pair, selected = triplets(dev, b"\n\r\n\n", 5, 5, 2, 2 - capacity, selected=True)
    assert n == 0 and pair == (0, 0) and plain == selected == [[-77, -77]] * 3


def test_one_triplet_more_than_the_arrays_hold(dev):
    body = b"1 1 5\n2 3 6\n3 5 7\n"
    for selected, text in ((False, "parse_triplets: the chunk has 3 entries, capacity is 2"),
                           (True, "parse_triplets_cols: 3 entries are kept, capacity is 2")):
        host = np.frombuffer(body, dtype=np.uint8).copy()
        arrays = [torch.full((3,), -77, dtype=torch.int32, device="cuda") for _ in range(3)]
        kw = {"col_map": identity(5), "n_cols_out": 5} if selected else {}
        with pytest.raises(_lib.IcnvError, match=text):
            dev.parse_triplets_into(torch.from_numpy(host).cuda(), host, host.size, _lib.MM_INTEGER, 3, 5, *arrays, 1, **kw)
        assert all(a.tolist() == [-77] * 3 for a in arrays)
