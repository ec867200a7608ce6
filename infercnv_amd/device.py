"""Device-resident entry points: thin wrappers that hand torch CUDA tensors'
data pointers to the C ABI (`*_dev` functions of include/icnv.h).

PyTorch is used only for device memory, streams and (in `sharded.py`)
torch.distributed -- all arithmetic happens in libicnv_hip.so.

Layout: an expression matrix is a contiguous float64 tensor of shape
(C cells, G genes): row-major (C, G) is byte-identical to R's column-major
genes x cells `expr.data` (R/inferCNV.R:18), i.e. element (gene g, cell c) sits
at offset g + G*c.  State matrices are uint8 (C, G).
"""
from __future__ import annotations

import ctypes as ct
import functools
import os

import numpy as np
import torch

from . import _lib
from ._lib import Cfg, check, f64, i32, pack_groups
from .text_stream import LineChunks, _pinned


def _stream():
    return ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ct.c_void_p(t.data_ptr()) if t is not None else ct.c_void_p(0)


def _counters(name, fields, reset):
    """The int64 counters of icnv_<name>_stats as a dict keyed by `fields`; reset=True zeroes them afterwards
    (icnv_<name>_stats_reset)."""
    L = _lib.load()
    out = (ct.c_int64 * len(fields))()
    check(getattr(L, f"icnv_{name}_stats")(out, len(fields)))
    if reset:
        getattr(L, f"icnv_{name}_stats_reset")()
    return dict(zip(fields, (int(v) for v in out)))


def _check_matrix(x, dtype=torch.float64):
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == dtype and x.dim() == 2 and x.is_contiguous()):
        raise TypeError(f"expected a contiguous CUDA {dtype} tensor of shape (cells, genes)")
    return x.shape[0], x.shape[1]


def _check_matrix_ld(x, dtype=torch.float64):
    """(C, G, ld) of a CUDA matrix whose rows -- the cells -- are contiguous and lie `ld` elements apart: a contiguous
    (cells, genes) tensor (ld = G) or the [:, :G] view of a wider one (padded_matrix)."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == dtype and x.dim() == 2 and (x.shape[1] <= 1 or x.stride(1) == 1)
            and (x.shape[0] <= 1 or x.stride(0) >= x.shape[1])):
        raise TypeError(f"expected a CUDA {dtype} tensor of shape (cells, genes) with contiguous rows")
    return x.shape[0], x.shape[1], (x.stride(0) if x.shape[0] > 1 else x.shape[1])


def padded_matrix(C, G, dtype=torch.float64, device="cuda", multiple=16):
    """A (C, G) matrix whose rows start `ld = G rounded up to a multiple of 16` elements apart -- every cell on a cache line
    (float64) / a 16-byte word (uint8) of its own, whatever G is.  The per-cell Viterbi reads and writes such matrices at the
    speed of a gene count that is a multiple of 16 (icnv_viterbi_cells_ld_dev); ChainPlan.apply / smooth_chain write their
    HMM input into one when it is passed as `pre` (icnv_chain_apply_ld_dev).  The padding columns are never read or written."""
    ld = (int(G) + multiple - 1) // multiple * multiple
    return torch.empty((int(C), ld), dtype=dtype, device=device)[:, :int(G)]


def init(device=None):
    """Bind the calling thread to `device` (defaults to torch's current device)."""
    L = _lib.load()
    if device is None:
        device = torch.cuda.current_device()
    check(L.icnv_init(int(device)))
    if os.environ.get("ICNV_VITERBI_MODE"):     # developer switch: 1 = exact Viterbi kernel only (see viterbi_set_mode)
        check(L.icnv_viterbi_set_mode(int(os.environ["ICNV_VITERBI_MODE"])))


def release_pool():
    """Hand the library's cached device blocks (workspace pool, resident matrices, Viterbi tables) back to the driver
    (icnv_shutdown; the library stays usable, the next call allocates again).  For callers that need the whole HBM for
    one large matrix after smaller runs -- the 1 M-cell case holds 270 of the 288 GB."""
    torch.cuda.synchronize()
    _lib.load().icnv_shutdown()


# ------------------------------------------------------------------ smoothing chain
def smooth_chain(x, chr_start, ref_groups, window_length=101, max_thresh=3.0, use_bounds=True,
                 sd_amplifier=1.5, noise_filter=None, stage_mask=_lib.ST_ALL, out=None, want_pre_denoise=False,
                 inv_log=False):
    """Steps 8,9,10,11,12,14,22 of run() (R/inferCNV_ops.R:771-1589) fused on the
    GPU.  Returns (out, pre_denoise or None).  inv_log: the stand-alone
    subtract_ref_expr_from_obs(inv_log=TRUE) (stage_mask must be ST_SUBTRACT_REF_1 alone)."""
    L = _lib.load()
    C, G = _check_matrix(x)
    cfg = Cfg(G, C, chr_start, ref_groups, window_length, max_thresh, use_bounds, sd_amplifier, noise_filter,
              stage_mask, inv_log)
    if out is None:
        out = torch.empty_like(x)
    pre = torch.empty_like(x) if want_pre_denoise else None
    check(L.icnv_smooth_chain_dev(_ptr(x), _ptr(out), _ptr(pre), cfg.ptr(), _stream()))
    return out, pre


# ------------------------------------------------------------------ window smoothers of step 10 (DESIGN K16)
def smooth_windows(x, table, out=None):
    """The banded window operator of smooth_method "runmeans" / "coordinates" (icnv_smooth_windows_dev, DESIGN K16) on a
    (C, G) CUDA float64 matrix with contiguous rows (a padded_matrix is fine, for x and for out): out[c, g] = the sequential
    sum of x[c, lo[g] + t] * w[w_off[g] + t] over t < len[g], divided by denom[g].  table: smooth_windows.WindowTable in the
    matrix's gene order.  out must not overlap x.  A non-finite input value raises IcnvError.  Synchronises the stream."""
    L = _lib.load()
    C, G, ld = _check_matrix_ld(x)
    if table.G != G:
        raise ValueError(f"the table has {table.G} genes, the matrix {G}")
    if out is None:
        out = torch.empty((C, G), dtype=torch.float64, device=x.device)
    Co, Go, ld_out = _check_matrix_ld(out)
    if (Co, Go) != (C, G):
        raise ValueError("out must have the shape of x")
    lo, lop = i32(table.lo)
    ln, lnp = i32(table.len)
    den, denp = f64(table.denom)
    if table.w is not None:
        off = np.ascontiguousarray(table.w_off, dtype=np.int64)
        offp = off.ctypes.data_as(ct.POINTER(ct.c_int64))
        w, wp = f64(table.w)
    else:
        offp, wp = None, None
    check(L.icnv_smooth_windows_dev(_ptr(x), int(ld), _ptr(out), int(ld_out), G, C, lop, lnp, offp, wp, denp, _stream()))
    return out


SMOOTH_WINDOWS_STATS = ("calls", "tiles_lds", "tiles_spilled", "weighted_calls", "window_rows", "us")


def smooth_windows_stats(reset=False):
    """icnv_smooth_windows_stats as a dict (`us`: wall time of the calls in microseconds); reset=True zeroes the counters."""
    return _counters("smooth_windows", SMOOTH_WINDOWS_STATS, reset)


# ------------------------------------------------------------------ data layer of plot_cnv (DESIGN K17)
def quantiles_excluding_into(x, exclude, probs, quantiles, order_stats, counts, minmax):
    """icnv_quantiles_excluding_dev into caller-owned numpy arrays (float64 [n], float64 [2 n], int64 [2], float64 [2]; the
    last three may be None).  On an IcnvError they are left as they were."""
    L = _lib.load()
    C, G, ld = _check_matrix_ld(x)
    pr, prp = f64(probs)
    for a, dt in ((quantiles, np.float64), (order_stats, np.float64), (counts, np.int64), (minmax, np.float64)):
        if a is not None and not (isinstance(a, np.ndarray) and a.dtype == dt and a.flags.c_contiguous):
            raise TypeError("the outputs are contiguous numpy arrays of float64 / float64 / int64 / float64")
    if quantiles.size < pr.size or (order_stats is not None and order_stats.size < 2 * pr.size) or \
            (counts is not None and counts.size < 2) or (minmax is not None and minmax.size < 2):
        raise ValueError("an output array is too short")
    dp = lambda a: a.ctypes.data_as(ct.POINTER(ct.c_double)) if a is not None else None
    cp = counts.ctypes.data_as(ct.POINTER(ct.c_int64)) if counts is not None else None
    check(L.icnv_quantiles_excluding_dev(_ptr(x), int(ld), G, C, float(exclude), prp, int(pr.size), dp(quantiles), dp(order_stats),
                                         cp, dp(minmax), _stream()))


def quantiles_excluding(x, exclude, probs):
    """quantile(x[x != exclude], probs, type = 7) of a (C, G) CUDA float64 matrix with contiguous rows (a padded_matrix is
    fine), exactly and without a sort (icnv_quantiles_excluding_dev, DESIGN K17): the "auto" x.range of plot_cnv
    (R/inferCNV_heatmap.R:159).  exclude = NaN keeps every value; up to 8 probabilities per call.  Returns a dict of
    numpy values: quantiles [n], lo / hi [n] (the two order statistics each quantile interpolates), n_kept, n_excluded, min,
    max (over all values).  A non-finite value, no kept value or a probability outside [0, 1] raises IcnvError."""
    n = np.asarray(probs, dtype=np.float64).size
    q, st = np.zeros(n), np.zeros(2 * n)
    cnt, mm = np.zeros(2, dtype=np.int64), np.zeros(2)
    quantiles_excluding_into(x, exclude, probs, q, st, cnt, mm)
    return {"quantiles": q, "lo": st[0::2].copy(), "hi": st[1::2].copy(), "n_kept": int(cnt[0]), "n_excluded": int(cnt[1]),
            "min": float(mm[0]), "max": float(mm[1])}


def heatmap_bins(x, breaks, rows=None, out=None):
    """hist(x[rows, ], breaks)$counts after forcing every value into [breaks[0], breaks[-1]] (icnv_heatmap_bins_dev, DESIGN
    K17; R/inferCNV_heatmap.R:1934-1935, :2524): bin b holds breaks[b] < v <= breaks[b + 1], v == breaks[0] goes in bin 0.
    rows: 0-based cells in any order or subset (default: all).  Returns int64 numpy counts [len(breaks) - 1] (written into
    `out` when given; untouched on an IcnvError)."""
    L = _lib.load()
    C, G, ld = _check_matrix_ld(x)
    br, brp = f64(breaks)
    r, rp = i32(np.arange(C) if rows is None else rows)
    if out is None:
        out = np.zeros(max(br.size - 1, 1), dtype=np.int64)
    if not (isinstance(out, np.ndarray) and out.dtype == np.int64 and out.flags.c_contiguous and out.size >= br.size - 1):
        raise TypeError("out must be a contiguous int64 numpy array of len(breaks) - 1 entries")
    check(L.icnv_heatmap_bins_dev(_ptr(x), int(ld), G, C, rp, int(r.size), brp, int(br.size), out.ctypes.data_as(ct.POINTER(ct.c_int64)),
                                  _stream()))
    return out


def heatmap_raster(x, breaks, order, H, W, out=None):
    """The heatmap panel as an (H, W) CUDA uint8 image of bin indices (icnv_heatmap_raster_dev, DESIGN K17): pixel row i shows
    cell order[((2 i + 1) n) // (2 H)], pixel column j gene ((2 j + 1) G) // (2 W), binned as heatmap_bins bins.  order:
    0-based cells, top row first.  `out` (contiguous CUDA uint8 (H, W)) is untouched on an IcnvError."""
    L = _lib.load()
    C, G, ld = _check_matrix_ld(x)
    br, brp = f64(breaks)
    o, op = i32(order)
    if out is None:
        out = torch.empty((int(H), int(W)), dtype=torch.uint8, device=x.device)
    if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == (int(H), int(W))):
        raise TypeError("out must be a contiguous CUDA uint8 tensor of shape (H, W)")
    check(L.icnv_heatmap_raster_dev(_ptr(x), int(ld), G, C, op, int(o.size), brp, int(br.size), int(H), int(W), _ptr(out), _stream()))
    return out


HEATMAP_STATS = ("calls", "radix_passes", "candidates", "us")


def heatmap_stats(reset=False):
    """icnv_heatmap_stats as a dict (`us`: wall time of the calls in microseconds); reset=True zeroes the counters."""
    return _counters("heatmap", HEATMAP_STATS, reset)


# ------------------------------------------------------------------ matrix files of plot_cnv (DESIGN K20)
TABLE_ORIENTATIONS = {"gene_rows": _lib.TABLE_GENE_ROWS, "cell_rows": _lib.TABLE_CELL_ROWS}   # ICNV_TABLE_* of include/icnv.h


def pack_labels(labels):
    """Row labels (str or bytes, written as they are) as (uint8 bytes, int64 offsets [n + 1]) for format_table_into."""
    enc = [l if isinstance(l, bytes) else str(l).encode("utf-8") for l in labels]
    off = np.zeros(len(enc) + 1, dtype=np.int64)
    np.cumsum([len(b) for b in enc], out=off[1:])
    return np.frombuffer(b"".join(enc) + b"\0", dtype=np.uint8), off


def format_table_into(x, out, row0, n_rows, cells, orientation, packed_labels=None, sep=" "):
    """icnv_format_table_dev into `out`, a contiguous CUDA uint8 tensor whose size is the capacity: the file rows row0 ..
    row0 + n_rows - 1, as many as the call attempts and `out` holds.  cells: a contiguous int32 numpy array.  packed_labels:
    pack_labels() of the labels of ALL rows of the table (the range is cut out here), or None.  Returns (rows done, bytes,
    int64 row offsets [rows done + 1]).  Synchronises the stream."""
    L = _lib.load()
    C, G, ld = _check_matrix_ld(x)
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and out.dim() == 1 and out.is_contiguous()):
        raise TypeError("out must be a contiguous one-dimensional CUDA uint8 tensor")
    if not (isinstance(cells, np.ndarray) and cells.dtype == np.int32 and cells.flags.c_contiguous):
        raise TypeError("cells must be a contiguous int32 numpy array")
    sep_b = sep if isinstance(sep, bytes) else str(sep).encode("utf-8")
    row0, n_rows = int(row0), int(n_rows)
    labp, offp, off = None, None, None
    if packed_labels is not None:
        lab, off_all = packed_labels
        if row0 < 0 or n_rows < 0 or row0 + n_rows + 1 > off_all.size:
            raise ValueError("the labels do not cover the row range")
        off = np.ascontiguousarray(off_all[row0:row0 + n_rows + 1] - off_all[row0])
        offp = off.ctypes.data_as(ct.POINTER(ct.c_int64))
        labp = ct.c_void_p(lab.ctypes.data + int(off_all[row0]))
    offsets = np.zeros(max(n_rows, 0) + 1, dtype=np.int64)
    done, nbytes = ct.c_int64(0), ct.c_int64(0)
    check(L.icnv_format_table_dev(_ptr(x), int(ld), G, C, int(orientation), row0, n_rows, cells.ctypes.data_as(ct.POINTER(ct.c_int32)),
                                  int(cells.size), labp, offp, sep_b, _ptr(out), int(out.numel()),
                                  offsets.ctypes.data_as(ct.POINTER(ct.c_int64)), ct.byref(done), ct.byref(nbytes), _stream()))
    return int(done.value), int(nbytes.value), offsets[:int(done.value) + 1]


def format_table(x, *, rows, cells, orientation, labels=None, sep=" ", out=None, capacity=None):
    """A chunk of a matrix file as R's write.table prints it (icnv_format_table_dev, DESIGN K20): every number with 15
    significant digits, correctly rounded, trailing zeros dropped, fixed notation unless scientific is strictly narrower.
    x: (C, G) CUDA float64 with contiguous rows (a padded_matrix is fine).  orientation "gene_rows": file row i is gene i and
    its fields run over `cells` in the order given; "cell_rows": file row i is cell cells[i] and its fields run over all
    genes.  rows = (first file row, number of rows).  labels: one str or bytes per row of the range, written as it is before
    the row's first separator (None: no labels).  out: a CUDA uint8 tensor that serves as the device buffer (its size is the
    capacity; default: `capacity` bytes, or what the range needs when every field takes its 22 bytes).  Returns (bytes, rows
    done): the call stops before the first row that does not fit, and a caller goes on from there."""
    C, G, _ = _check_matrix_ld(x)
    row0, n_rows = (int(v) for v in rows)
    cells = np.ascontiguousarray(cells, dtype=np.int32)
    code = TABLE_ORIENTATIONS[orientation] if isinstance(orientation, str) else int(orientation)
    packed = None
    if labels is not None:
        if len(labels) != n_rows:
            raise ValueError("one label per row of the range")
        lab, off = pack_labels(labels)
        packed = (lab, np.concatenate([np.zeros(max(row0, 0), dtype=np.int64), off]))   # rows before the range: no bytes
    if out is None:
        if capacity is None:
            n_fields = cells.size if code == _lib.TABLE_GENE_ROWS else G
            capacity = max(n_rows, 1) * max(n_fields, 1) * 23 + (int(packed[1][-1]) + n_rows if packed else 0)
        out = torch.empty(max(int(capacity), 1), dtype=torch.uint8, device=x.device)
    done, nbytes, _ = format_table_into(x, out, row0, n_rows, cells, code, packed, sep)
    return out[:nbytes].cpu().numpy().tobytes(), done


TABLE_TEXT_STATS = ("calls", "rows", "elements", "host_formatted", "bytes", "collect_rounds", "us")


def table_text_stats(reset=False):
    """icnv_table_text_stats as a dict (`host_formatted`: elements the digits pass could not certify, formatted by the host;
    `us`: wall time of the calls in microseconds); reset=True zeroes the counters."""
    return _counters("table_text", TABLE_TEXT_STATS, reset)


# ------------------------------------------------------------------ CNV region reports (DESIGN K24)
REPORT_KINDS = {"genes": _lib.REPORT_GENES, "regions": _lib.REPORT_REGIONS}   # ICNV_REPORT_* of include/icnv.h
CNV_REPORT_STATS = ("calls", "records", "lines", "bytes", "us")


def _packed(table, name):
    b, off = table
    if not (isinstance(b, np.ndarray) and b.dtype == np.uint8 and b.flags.c_contiguous and isinstance(off, np.ndarray)
            and off.dtype == np.int64 and off.flags.c_contiguous and off.size >= 1 and b.size >= int(off[-1])):
        raise TypeError(f"{name} must be pack_labels() output: (uint8 bytes, int64 offsets)")
    return b, off


class CnvReportPlan:
    """One report file of generate_cnv_region_reports on the device (icnv_cnv_report_begin_dev .. _end, DESIGN K24).
    kind: "genes" (<prefix>.pred_cnv_genes.dat, a line per gene of every record) or "regions" (.pred_cnv_regions.dat, a line
    per record).  records: the int32 (6, n) CUDA tensor cnv_runs() returned (rows may lie further apart than n); groups,
    chrs, genes: pack_labels() of the cell-group names by list position, the chromosome names by chromosome index and the gene
    names in the gene order the records count in; start, end: int64 numpy arrays in that order.  The tables go to the device
    once; total_bytes, total_lines and max_record_bytes describe the whole body.  format_into() writes chunks of whole
    records; close() (or the with statement) frees the plan."""

    def __init__(self, kind, records, groups, chrs, genes, start, end):
        L = _lib.load()
        code = REPORT_KINDS[kind] if isinstance(kind, str) else int(kind)
        if not (isinstance(records, torch.Tensor) and records.is_cuda and records.dtype == torch.int32 and records.dim() == 2
                and records.shape[0] == 6 and (records.shape[1] <= 1 or records.stride(1) == 1)):
            raise TypeError("records must be the int32 (6, n) CUDA tensor of cnv_runs()")
        n = int(records.shape[1])
        stride = int(records.stride(0))
        if stride < n:
            raise TypeError("the rows of records overlap")
        self._tables = [_packed(groups, "groups"), _packed(chrs, "chrs"), _packed(genes, "genes")]
        G = self._tables[2][1].size - 1
        self._pos = [np.ascontiguousarray(start, dtype=np.int64), np.ascontiguousarray(end, dtype=np.int64)]
        if self._pos[0].shape != (G,) or self._pos[1].shape != (G,):
            raise ValueError("one start and one end per gene name")
        self._records = records                     # the plan reads them until close()
        self.n_records = n
        self._h = ct.c_void_p()
        totals = (ct.c_int64 * 3)()
        i64p = ct.POINTER(ct.c_int64)
        tab = [x for b, off in self._tables for x in (ct.c_void_p(b.ctypes.data), off.ctypes.data_as(i64p), off.size - 1)]
        rc = L.icnv_cnv_report_begin_dev(ct.byref(self._h), code, _ptr(records), stride, n, *tab[:8], self._pos[0].ctypes.data_as(i64p),
                                         self._pos[1].ctypes.data_as(i64p), G, totals, _stream())
        if rc == _lib.ERR_ARG:
            raise ValueError(L.icnv_last_error().decode("utf-8", "replace"))
        check(rc)
        self.total_bytes, self.total_lines, self.max_record_bytes = (int(v) for v in totals)

    def format_into(self, out, rec0):
        """icnv_cnv_report_format_dev: the records rec0 .. into `out`, a contiguous CUDA uint8 tensor whose size is the
        capacity, as many whole records as it holds.  Returns (records done, bytes, int64 record offsets [done + 1]).
        Synchronises the stream."""
        L = _lib.load()
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and out.dim() == 1 and out.is_contiguous()):
            raise TypeError("out must be a contiguous one-dimensional CUDA uint8 tensor")
        rec0 = int(rec0)
        offsets = np.zeros(max(self.n_records - rec0, 0) + 1, dtype=np.int64)
        done, nbytes = ct.c_int64(0), ct.c_int64(0)
        check(L.icnv_cnv_report_format_dev(self._h, rec0, _ptr(out), int(out.numel()), offsets.ctypes.data_as(ct.POINTER(ct.c_int64)),
                                           ct.byref(done), ct.byref(nbytes), _stream()))
        return int(done.value), int(nbytes.value), offsets[:int(done.value) + 1]

    def close(self):
        if self._h:
            _lib.load().icnv_cnv_report_end(self._h)
            self._h = ct.c_void_p()
        self._records = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def cnv_report(kind, records, groups, chrs, genes, start, end, capacity=None):
    """The whole body of one report file as bytes (CnvReportPlan, chunk after chunk of `capacity` bytes): for tests and small
    reports; generate_cnv_region_reports streams the chunks to the file instead."""
    with CnvReportPlan(kind, records, groups, chrs, genes, start, end) as plan:
        if plan.n_records == 0:
            return b""
        cap = max(int(capacity) if capacity is not None else plan.total_bytes, 1)
        out = torch.empty(cap, dtype=torch.uint8, device=records.device)
        parts, rec = [], 0
        while rec < plan.n_records:
            done, nbytes, _ = plan.format_into(out, rec)
            parts.append(out[:nbytes].cpu().numpy().tobytes())
            rec += done
        return b"".join(parts)


def cnv_report_stats(reset=False):
    """icnv_cnv_report_stats as a dict (`calls`: format calls; `us`: their wall time in microseconds); reset=True zeroes the
    counters."""
    return _counters("cnv_report", CNV_REPORT_STATS, reset)


# ------------------------------------------------------------------ count matrices from text (DESIGN K21)
TABLE_PARSE_STATS = ("calls", "rows", "fields", "host_parsed", "bytes", "collect_rounds", "us")
READ_TABLE_CHUNK = 64 << 20        # bytes of one chunk of read_table; ICNV_READ_TABLE_CHUNK (developer switch) overrides it


def table_parse_stats(reset=False):
    """icnv_table_parse_stats as a dict (`host_parsed`: fields the parse pass could not certify, parsed by the host's strtod;
    `us`: wall time of the calls in microseconds); reset=True zeroes the counters."""
    return _counters("table_parse", TABLE_PARSE_STATS, reset)


def _host_text_ptr(host):
    """The host copy of a chunk for the parse entries, or NULL: the chunk is a piece of a file inflated on the device (K30), and
    the library fetches it from text_dev if a field it cannot certify or a refusal asks for it."""
    return None if host is None else ct.c_void_p(host.ctypes.data)


def _check_text(text_dev, text_host, n_bytes):
    """The argument checks the parse entries share: the host copy of the chunk as a numpy array, or None."""
    if not (isinstance(text_dev, torch.Tensor) and text_dev.is_cuda and text_dev.dtype == torch.uint8 and text_dev.dim() == 1
            and text_dev.is_contiguous()):
        raise TypeError("text_dev must be a contiguous one-dimensional CUDA uint8 tensor")
    host = text_host.numpy() if isinstance(text_host, torch.Tensor) else text_host
    if host is not None and not (isinstance(host, np.ndarray) and host.dtype == np.uint8 and host.ndim == 1 and host.flags.c_contiguous):
        raise TypeError("text_host must be a contiguous one-dimensional uint8 array, or None")
    n_bytes = int(n_bytes)
    if n_bytes < 1 or n_bytes > text_dev.numel() or (host is not None and n_bytes > host.size):
        raise ValueError("n_bytes must be 1 .. the size of both copies of the text")
    return host


def parse_table_into(text_dev, text_host, n_bytes, sep, out, row0, max_rows, line0=1, col_map=None):
    """icnv_parse_table_dev: the first n_bytes of `text_dev` (contiguous CUDA uint8) and of `text_host` (a contiguous uint8
    numpy array or CPU tensor with the same bytes) are whole lines of a table with out.shape[0] numeric columns; row i of them
    goes to out[:, row0 + i].  out: a CUDA float64 (n_cols, ld) tensor with contiguous rows.  Returns (rows found, int64 label
    ranges [rows, 2] into the bytes).  text_host None: no host copy exists; the ranges then still include a label's quotes.  On an IcnvError `out` is as it was.  Synchronises the stream.
    With col_map (parse_table_cols_into), icnv_parse_table_cols_dev: the table has col_map.numel() numeric columns, of which the
    map selects out.shape[0]."""
    L = _lib.load()
    if col_map is not None and not (isinstance(col_map, torch.Tensor) and col_map.is_cuda and col_map.dtype == torch.int32 and col_map.dim() == 1
                                    and col_map.is_contiguous() and col_map.numel() >= 1):
        raise TypeError("col_map must be a contiguous one-dimensional CUDA int32 tensor")
    host = _check_text(text_dev, text_host, n_bytes)
    n_out, _, ld = _check_matrix_ld(out)
    row0, max_rows = int(row0), int(max_rows)
    if row0 < 0 or max_rows < 1 or row0 + max_rows > out.shape[1]:
        raise ValueError("rows row0 .. row0 + max_rows - 1 must be columns of out")
    if n_out == 1:
        ld = out.shape[1]
    sep_b = sep if isinstance(sep, bytes) else str(sep).encode("utf-8")
    ranges = np.zeros((max_rows, 2), dtype=np.int64)
    n_rows = ct.c_int64(0)
    n_cols = n_out if col_map is None else int(col_map.numel())
    args = (_ptr(text_dev), _host_text_ptr(host), int(n_bytes), sep_b, n_cols, int(line0), _ptr(out), int(ld), row0, max_rows,
            ranges.ctypes.data_as(ct.POINTER(ct.c_int64)), ct.byref(n_rows))
    if col_map is None:
        check(L.icnv_parse_table_dev(*args, _stream()))
    else:
        check(L.icnv_parse_table_cols_dev(*args, _ptr(col_map), n_out, _stream()))
    return int(n_rows.value), ranges[:int(n_rows.value)]


def _selected_columns(cells, who):
    """The `cells` argument of read_table / read_mtx as an int64 array: 0-based file columns, any order, no repeats."""
    sel = np.asarray(cells)
    if sel.ndim != 1 or sel.size == 0:
        raise ValueError(f"{who}: cells must be a non-empty list of columns")
    if not np.issubdtype(sel.dtype, np.integer):
        raise ValueError(f"{who}: cells must be integers")
    sel = sel.astype(np.int64)
    if sel.min() < 0:
        raise ValueError(f"{who}: cells entry {int(sel.min())} is negative")
    uniq, counts = np.unique(sel, return_counts=True)
    if uniq.size != sel.size:
        raise ValueError(f"{who}: cells lists column {int(uniq[counts > 1][0])} more than once")
    return sel


def _column_map(sel, n_cols, who, dev):
    """The device map of icnv_parse_*_cols_dev for the selection `sel` of a file with n_cols columns."""
    if int(sel.max()) >= n_cols:
        bad = int(sel[sel >= n_cols][0])
        raise ValueError(f"{who}: cells entry {bad} is not a column of the file, which has {n_cols}")
    col_map = np.full(n_cols, -1, dtype=np.int32)
    col_map[sel] = np.arange(sel.size, dtype=np.int32)
    return torch.from_numpy(col_map).to(dev)


def parse_table_cols_into(text_dev, text_host, n_bytes, sep, out, row0, max_rows, col_map, line0=1):
    """icnv_parse_table_cols_dev (DESIGN K26): parse_table_into for the columns a map selects.  col_map: a contiguous CUDA
    int32 vector with one entry per numeric column of the FILE, the row of `out` (out.shape[0] = n_cols_out) that column goes
    to, or -1.  The fields of skipped columns are not examined.  Returns (rows found, label ranges)."""
    if col_map is None:
        raise TypeError("col_map must be a contiguous one-dimensional CUDA int32 tensor")
    return parse_table_into(text_dev, text_host, n_bytes, sep, out, row0, max_rows, line0=line0, col_map=col_map)


def gather_matrix(x, genes=None, cells=None, out=None):
    """out[j, i] = x[cells[j], genes[i]] on the device (icnv_gather_matrix_dev): the kept, ordered genes and the kept cells of
    CreateInfercnvObject in one pass.  x: (C, G) CUDA float64 with contiguous rows; genes / cells: 0-based, any order, None for
    all of them in order.  Returns the contiguous (len(cells), len(genes)) tensor."""
    L = _lib.load()
    C, G, ld = _check_matrix_ld(x)
    g, gp = i32(genes) if genes is not None else (None, None)
    c, cp = i32(cells) if cells is not None else (None, None)
    ng, nc = (g.size if g is not None else G), (c.size if c is not None else C)
    if out is None:
        out = torch.empty((nc, ng), dtype=torch.float64, device=x.device)
    if _check_matrix(out) != (nc, ng):
        raise ValueError("out must have the shape (cells, genes) of the lists")
    check(L.icnv_gather_matrix_dev(_ptr(x), int(ld), G, C, gp, ng, cp, nc, _ptr(out), ng, _stream()))
    return out


# ------------------------------------------------------------------ exact sum of a matrix (DESIGN K23)
def matrix_sum(x):
    """The exact sum of a matrix, rounded to double once, to nearest with ties to even (icnv_matrix_sum_dev, DESIGN K23):
    math.fsum(x) wherever math.fsum returns, and the same rule where it raises "intermediate overflow".  x: a (C, G) CUDA
    float64 matrix with contiguous rows (a padded_matrix is fine: the padding is never read), or a 2-D float64 numpy array
    with contiguous rows, which the library uploads (icnv_matrix_sum).  Any NaN gives NaN, infinities of both signs NaN,
    of one sign that infinity; an exact sum beyond the double range +-Inf; a zero sum +0.0.  Synchronises the stream."""
    L = _lib.load()
    s = ct.c_double(0.0)
    if isinstance(x, np.ndarray):
        if not (x.dtype == np.float64 and x.ndim == 2 and x.size and (x.shape[1] <= 1 or x.strides[1] == 8)
                and (x.shape[0] <= 1 or (x.strides[0] % 8 == 0 and x.strides[0] >= 8 * x.shape[1]))):
            raise TypeError("expected a non-empty float64 numpy array of shape (cells, genes) with contiguous rows")
        C, G = x.shape
        ld = x.strides[0] // 8 if C > 1 else G
        check(L.icnv_matrix_sum(ct.c_void_p(x.ctypes.data), int(ld), G, C, ct.byref(s)))
    else:
        C, G, ld = _check_matrix_ld(x)
        check(L.icnv_matrix_sum_dev(_ptr(x), int(ld), G, C, ct.byref(s), _stream()))
    return s.value


def matrix_mean(x):
    """mean(expr.data) as plot_per_group and plot_cnv's default x.center take it: matrix_sum(x) / (G * C)."""
    return matrix_sum(x) / (x.shape[0] * x.shape[1])


# ------------------------------------------------------------------ reference z-score gene filter (DESIGN K32)
def zscore_gene_filter(x, ref_cells, row_mean=None):
    """(mean, sd, row_mean) of the reference-based gene filter of the subclustering (icnv_zscore_gene_filter_dev, DESIGN K32):
    mean and two-pass sd (n - 1) over all values of the listed cells of a (C, G) CUDA float64 matrix with contiguous rows, and
    per gene the mean over those cells of |(x - mean) / sd|, as a (G,) CUDA tensor.  Double-double sums rounded once, in a
    fixed order.  ref_cells: 0-based, any order, at least one.  Synchronises the stream."""
    L = _lib.load()
    C, G, ld = _check_matrix_ld(x)
    idx, ip = i32(ref_cells)
    if idx.ndim != 1:
        raise ValueError("ref_cells must be an index vector")
    if row_mean is None:
        row_mean = torch.empty(G, dtype=torch.float64, device=x.device)
    if not (isinstance(row_mean, torch.Tensor) and row_mean.is_cuda and row_mean.dtype == torch.float64 and row_mean.is_contiguous()
            and tuple(row_mean.shape) == (G,)):
        raise TypeError("row_mean must be a contiguous CUDA float64 tensor of G values")
    out = (ct.c_double * 2)(float("nan"), float("nan"))
    check(L.icnv_zscore_gene_filter_dev(_ptr(x), int(ld), G, C, ip, idx.size, out, _ptr(row_mean), _stream()))
    return out[0], out[1], row_mean


def _unquote(b):
    return b[1:-1] if len(b) >= 2 and b[:1] == b"\"" and b[-1:] == b"\"" else b


def _open_text(path, buffering=-1):
    """The file at `path` open for reading its bytes, decompressed by Python's gzip where the name ends in .gz."""
    import gzip
    return gzip.open(path, "rb") if str(path).endswith(".gz") else open(path, "rb", buffering=buffering)


def _count_newlines(path, n_bytes):
    """'\\n' among the first n_bytes of the (decompressed) file: the error path of read_table."""
    count = 0
    with _open_text(path) as f:
        while n_bytes > 0:
            block = f.read(min(n_bytes, 1 << 24))
            if not block:
                break
            count += block.count(b"\n")
            n_bytes -= len(block)
    return count


def _gunzip_text(path, stats):
    """The inflated text of a .gz path as a CUDA uint8 vector where gunzip.gunzip takes it (DESIGN K30), else None;
    stats["source"] says which: "device_gunzip", or "host" with the reason in stats["source_reason"]."""
    from . import gunzip
    stats["source"], stats["source_reason"] = "host", "not a .gz path"
    if not str(path).endswith(".gz"):
        return None
    if not gunzip.enabled():
        stats["source_reason"] = "switched off by ICNV_GUNZIP=0 or ICNV_INFLATE=0"
        return None
    text = gunzip.gunzip(path)
    if text is None:
        stats["source_reason"] = gunzip.gunzip_stats()["reason"]
        return None
    stats["source"], stats["source_reason"] = "device_gunzip", ""
    return text


def _dev_last_newline(text, lo, hi):
    """Index of the last '\\n' of the CUDA vector text[lo:hi], or lo - 1: 64 KiB pieces are fetched from the end."""
    while hi > lo:
        a = max(lo, hi - (1 << 16))
        hit = np.flatnonzero(text[a:hi].cpu().numpy() == 10)
        if hit.size:
            return a + int(hit[-1])
        hi = a
    return lo - 1


def _dev_line_chunks(text, pos, cap, stats):
    """(begin, end) of consecutive chunks of whole lines of text[pos:], each about cap bytes: longer where one line is."""
    n = int(text.numel())
    while pos < n:
        span = cap
        while True:
            end = min(n, pos + span)
            cut = n if end == n else _dev_last_newline(text, pos, end) + 1
            if cut > pos:
                break
            span *= 2                                              # one line is longer than the chunk: look further
            if "grown" in stats:
                stats["grown"] += 1
        yield pos, cut
        pos = cut


def _dev_aligned(text, a, b, stage):
    """text[a:b] where the parse entries can take it -- on a 16-byte boundary: the view itself, or a device-to-device copy.
    Returns (chunk, stage)."""
    if (text.data_ptr() + a) % 16 == 0:
        return text[a:b], stage
    if stage is None or stage.numel() < b - a:
        stage = torch.empty(b - a, dtype=torch.uint8, device=text.device)
    stage[:b - a].copy_(text[a:b])
    return stage[:b - a], stage


def _dev_labels(chunk, ranges):
    """The row names of a chunk that has no host copy: the label bytes gathered on the device, fetched in one piece, and the
    enclosing quotes dropped here (what tp_label_slice does where there is a host copy)."""
    lens = ranges[:, 1] - ranges[:, 0]
    total = int(lens.sum())
    raw = b""
    if total:
        lens_t = torch.from_numpy(lens).to(chunk.device)
        first = torch.from_numpy(np.ascontiguousarray(ranges[:, 0])).to(chunk.device) - (torch.cumsum(lens_t, 0) - lens_t)
        idx = torch.repeat_interleave(first, lens_t) + torch.arange(total, device=chunk.device)
        raw = chunk[idx].cpu().numpy().tobytes()
    out, o = [], 0
    for k in lens.tolist():
        out.append(_unquote(raw[o:o + k]).decode("utf-8", "surrogateescape"))
        o += k
    return out


def _table_columns(header_line, first_data_line, sep_b):
    """The names (bytes) of the numeric columns of a table: the header line (without its '\\n') has one name per numeric
    column, as write.table writes it, or one more with a corner label in front; the first line with data (None: the file has
    none) decides which.  Quotes around a name are dropped."""
    if first_data_line is None:
        raise ValueError("read_table: the file has no data row")
    line = header_line[:-1] if header_line.endswith(b"\r") else header_line
    header_names = [_unquote(t) for t in line.split(sep_b)]
    k = first_data_line.count(sep_b) + 1
    if len(header_names) == k - 1:
        col_names = header_names
    elif len(header_names) == k and k >= 2:
        col_names = header_names[1:]
    else:
        raise ValueError(f"read_table: the header has {len(header_names)} names, the first row has {k} fields")
    if len(col_names) < 1:
        raise ValueError("read_table: the table has no numeric column")
    return col_names


def _parse_table_chunk(chunk, host, nb, sep_b, scratch, col_map, file_line):
    """The nb bytes of whole lines at the start of `chunk` (on the device; host: the same bytes, or None) through
    parse_table_into -- with col_map where one is given -- into `scratch`, a (rows of x, any) CUDA float64 block
    that is replaced when the chunk may hold more rows than it has columns.  Returns (rows, label ranges, scratch).  A refusal
    is raised a second time with the file's line numbers; file_line() is then called for the lines of the file before the chunk."""
    n_cols = scratch.shape[0] if col_map is None else int(col_map.numel())
    max_rows = nb // (n_cols + 1) + 1                              # a row is at least its separators and its line end
    if scratch.shape[1] < max_rows:
        scratch = torch.empty((scratch.shape[0], max_rows), dtype=torch.float64, device=chunk.device)

    def parse(line0=1):
        return parse_table_into(chunk, host, nb, sep_b, scratch, 0, max_rows, line0=line0, col_map=col_map)
    try:
        rows, ranges = parse()
    except _lib.IcnvError as exc:
        short = "max_rows" in str(exc)                             # more lines than full rows fit: some row is too short
        if exc.code != _lib.ERR_ARG or not (short or "line " in str(exc)):
            raise
        if short:
            max_rows = int((chunk[:nb] == 10).sum()) + 1
            scratch = torch.empty((scratch.shape[0], max_rows), dtype=torch.float64, device=chunk.device)
        parse(line0=1 + file_line())                               # the refusal again, with the file's line number
        raise
    return rows, ranges, scratch


def _read_table_device(text, sep_b, cap0, sel, stats):
    """read_table's body for a file that lies inflated on the device: (row names, column names as bytes, parts).  The header
    and the first data line are fetched; the body goes to the parse entries as views or device-to-device copies of `text`."""
    import time
    dev, n = text.device, int(text.numel())
    fetch = 1 << 16
    while True:                                                    # the header line and the first line with data
        head = text[:min(n, fetch)].cpu().numpy().tobytes()
        lines = head.split(b"\n")
        data = [l for l in lines[1:-1] if l not in (b"", b"\r")] if len(head) < n else [l for l in lines[1:] if l not in (b"", b"\r")]
        if data or len(head) == n:
            break
        fetch *= 2
    col_names = _table_columns(lines[0], data[0] if data else None, sep_b)
    n_cols = len(col_names)
    col_map = None if sel is None else _column_map(sel, n_cols, "read_table", dev)
    scratch = torch.empty((n_cols if sel is None else sel.size, 0), dtype=torch.float64, device=dev)
    row_names, parts, stage = [], [], None
    for a, b in _dev_line_chunks(text, min(len(lines[0]) + 1, n), cap0, stats):
        t0 = time.perf_counter()
        chunk, stage = _dev_aligned(text, a, b, stage)
        rows, ranges, scratch = _parse_table_chunk(chunk, None, b - a, sep_b, scratch, col_map, lambda: int((text[:a] == 10).sum()))
        stats["parse_s"] += time.perf_counter() - t0
        if rows:
            parts.append(scratch[:, :rows].clone())
            row_names += _dev_labels(chunk, ranges)
        stats["chunks"] += 1
    stats["bytes"] = n
    return row_names, col_names, parts


def _table_result(row_names, col_names, parts, stats, before, t_start):
    import time
    if not parts:
        raise ValueError("read_table: the file has no data row")
    x = parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)
    x = x.contiguous()
    col_names = [c.decode("utf-8", "surrogateescape") for c in col_names]
    after = table_parse_stats()
    stats.update({k: after[k] - before[k] for k in TABLE_PARSE_STATS})
    torch.cuda.synchronize()                                       # the last chunk's copy and the concatenation are part of the total
    stats["wall_s"] = time.perf_counter() - t_start
    return row_names, col_names, x, stats


def read_table(path, sep="\t", chunk_bytes=None, cells=None):
    """read.table(path, sep = sep, header = TRUE, row.names = 1, check.names = FALSE) of a numeric table, parsed on the device
    (icnv_parse_table_dev, DESIGN K21; the grammar and what is refused: include/icnv.h "count matrices from text").
    Returns (row names, column names, x, stats): x is the (n_cols, n_rows) CUDA float64 tensor -- for a genes x cells file the
    (cells, genes) matrix every device.* entry takes --, stats a dict of counts and seconds (the counters of table_parse_stats
    for this call among them).

    The header line is read here: it has one name per numeric column, as write.table writes it, or one more with a corner
    label in front.  Quotes around a name are dropped.  The body is streamed in chunks of whole lines through two pinned and two
    device buffers: a thread (text_stream.LineChunks) reads chunk i + 1 from the file while chunk i is copied and parsed; a buffer grows when one line
    is longer than chunk_bytes.  A path that ends in .gz (R/inferCNV.R:146-150 reads it through gzfile) is first offered to
    gunzip.gunzip (DESIGN K30): a one-member gzip file of at least gunzip.GUNZIP_MIN_BYTES is inflated on the device, its header
    line and first data line are fetched, and the body goes to the same parse entries in chunks of whole lines that are views or
    device-to-device copies of the inflated tensor -- it does not cross PCIe (the last newline of a chunk is looked for in 64 KiB
    pieces; the row names are gathered on the device and fetched; a chunk comes to the host only when it holds a field the
    device pass cannot certify, or is refused).  stats["source"] is then "device_gunzip"; any other file -- stats["source"]
    "host", stats["source_reason"] why -- is decompressed by Python's gzip into the pinned chunks.  Both routes return the same
    values and the same refusals.  .rds is not read here (NotImplementedError): read_rds_counts reads it (DESIGN K34), and
    CreateInfercnvObject branches to it before this function.  A refused byte raises IcnvError
    with the file line and the field.

    cells (DESIGN K26): a list of 0-based numeric file columns, in any order, without repeats (ValueError before the file is
    opened for an empty list, a repeat or a negative entry; once the header is read for an entry that is no column, with the
    entry and the count).  Row k of x is then file column cells[k] -- x is (len(cells), n_rows), and so are the per-chunk
    scratch and parts --, through icnv_parse_table_cols_dev: the fields of the other columns are not examined, so a byte
    outside the grammar there is not reported.  All row names and ALL column names of the header still come back."""
    import time
    path = os.fspath(path)
    sel = None if cells is None else _selected_columns(cells, "read_table")
    if path.endswith(".rds"):
        raise NotImplementedError("read_table: .rds input is not read; pass the matrix as an array")
    sep_b = sep if isinstance(sep, bytes) else str(sep).encode("utf-8")
    if len(sep_b) != 1:
        raise ValueError("sep must be one byte")
    cap0 = max(64, int(chunk_bytes if chunk_bytes is not None else os.environ.get("ICNV_READ_TABLE_CHUNK", READ_TABLE_CHUNK)))
    dev = torch.device("cuda", torch.cuda.current_device())
    stats = {"bytes": 0, "chunks": 0, "read_s": 0.0, "parse_s": 0.0, "stall_s": 0.0, "grown": 0}
    before = table_parse_stats()
    t_start = time.perf_counter()
    text = _gunzip_text(path, stats)
    if text is not None:                                           # K30: the file lies inflated on the device; the body stays there
        return _table_result(*_read_table_device(text, sep_b, cap0, sel, stats), stats, before, t_start)
    copy_stream = torch.cuda.Stream(device=dev)
    dbuf = [None, None]

    def upload(job, start):
        slot, buf, n = job
        if dbuf[slot] is None or dbuf[slot].numel() < n - start:
            dbuf[slot] = torch.empty(max(cap0, n - start), dtype=torch.uint8, device=dev)
        event = torch.cuda.Event()
        with torch.cuda.stream(copy_stream):
            dbuf[slot][:n - start].copy_(buf[start:n], non_blocking=True)
            event.record(copy_stream)
        return event

    def next_newline(arr, p, n):
        while p < n:
            hi = min(n, p + (1 << 16))
            hit = np.flatnonzero(arr[p:hi] == 10)
            if hit.size:
                return p + int(hit[0])
            p = hi
        return n

    row_names, header_line, col_names, parts, scratch = [], None, None, [], None
    col_map = None                                                 # K26: the device map of the selection, once the columns are known
    offset, ahead = 0, None                                        # bytes of the file before this chunk; (job, event) copied ahead
    with _open_text(path, buffering=0) as f, LineChunks(f, cap0, stats) as chunks:
        try:
            job = chunks.get()
            while job is not None:
                slot, buf, n = job
                event, ahead = (ahead[1] if ahead is not None else None), None     # a copy ahead was this chunk's
                arr = buf.numpy()
                start = 0
                if header_line is None and n:
                    first = next_newline(arr, 0, n)
                    header_line = arr[:first].tobytes()
                    start = min(first + 1, n)
                p = start
                while p < n and col_names is None:                 # the first data line decides which header shape this is
                    e = next_newline(arr, p, n)
                    raw = arr[p:e].tobytes()
                    if raw not in (b"", b"\r"):
                        col_names = _table_columns(header_line, raw, sep_b)
                        if sel is not None:
                            col_map = _column_map(sel, len(col_names), "read_table", dev)
                        scratch = torch.empty((len(col_names) if sel is None else sel.size, 0), dtype=torch.float64, device=dev)
                    p = e + 1
                nb = n - start
                if col_names is not None and nb > 0:
                    if event is None:
                        event = upload(job, start)
                    t0 = time.perf_counter()
                    peek = chunks.get_nowait()                     # the next chunk's copy runs beside this parse
                    if peek is not None:
                        ahead = (peek, upload(peek, 0))
                    torch.cuda.current_stream().wait_event(event)
                    host = arr[start:n]
                    rows, ranges, scratch = _parse_table_chunk(dbuf[slot], host, nb, sep_b, scratch, col_map,
                                                               lambda: _count_newlines(path, offset + start))
                    stats["parse_s"] += time.perf_counter() - t0
                    if rows:
                        parts.append(scratch[:, :rows].clone())
                        for b, e in ranges.tolist():
                            row_names.append(host[b:e].tobytes().decode("utf-8", "surrogateescape"))
                    stats["chunks"] += 1
                offset += n
                stats["bytes"] += n
                chunks.release(slot)
                t0 = time.perf_counter()
                job = ahead[0] if ahead is not None else chunks.get()
                stats["stall_s"] += time.perf_counter() - t0
        finally:
            torch.cuda.synchronize()                               # a copy ahead may still read a pinned buffer
    if col_names is None:
        parts = []
    return _table_result(row_names, col_names, parts, stats, before, t_start)


def smooth_chain_windows(x, chr_start, ref_groups, table, max_thresh=3.0, use_bounds=True, sd_amplifier=1.5, noise_filter=None,
                         denoise=True, want_pre_denoise=False):
    """smooth_chain with step 10 replaced by the window operator (smooth_method "runmeans" / "coordinates"): the chain with
    steps 8 and 9, smooth_windows(table), then the chain with steps 11, 12, 14 (and 22) -- three library calls, the matrix
    never leaves the device.  max_thresh None skips step 9.  Returns (out, pre_denoise or None)."""
    m1 = _lib.ST_SUBTRACT_REF_1 | (0 if max_thresh is None else _lib.ST_MAX_THRESH)
    m2 = _lib.ST_CENTER | _lib.ST_SUBTRACT_REF_2 | _lib.ST_INVERT_LOG2 | (_lib.ST_DENOISE if denoise else 0)
    a, _ = smooth_chain(x, chr_start, ref_groups, max_thresh=max_thresh, use_bounds=use_bounds, stage_mask=m1)
    b = smooth_windows(a, table)
    return smooth_chain(b, chr_start, ref_groups, use_bounds=use_bounds, sd_amplifier=sd_amplifier, noise_filter=noise_filter,
                        stage_mask=m2, out=a, want_pre_denoise=want_pre_denoise and denoise)


class ChainPlan:
    """Split-phase chain (icnv_chain_* in include/icnv.h) for cell-sharded runs:
    for each reference round r: partial(r) -> all-reduce(sum) -> finish(r); then apply()."""

    def __init__(self, G, C, chr_start, ref_groups_local, **kw):
        self.L = _lib.load()
        self.cfg = Cfg(G, C, chr_start, ref_groups_local, **kw)
        h = ct.c_void_p()
        check(self.L.icnv_chain_begin(ct.byref(h), self.cfg.ptr()))
        self.h = h
        self.G, self.C = G, C

    @property
    def num_rounds(self):
        return self.L.icnv_chain_num_rounds(self.h)

    def round_partial(self, r, x):
        """Enqueue this rank's partial statistic; returns a float64 CUDA tensor
        *view* of the library's buffer (all-reduce it in place)."""
        p, n = ct.c_void_p(), ct.c_int64()
        check(self.L.icnv_chain_round_partial_dev(self.h, r, _ptr(x), ct.byref(p), ct.byref(n), _stream()))
        return _wrap_f64(p.value, n.value, x.device)

    def round_finish(self, r):
        check(self.L.icnv_chain_round_finish_dev(self.h, r, _stream()))

    def apply(self, x, out=None, want_pre_denoise=False, pre=None):
        """`pre`: a preallocated tensor for the matrix before step 22 (implies want_pre_denoise); a padded_matrix() is
        written with its leading dimension (icnv_chain_apply_ld_dev)."""
        if out is None:
            out = torch.empty_like(x)
        if pre is None and want_pre_denoise:
            pre = torch.empty_like(x)
        if pre is not None and not pre.is_contiguous():
            _, G, ld = _check_matrix_ld(pre)
            assert G == self.G and pre.shape[0] == self.C
            check(self.L.icnv_chain_apply_ld_dev(self.h, _ptr(x), _ptr(out), _ptr(pre), int(ld), _stream()))
            return out, pre
        check(self.L.icnv_chain_apply_dev(self.h, _ptr(x), _ptr(out), _ptr(pre), _stream()))
        return out, pre

    def denoise_params(self):
        buf = (ct.c_double * 2)()
        check(self.L.icnv_chain_get_denoise(self.h, buf, _stream()))
        return buf[0], buf[1]

    def close(self):
        if self.h:
            self.L.icnv_chain_end(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _DevView:
    """Expose a raw device pointer through __cuda_array_interface__."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (ptr, False), "version": 2}


def _wrap_f64(ptr, n, device):
    return torch.as_tensor(_DevView(ptr, n), device=device)


def remove_outliers(x, lower=None, upper=None, out=None):
    """remove_outliers_norm (R/inferCNV_ops.R:1969-2054) on a device-resident (C, G) matrix; bounds None = "average_bound".
    Returns (matrix, (lower, upper) used)."""
    L = _lib.load()
    C, G = x.shape
    if out is None:
        out = torch.empty_like(x)
    used = (ct.c_double * 2)()
    nan = float("nan")
    check(L.icnv_remove_outliers_dev(_ptr(x), _ptr(out), G, C, nan if lower is None else float(lower),
                                     nan if upper is None else float(upper), used, _stream()))
    return out, (used[0], used[1])


def average_bounds(x):
    """get_average_bounds (R/inferCNV_ops.R:2723-2742) -> (lower, upper)."""
    L = _lib.load()
    C, G = _check_matrix(x)
    out = (ct.c_double * 2)()
    check(L.icnv_average_bounds_dev(_ptr(x), G, C, out, _stream()))
    return out[0], out[1]


# ------------------------------------------------------------------ ingest (steps 3-4)
def col_sums(x):
    """colSums per cell (R/inferCNV_ops.R:3089) -> float64 (C,) tensor."""
    L = _lib.load()
    C, G = _check_matrix(x)
    out = torch.empty(C, dtype=torch.float64, device=x.device)
    check(L.icnv_col_sums_dev(_ptr(x), G, C, _ptr(out), _stream()))
    return out


def normalize_log2(x, col_sums_t=None, normalize_factor=None, do_normalize=True, do_log2=True, out=None):
    """normalize_counts_by_seq_depth + log2xplus1 (R/inferCNV_ops.R:3064-3111, 2756-2769).  With
    normalize_factor=None the factor is median(colSums) of THIS matrix; a cell-sharded caller
    all-gathers the column sums and passes the global median instead."""
    L = _lib.load()
    C, G = _check_matrix(x)
    if do_normalize and col_sums_t is None:
        col_sums_t = col_sums(x)
    if do_normalize and normalize_factor is None:
        srt = torch.sort(col_sums_t).values
        n = srt.numel()
        normalize_factor = float(srt[n // 2]) if n % 2 else float((srt[n // 2 - 1] + srt[n // 2]) * 0.5)
    if out is None:
        out = torch.empty_like(x)
    check(L.icnv_normalize_log2_dev(_ptr(x), _ptr(out), G, C, _ptr(col_sums_t), float(normalize_factor or 0.0),
                                    int(do_normalize), int(do_log2), _stream()))
    return out


# ------------------------------------------------------------------ HMM
def viterbi_cells(x, chr_start, means, sd_shared, logPi, logDelta, states=None):
    """predict_CNV_via_HMM_on_indiv_cells (R/inferCNV_HMM.R:284-324) / i3 variant
    (R/inferCNV_i3HMM.R:180-225).  Returns (states uint8 (C, G), n_underflow int32[1] tensor)."""
    L = _lib.load()
    C, G, ld_x = _check_matrix_ld(x)
    cs, cp = i32(chr_start)
    m, mp = f64(means)
    lp = np.asfortranarray(logPi, dtype=np.float64)
    ld, ldp = f64(logDelta)
    if states is None:
        # (a padded input gets padded states: the traceback then writes aligned 16-byte words for every cell)
        states = torch.empty((C, G), dtype=torch.uint8, device=x.device) if ld_x == G else padded_matrix(C, G, torch.uint8, x.device)
    _, Gs, ld_st = _check_matrix_ld(states, torch.uint8)
    assert Gs == G and states.shape[0] == C
    bad = torch.zeros(1, dtype=torch.int32, device=x.device)
    if ld_x == G and ld_st == G:
        check(L.icnv_viterbi_cells_dev(_ptr(x), _ptr(states), G, C, cp, cs.size - 1, m.size, mp, float(sd_shared),
                                       lp.ctypes.data_as(ct.POINTER(ct.c_double)), ldp, _ptr(bad), _stream()))
    else:
        check(L.icnv_viterbi_cells_ld_dev(_ptr(x), int(ld_x), _ptr(states), int(ld_st), G, C, cp, cs.size - 1, m.size, mp,
                                          float(sd_shared), lp.ctypes.data_as(ct.POINTER(ct.c_double)), ldp, _ptr(bad), _stream()))
    return states, bad


def viterbi_set_mode(mode):
    """0 = auto (certified fast path when the parameters are eligible), 1 = exact kernel only, 2 = auto without the
    staged fast kernel (developer A/B)."""
    check(_lib.load().icnv_viterbi_set_mode(int(mode)))


def viterbi_last_stats():
    """{path, sequences, flagged, table_intervals, fallback} of the last per-cell Viterbi call on this device
    (synchronises with it).  path "fast": the certified fast kernel ran; fallback: its last column batch had so many
    flagged sequences that the exact kernel recomputed the whole batch (decided on the device, per batch)."""
    buf = (ct.c_int64 * 4)()
    check(_lib.load().icnv_viterbi_last_stats(buf))
    return {"path": "fast" if buf[0] >= 1 else "exact", "sequences": int(buf[1]), "flagged": int(buf[2]),
            "table_intervals": int(buf[3]), "fallback": buf[0] == 2,
            # which fast kernel: "staged" (observations through LDS, short table), "register" (full table), "staged+register"
            # (the staged kernel's batch left its table and was redone with the full one)
            "kernel": {0: "exact", 1: "register", 2: "exact", 3: "staged", 4: "staged+register"}[int(buf[0])]}


def viterbi_groups(x, chr_start, groups, means, sd_shared_per_group, logPi, logDelta, states=None):
    """predict_CNV_via_HMM_on_tumor_subclusters / _whole_tumor_samples
    (R/inferCNV_HMM.R:345-408, 509-567; i3: R/inferCNV_i3HMM.R:249-389)."""
    L = _lib.load()
    C, G = _check_matrix(x)
    cs, cp = i32(chr_start)
    idx, off = pack_groups(groups)
    idx, ip = i32(idx)
    off, op = i32(off)
    m, mp = f64(means)
    sd, sdp = f64(sd_shared_per_group)
    lp = np.asfortranarray(logPi, dtype=np.float64)
    ld, ldp = f64(logDelta)
    if states is None:
        states = torch.empty((C, G), dtype=torch.uint8, device=x.device)
    bad = torch.zeros(1, dtype=torch.int32, device=x.device)
    check(L.icnv_viterbi_groups_dev(_ptr(x), _ptr(states), G, C, cp, cs.size - 1, ip, op, len(groups), m.size, mp,
                                    sdp, lp.ctypes.data_as(ct.POINTER(ct.c_double)), ldp, _ptr(bad), _stream()))
    return states, bad


class GroupHMMPlan:
    """The i3 HMM at group level with device-resident parameters (icnv_group_hmm_* in include/icnv.h): the group structure is
    uploaded once; `i3_partial(x)` returns the three shifted moments as a CUDA tensor view (all-reduce it in place in a
    cell-sharded run), `i3_finish(states, ...)` derives mu / sigma / delta on the device and runs the Viterbi + broadcast.
    No host round trip inside a step."""

    def __init__(self, G, C, chr_start, groups, ref_cells):
        self.L = _lib.load()
        self.G, self.C = int(G), int(C)
        self.cs, cp = i32(chr_start)
        idx, off = pack_groups(groups)
        self.idx, ip = i32(idx)
        self.off, op = i32(off)
        self.ref, rp = i32(ref_cells)
        h = ct.c_void_p()
        check(self.L.icnv_group_hmm_begin(ct.byref(h), self.G, self.C, cp, self.cs.size - 1, ip, op, len(groups), rp, self.ref.size))
        self.h = h

    def i3_partial(self, x):
        C, G = _check_matrix(x)
        assert (C, G) == (self.C, self.G)
        p = ct.c_void_p()
        check(self.L.icnv_group_hmm_i3_partial_dev(self.h, _ptr(x), ct.byref(p), _stream()))
        return _wrap_f64(p.value, 3, x.device)

    def i3_finish(self, logPi, logDelta, z_abs, delta_abs=None, states=None, device=None):
        if states is None:
            states = torch.empty((self.C, self.G), dtype=torch.uint8, device=device or "cuda")
        lp = np.asfortranarray(logPi, dtype=np.float64)
        ld, ldp = f64(logDelta)
        check(self.L.icnv_group_hmm_i3_finish_dev(self.h, _ptr(states), lp.ctypes.data_as(ct.POINTER(ct.c_double)), ldp, float(z_abs),
                                                  float("nan") if delta_abs is None else float(delta_abs), None, _stream()))
        return states

    def i3_params(self):
        """(mu, sigma, delta) of the last finish (synchronises)."""
        buf = (ct.c_double * 3)()
        check(self.L.icnv_group_hmm_get_i3_params(self.h, buf, _stream()))
        return buf[0], buf[1], buf[2]

    def close(self):
        if self.h:
            self.L.icnv_group_hmm_end(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def group_means(x, groups):
    """rowMeans(expr.data[, group]) per group -> (n_groups, G) tensor."""
    L = _lib.load()
    C, G = _check_matrix(x)
    idx, off = pack_groups(groups)
    idx, ip = i32(idx)
    off, op = i32(off)
    out = torch.empty((len(groups), G), dtype=torch.float64, device=x.device)
    check(L.icnv_group_means_dev(_ptr(x), G, C, ip, op, len(groups), _ptr(out), _stream()))
    return out


def cell_distances(x, cells):
    """parallelDist(t(expr.data[, cells])) (Euclidean; R/inferCNV_tumor_subclusters.R:191) -> (n, n) tensor."""
    L = _lib.load()
    C, G = _check_matrix(x)
    idx, ip = i32(cells)
    out = torch.empty((idx.size, idx.size), dtype=torch.float64, device=x.device)
    check(L.icnv_cell_distances_dev(_ptr(x), G, C, ip, idx.size, _ptr(out), _stream()))
    return out


def knn(x, problems, k):
    """Exact k nearest neighbours per problem: RANN::nn2(t(expr.data[genes, cells]), k = k)
    (R/inferCNV_tumor_subclusters.R:726) for a batch of problems in one call (icnv_knn_dev, DESIGN K8).

    problems: list of (genes, cells) 0-based index vectors (the gene order is the summation order).  Returns
    (nn_idx int32, nn_dist float64) CUDA tensors of shape (sum of the problems' cells, k), the rows packed by problem;
    nn_idx holds positions within the problem's cell list (R: 1-based cell numbers)."""
    L = _lib.load()
    C, G = _check_matrix(x)
    gidx, goff = pack_groups([g for g, _ in problems])
    cidx, coff = pack_groups([c for _, c in problems])
    gidx, gp = i32(gidx)
    goff, gop = i32(goff)
    cidx, cp = i32(cidx)
    coff, cop = i32(coff)
    n = int(coff[-1]) if coff.size else 0
    nn_idx = torch.empty((n, max(int(k), 0)), dtype=torch.int32, device=x.device)
    nn_dist = torch.empty((n, max(int(k), 0)), dtype=torch.float64, device=x.device)
    check(L.icnv_knn_dev(_ptr(x), G, C, gp, gop, cp, cop, len(problems), int(k), _ptr(nn_idx), _ptr(nn_dist), _stream()))
    return nn_idx, nn_dist


KNN_STATS = ("calls", "problems", "query_rows", "row_blocks", "screened_rows", "candidates", "overflow_rows",
             "exhaustive_rows", "forced_exhaustive_rows")


def knn_stats(reset=False):
    """icnv_knn_stats as a dict (synchronises the device); reset=True zeroes the counters afterwards."""
    return _counters("knn", KNN_STATS, reset)


HCLUST_METHODS = {"ward.D": 1, "ward.D2": 2, "single": 3, "complete": 4, "average": 5, "mcquitty": 6, "centroid": 7,
                  "median": 8}   # ICNV_HCLUST_* of include/icnv.h


def _hclust_code(method):
    """An R method name -> its ICNV_HCLUST_* code; an unknown name -> -1, which the library refuses (ICNV_ERR_UNSUPPORTED)."""
    return HCLUST_METHODS.get(method, -1) if isinstance(method, str) else int(method)


def hclust(dist, method="ward.D2"):
    """hclust(as.dist(dist), method) of an (n, n) CUDA float64 distance matrix (rows contiguous; fastcluster's hclust as the
    reference calls it, R/inferCNV_tumor_subclusters.R:191, R/inferCNV_ops.R:3242) by icnv_hclust_dev (DESIGN K9).
    Returns CUDA tensors (merge int32 (n-1, 2), height float64 (n-1,), order int32 (n,)) with R's values: merge rows as R
    stores them (singletons -(i+1), clusters by step), order 1-based.  Synchronises the device."""
    L = _lib.load()
    n, n2, ld = _check_matrix_ld(dist)
    if n != n2:
        raise ValueError("dist must be square")
    m = max(n - 1, 0)
    merge = torch.empty((2, m), dtype=torch.int32, device=dist.device)      # column-major (n-1) x 2
    height = torch.empty(m, dtype=torch.float64, device=dist.device)
    order = torch.empty(n, dtype=torch.int32, device=dist.device)
    check(L.icnv_hclust_dev(_ptr(dist), ld, n, _hclust_code(method), _ptr(merge), _ptr(height), _ptr(order), _stream()))
    return merge.t(), height, order


def hclust_cells(x, problems, method="ward.D2"):
    """hclust(parallelDist(t(expr.data[genes, cells])), method) for a batch of problems in one call (icnv_hclust_cells_dev,
    DESIGN K9): the distances bit-equal to R's sequential dist, the clustering in LDS or HBM, nothing but the result leaves the device.
    problems: list of (genes, cells) 0-based index vectors, at least two cells each.  Returns a list of (merge, height,
    order) CUDA tensors per problem, as `hclust` returns them."""
    L = _lib.load()
    C, G = _check_matrix(x)
    gidx, goff = pack_groups([g for g, _ in problems])
    cidx, coff = pack_groups([c for _, c in problems])
    gidx, gp = i32(gidx)
    goff, gop = i32(goff)
    cidx, cp = i32(cidx)
    coff, cop = i32(coff)
    cells = int(coff[-1]) if coff.size else 0
    merges = max(cells - len(problems), 0)
    merge = torch.empty(2 * merges, dtype=torch.int32, device=x.device)
    height = torch.empty(merges, dtype=torch.float64, device=x.device)
    order = torch.empty(cells, dtype=torch.int32, device=x.device)
    check(L.icnv_hclust_cells_dev(_ptr(x), G, C, gp, gop, cp, cop, len(problems), _hclust_code(method), _ptr(merge),
                                  _ptr(height), _ptr(order), _stream()))
    out = []
    for p in range(len(problems)):
        n = int(coff[p + 1] - coff[p])
        m0 = int(coff[p]) - p
        out.append((merge[2 * m0:2 * (m0 + n - 1)].view(2, n - 1).t(), height[m0:m0 + n - 1], order[int(coff[p]):int(coff[p + 1])]))
    return out


HCLUST_STATS = ("calls", "problems", "lds_problems", "hbm_problems", "chain_steps", "us")


def hclust_stats(reset=False):
    """icnv_hclust_stats as a dict (`us`: wall time of the calls in microseconds); reset=True zeroes the counters afterwards."""
    return _counters("hclust", HCLUST_STATS, reset)


def _u64(a):
    arr = np.ascontiguousarray(np.asarray(a, dtype=np.uint64))
    return arr, arr.ctypes.data_as(ct.POINTER(ct.c_uint64))


def random_trees(x, clades, tokens, window_size=101, n_iter=100, seed=0, method="ward.D2"):
    """The permutation statistic of the random-trees subclustering for a batch of clades in one call
    (icnv_random_trees_dev, DESIGN K10; R/inferCNV_tumor_subclusters.random_smoothed_trees.R:217-298): per clade the
    observed tree of its smoothed, median-centred cells and max(height) of n_iter trees of gene-wise permuted copies.
    clades: list of 0-based cell index vectors (>= 2 cells each); tokens: one uint64 per clade (the permutation stream's
    second key word).  Returns (trees, rand_max) -- trees a list of (merge, height, order) CUDA tensors per clade as
    `hclust` returns them, rand_max a CUDA float64 tensor (n_clades, n_iter).  Synchronises the device."""
    L = _lib.load()
    C, G = _check_matrix(x)
    if len(tokens) != len(clades):
        raise ValueError("one token per clade")
    cidx, coff = pack_groups(clades)
    cidx, cp = i32(cidx)
    coff, cop = i32(coff)
    tok, tp = _u64(tokens)
    P = len(clades)
    cells = int(coff[-1]) if coff.size else 0
    merges = max(cells - P, 0)
    merge = torch.empty(max(2 * merges, 1), dtype=torch.int32, device=x.device)
    height = torch.empty(max(merges, 1), dtype=torch.float64, device=x.device)
    order = torch.empty(max(cells, 1), dtype=torch.int32, device=x.device)
    rand = torch.empty((P, max(int(n_iter), 1)), dtype=torch.float64, device=x.device)
    check(L.icnv_random_trees_dev(_ptr(x), G, C, cp, cop, tp, P, int(window_size), int(n_iter), int(seed) & (2**64 - 1),
                                  _hclust_code(method), _ptr(merge), _ptr(height), _ptr(order), _ptr(rand), _stream()))
    trees = []
    for p in range(P):
        n = int(coff[p + 1] - coff[p])
        m0 = int(coff[p]) - p
        trees.append((merge[2 * m0:2 * (m0 + n - 1)].view(2, n - 1).t(), height[m0:m0 + n - 1], order[int(coff[p]):int(coff[p + 1])]))
    return trees, rand


def random_trees_matrix(x, cells, window_size=101, seed=0, token=0, iteration=-1, stages=_lib.RT_PERMUTE | _lib.RT_SMOOTH | _lib.RT_CENTER):
    """One (clade, iteration) matrix of `random_trees` after the stages in `stages` (_lib.RT_PERMUTE | RT_SMOOTH |
    RT_CENTER), as a CUDA (len(cells), G) float64 tensor (icnv_random_trees_matrix_dev).  iteration=-1: the observed matrix."""
    L = _lib.load()
    C, G = _check_matrix(x)
    cidx, cp = i32(cells)
    out = torch.empty((max(cidx.size, 1), G), dtype=torch.float64, device=x.device)
    check(L.icnv_random_trees_matrix_dev(_ptr(x), G, C, cp, int(cidx.size), int(window_size), int(seed) & (2**64 - 1),
                                         int(token) & (2**64 - 1), int(iteration), int(stages), _ptr(out), _stream()))
    return out[:cidx.size]


RANDOM_TREES_STATS = ("calls", "clades", "permuted", "waves", "chain_steps", "us")


def random_trees_stats(reset=False):
    """icnv_random_trees_stats as a dict (`us`: wall time of the calls in microseconds); reset=True zeroes the counters."""
    return _counters("random_trees", RANDOM_TREES_STATS, reset)


LEIDEN_OBJECTIVES = {"CPM": _lib.LEIDEN_CPM, "modularity": _lib.LEIDEN_MODULARITY}   # ICNV_LEIDEN_* of include/icnv.h


def _leiden_objective(objective):
    """An R objective_function name -> its ICNV_LEIDEN_* code; an unknown name -> -1, which the library refuses."""
    return LEIDEN_OBJECTIVES.get(objective, -1) if isinstance(objective, str) else int(objective)


def _leiden_offsets(nn_idx, sizes):
    if not (nn_idx.is_cuda and nn_idx.dtype == torch.int32 and nn_idx.dim() == 2 and nn_idx.is_contiguous()):
        raise ValueError("nn_idx must be a contiguous (sum n_p, k) int32 CUDA tensor")
    off = np.zeros(len(sizes) + 1, dtype=np.int64)
    off[1:] = np.cumsum(np.asarray(sizes, dtype=np.int64))
    if off[-1] != nn_idx.shape[0]:
        raise ValueError("the problem sizes must add up to the rows of nn_idx")
    return i32(off)


def leiden(nn_idx, sizes, objective, resolution, beta=0.01, n_iterations=2, seed=0, tokens=None):
    """cluster_leiden on the kNN graph of .leiden_simple_snn (R/inferCNV_tumor_subclusters.R:726-741) for a batch of problems
    in one call (icnv_leiden_dev, DESIGN K11).  nn_idx: the (sum n_p, k) int32 CUDA tensor of `knn` (positions within each
    problem); sizes: n_p per problem; objective "CPM" or "modularity"; resolution one gamma or one per problem; tokens one
    uint64 per problem (the stream's second key word, default 0).  Returns (membership, n_clusters): a 1-based int32 CUDA
    tensor (sum n_p,) and a numpy int32 array per problem.  Synchronises the device."""
    L = _lib.load()
    off, op = _leiden_offsets(nn_idx, sizes)
    P = len(sizes)
    res, rp = f64(np.broadcast_to(np.asarray(resolution, dtype=np.float64), (P,)))
    tok, tp = _u64([0] * P if tokens is None else tokens)
    if tok.size != P:
        raise ValueError("one token per problem")
    memb = torch.empty(max(int(off[-1]), 1), dtype=torch.int32, device=nn_idx.device)
    ncl = np.zeros(max(P, 1), dtype=np.int32)
    check(L.icnv_leiden_dev(_ptr(nn_idx), int(nn_idx.shape[1]), op, P, _leiden_objective(objective), rp, float(beta),
                            int(n_iterations), int(seed) & (2**64 - 1), tp, _ptr(memb), ncl.ctypes.data_as(_lib._ip), _stream()))
    return memb[:int(off[-1])], ncl[:P]


def snn_graph(nn_idx, sizes):
    """The graph of `leiden` as one CSR over the batch (icnv_snn_graph_dev): (row_off int64, col int32, strength int64) CUDA
    tensors; problem p's rows follow each other, columns are positions within the problem, rows ascending."""
    L = _lib.load()
    off, op = _leiden_offsets(nn_idx, sizes)
    n, k = int(off[-1]), int(nn_idx.shape[1])
    row_off = torch.empty(n + 1, dtype=torch.int64, device=nn_idx.device)
    col = torch.empty(max(2 * k * n, 1), dtype=torch.int32, device=nn_idx.device)
    strength = torch.empty(max(n, 1), dtype=torch.int64, device=nn_idx.device)
    check(L.icnv_snn_graph_dev(_ptr(nn_idx), k, op, len(sizes), _ptr(row_off), _ptr(col), _ptr(strength), _stream()))
    return row_off, col[:int(row_off[-1].item())], strength[:n]


def leiden_graph(row_off, col, weight, loop, sizes, objective, resolution, beta=0.01, n_iterations=2, seed=0, tokens=None,
                 loop_weight=_lib.SNN_WEIGHT_ONE):
    """`leiden` on a batch of weighted graphs instead of kNN blocks (icnv_leiden_graph_dev, DESIGN K18): the CSR of
    `snn_jaccard` -- row_off int64 (sum n_p + 1), col int32, weight int64, loop int32 (sum n_p) CUDA tensors.  For CPM the
    resolution is in units of the weights (the PCA route passes gamma * 2^24).  Returns (membership, n_clusters) as `leiden`."""
    L = _lib.load()
    for t, dt, name in ((row_off, torch.int64, "row_off"), (col, torch.int32, "col"), (weight, torch.int64, "weight"),
                        (loop, torch.int32, "loop")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dt and t.dim() == 1 and t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous 1-d {dt} CUDA tensor")
    off = np.zeros(len(sizes) + 1, dtype=np.int64)
    off[1:] = np.cumsum(np.asarray(sizes, dtype=np.int64))
    if off[-1] + 1 != row_off.shape[0] or loop.shape[0] < off[-1] or col.shape[0] != weight.shape[0]:
        raise ValueError("the problem sizes must add up to the rows of the CSR")
    off, op = i32(off)
    P = len(sizes)
    res, rp = f64(np.broadcast_to(np.asarray(resolution, dtype=np.float64), (P,)))
    tok, tp = _u64([0] * P if tokens is None else tokens)
    if tok.size != P:
        raise ValueError("one token per problem")
    if P and int(row_off[-1].item()) > col.shape[0]:
        raise ValueError("col and weight are shorter than row_off says")
    memb = torch.empty(max(int(off[-1]), 1), dtype=torch.int32, device=col.device)
    ncl = np.zeros(max(P, 1), dtype=np.int32)
    check(L.icnv_leiden_graph_dev(_ptr(row_off), _ptr(col), _ptr(weight), _ptr(loop), int(loop_weight), op, P,
                                  _leiden_objective(objective), rp, float(beta), int(n_iterations), int(seed) & (2**64 - 1), tp,
                                  _ptr(memb), ncl.ctypes.data_as(_lib._ip), _stream()))
    return memb[:int(off[-1])], ncl[:P]


def snn_jaccard(nn_idx, sizes):
    """Seurat's ComputeSNN (prune.SNN = 1/15) on the kNN blocks of `knn` (icnv_snn_begin_dev / _fill_dev, DESIGN K18).
    Returns (row_off int64, col int32, shared int32, weight int64, loop int32) CUDA tensors: one ascending CSR over the batch
    (problem p's rows follow each other, columns are positions within the problem), the shared-neighbour counts s, their
    24-bit fixed-point Jaccard weights s / (2 k - s) and the loop flags (always 1).  Synchronises the device."""
    L = _lib.load()
    off, op = _leiden_offsets(nn_idx, sizes)
    n, k = int(off[-1]), int(nn_idx.shape[1])
    h, nnz = ct.c_void_p(0), ct.c_int64(0)
    check(L.icnv_snn_begin_dev(_ptr(nn_idx), k, op, len(sizes), ct.byref(h), ct.byref(nnz), _stream()))
    try:
        dev = nn_idx.device
        row_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        col = torch.empty(max(nnz.value, 1), dtype=torch.int32, device=dev)
        shared = torch.empty(max(nnz.value, 1), dtype=torch.int32, device=dev)
        weight = torch.empty(max(nnz.value, 1), dtype=torch.int64, device=dev)
        loop = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        check(L.icnv_snn_fill_dev(h, _ptr(row_off), _ptr(col), _ptr(shared), _ptr(weight), _ptr(loop), _stream()))
    finally:
        L.icnv_snn_end(h)
    return row_off, col[:nnz.value], shared[:nnz.value], weight[:nnz.value], loop[:n]


def _lpca_lists(x, problems):
    C, G, ld = _check_matrix_ld(x)
    gidx, goff = pack_groups([g for g, _ in problems])
    cidx, coff = pack_groups([c for _, c in problems])
    return C, G, ld, i32(gidx), i32(goff), i32(cidx), i32(coff)


def _check_packed(t, n, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.numel() == n):
        raise ValueError(f"{name} must be a contiguous CUDA float64 tensor with one entry per (problem, gene)")


def lpca_vstd(x, problems, mean, sd):
    """The standardised variance of FindVariableFeatures (icnv_lpca_vstd_dev, DESIGN K18) for a batch of (genes, cells)
    problems: mean and sd = sqrt(10^trend) packed per (problem, gene) as CUDA float64 tensors; returns v_std packed likewise."""
    L = _lib.load()
    C, G, ld, (gi, gp), (go, gop), (ci, cp), (co, cop) = _lpca_lists(x, problems)
    n = int(go[-1]) if go.size else 0
    _check_packed(mean, n, "mean")
    _check_packed(sd, n, "sd")
    out = torch.empty(max(n, 1), dtype=torch.float64, device=x.device)
    check(L.icnv_lpca_vstd_dev(_ptr(x), G, C, ld, gp, gop, cp, cop, len(problems), _ptr(mean), _ptr(sd), _ptr(out), _stream()))
    return out[:n]


def lpca_z_layout(n_feat, n_cells):
    """(offsets int64 (P + 1), ldz int64 (P)) of the feature-major blocks of `lpca_scale`: F_p rows of ldz_p = n_p + (n_p & 1)."""
    n_cells = np.asarray(n_cells, dtype=np.int64)
    ldz = n_cells + (n_cells & 1)
    off = np.zeros(len(n_cells) + 1, dtype=np.int64)
    off[1:] = np.cumsum(np.asarray(n_feat, dtype=np.int64) * ldz)
    return off, ldz


def lpca_scale(x, problems, mean, sd):
    """ScaleData of the features (icnv_lpca_scale_dev, DESIGN K18): z = min(10, (x - mean) / sd), feature-major blocks packed
    as `lpca_z_layout` says.  problems: (features, cells); mean, sd packed per (problem, feature)."""
    L = _lib.load()
    C, G, ld, (gi, gp), (go, gop), (ci, cp), (co, cop) = _lpca_lists(x, problems)
    n = int(go[-1]) if go.size else 0
    _check_packed(mean, n, "mean")
    _check_packed(sd, n, "sd")
    off, _ = lpca_z_layout([len(g) for g, _ in problems], [len(c) for _, c in problems])
    Z = torch.empty(max(int(off[-1]), 1), dtype=torch.float64, device=x.device)
    check(L.icnv_lpca_scale_dev(_ptr(x), G, C, ld, gp, gop, cp, cop, len(problems), _ptr(mean), _ptr(sd), _ptr(Z), _stream()))
    return Z[:int(off[-1])]


def lpca_gram(Z, n_feat, n_cells):
    """M_p = Z_p Z_p^T on the matrix cores (icnv_lpca_gram_dev, DESIGN K18): the (F_p, F_p) blocks packed one after another."""
    L = _lib.load()
    off, _ = lpca_z_layout(n_feat, n_cells)
    _check_packed(Z, int(off[-1]), "Z")
    nf, nfp = i32(n_feat)
    nc, ncp = i32(n_cells)
    total = int(np.sum(nf.astype(np.int64) ** 2))
    M = torch.empty(max(total, 1), dtype=torch.float64, device=Z.device)
    check(L.icnv_lpca_gram_dev(_ptr(Z), nfp, ncp, nf.size, _ptr(M), _stream()))
    return M[:total]


def lpca_project(Z, V, n_feat, n_cells, npcs, e_ld=10):
    """E = Z^T V per problem (icnv_lpca_project_dev, DESIGN K18).  V: the (F_p, npcs_p) row-major blocks packed one after
    another (CUDA float64).  Returns the (sum n_p, e_ld) embedding matrix, rows in problem order, unused components zero."""
    L = _lib.load()
    off, _ = lpca_z_layout(n_feat, n_cells)
    _check_packed(Z, int(off[-1]), "Z")
    nf, nfp = i32(n_feat)
    nc, ncp = i32(n_cells)
    npc, npp = i32(npcs)
    _check_packed(V, int(np.sum(nf.astype(np.int64) * npc)), "V")
    E = torch.empty((max(int(nc.sum()), 1), int(e_ld)), dtype=torch.float64, device=Z.device)
    check(L.icnv_lpca_project_dev(_ptr(Z), _ptr(V), nfp, ncp, npp, nf.size, _ptr(E), int(e_ld), _stream()))
    return E[:int(nc.sum())]


LEIDEN_STATS = ("calls", "problems", "levels", "move_visits", "refine_visits", "draws", "us")


def leiden_stats(reset=False):
    """icnv_leiden_stats as a dict (`us`: wall time of the calls in microseconds); reset=True zeroes the counters."""
    return _counters("leiden", LEIDEN_STATS, reset)


DE_TESTS = {"wilcoxon": _lib.DE_WILCOXON, "t": _lib.DE_T}   # ICNV_DE_* of include/icnv.h
DE_RULES = {"any": _lib.DE_MASK_ANY, "most": _lib.DE_MASK_MOST, "all": _lib.DE_MASK_ALL}


def de_tests(x, groups, comparisons, test="wilcoxon", jitter=True, seed=0):
    """The per-gene tests of get_DE_genes_basic (R/inferCNV_mask_non_DE.R:157-258) for a batch of comparisons in one call
    (icnv_de_tests_dev, DESIGN K12).  x: (C, G) CUDA float64 matrix with contiguous rows; groups: list of 0-based cell index
    vectors; comparisons: (x group, y group) pairs = (normal type, subcluster); test "wilcoxon" or "t".  Returns (stat, p,
    padj) CUDA float64 tensors (n_cmp, G): W or t, the p-values and their BH adjustment per row.  Synchronises the device."""
    L = _lib.load()
    C, G, ld = _check_matrix_ld(x)
    code = DE_TESTS.get(test, -1) if isinstance(test, str) else int(test)
    cidx, coff = pack_groups(groups)
    cidx, cp = i32(cidx)
    coff, cop = i32(coff)
    cmp = np.asarray(comparisons, dtype=np.int32).reshape(-1, 2)
    cmp, mp = i32(cmp)
    n = max(cmp.shape[0], 1)
    stat = torch.empty((n, G), dtype=torch.float64, device=x.device)
    p = torch.empty_like(stat)
    padj = torch.empty_like(stat)
    check(L.icnv_de_tests_dev(_ptr(x), G, C, ld, cp, cop, len(groups), mp, cmp.shape[0], code, int(bool(jitter)),
                              int(seed) & (2**64 - 1), _ptr(stat), _ptr(p), _ptr(padj), _stream()))
    return stat, p, padj


def mask_non_de(x, padj, p_val_thresh, base, cell_cmps, n_normal, rule="any", mask_val=None, out=None):
    """.mask_DE_genes (R/inferCNV_mask_non_DE.R:77-134) on the device (icnv_mask_non_de_dev): count(g, c) = base[c] + the
    comparisons k in cell_cmps[c] with padj[k, g] < p_val_thresh; the mask value where the rule holds.  mask_val None: the
    correctly rounded mean of x.  out: a (C, G) tensor (may be x), default a new one.  Returns (out, mask value used)."""
    L = _lib.load()
    C, G, ld = _check_matrix_ld(x)
    code = DE_RULES.get(rule, -1) if isinstance(rule, str) else int(rule)
    if out is None:
        out = torch.empty((C, G), dtype=torch.float64, device=x.device)
    Co, Go, ld_out = _check_matrix_ld(out)
    if (Co, Go) != (C, G):
        raise ValueError("out must have the shape of x")
    b, bp = i32(base)
    off = np.zeros(C + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(v) for v in cell_cmps])
    off, op = i32(off)
    idx = np.concatenate([np.asarray(v, dtype=np.int32) for v in cell_cmps]) if off[-1] else np.zeros(1, dtype=np.int32)
    idx, ip = i32(idx)
    n_cmp = padj.shape[0] if padj is not None else 0
    if padj is not None and not (padj.is_cuda and padj.dtype == torch.float64 and padj.is_contiguous() and padj.shape[-1] == G):
        raise TypeError("padj must be a contiguous (n_cmp, G) CUDA float64 tensor")
    used = ct.c_double(0.0)
    check(L.icnv_mask_non_de_dev(_ptr(x), G, C, ld, _ptr(padj), n_cmp, float(p_val_thresh), bp, op, ip, int(n_normal), code,
                                 int(mask_val is None), float("nan") if mask_val is None else float(mask_val), _ptr(out), ld_out,
                                 ct.byref(used), _stream()))
    return out, used.value


# ------------------------------------------------------------------ hidden spike-in (DESIGN K15)
def group_gene_tables(x, groups):
    """.get_mean_var_table / .get_mean_vs_p0_table (R/inferCNV_meanVarSim.R:178-211, R/inferCNV_simple_sim.R:100-154) for all
    groups in one call (icnv_group_gene_tables_dev, DESIGN K15).  x: (C, G) CUDA float64 matrix with contiguous rows; groups:
    list of non-empty 0-based cell index vectors (they may overlap).  Returns (m, v, nzero) CUDA tensors (n_groups, G): the
    correctly rounded mean, the variance (NaN for a one-cell group) and the int32 number of zeros.  Synchronises the device."""
    L = _lib.load()
    C, G, ld = _check_matrix_ld(x)
    cidx, coff = pack_groups(groups)
    cidx, cp = i32(cidx)
    coff, cop = i32(coff)
    n = max(len(groups), 1)
    m = torch.empty((n, G), dtype=torch.float64, device=x.device)
    v = torch.empty_like(m)
    nzero = torch.empty((n, G), dtype=torch.int32, device=x.device)
    check(L.icnv_group_gene_tables_dev(_ptr(x), G, C, ld, cp, cop, len(groups), _ptr(m), _ptr(v), _ptr(nzero), _stream()))
    return m, v, nzero


def hspike_simulate(means, num_cells, var_spline, p0_spline, seed, tokens, device=None):
    """.get_simulated_cell_matrix_using_meanvar_trend_helper + .apply_dropout (R/inferCNV_meanVarSim.R:23-55, 105-161) for
    several matrices in one launch (icnv_hspike_simulate_dev, DESIGN K15).  means: (n_mat, n_genes) host array, one row of
    gene means per matrix; var_spline / p0_spline: objects with knots, coef, xmin and range (smooth_spline.SmoothSpline);
    tokens: one uint64 per matrix.  Returns a (n_mat, num_cells, n_genes) CUDA float64 tensor: matrix k, cell c, gene g.
    Synchronises the device."""
    L = _lib.load()
    means, mp = f64(np.atleast_2d(np.asarray(means, dtype=np.float64)))
    n_mat, n_genes = means.shape
    tok, tp = _u64(tokens)
    if tok.size != n_mat:
        raise ValueError("one token per matrix")
    vk, vkp = f64(var_spline.knots)
    vc, vcp = f64(var_spline.coef)
    pk, pkp = f64(p0_spline.knots)
    pc, pcp = f64(p0_spline.coef)
    if vk.size != vc.size + 4 or pk.size != pc.size + 4:
        raise ValueError("a spline has nk coefficients and nk + 4 knots")
    out = torch.empty((n_mat, int(num_cells), n_genes), dtype=torch.float64, device=device if device is not None else "cuda")
    check(L.icnv_hspike_simulate_dev(mp, n_genes, int(num_cells), n_mat, vkp, vcp, vc.size, float(var_spline.xmin), float(var_spline.range),
                                     pkp, pcp, pc.size, float(p0_spline.xmin), float(p0_spline.range), int(seed) & (2**64 - 1), tp,
                                     _ptr(out), _stream()))
    return out


DE_STATS = ("calls", "comparisons", "genes", "segments_lds", "segments_hbm", "waves", "us")


def de_stats(reset=False):
    """icnv_de_stats as a dict (`us`: wall time of the test calls in microseconds); reset=True zeroes the counters."""
    return _counters("de", DE_STATS, reset)


def _bayes_offsets(regions_cells):
    off = np.zeros(len(regions_cells) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(c) for c in regions_cells])
    return off, off.ctypes.data_as(ct.POINTER(ct.c_int64))


def bayes_loglik(x, regions, mu, tau):
    """The likelihood pass of the mixture model of the predicted CNV regions (icnv_bayes_loglik_dev, DESIGN K13).  x: (C, G)
    CUDA float64 matrix with contiguous rows; regions: list of (first gene, gene count, 0-based cell index vector); mu, tau:
    the K state means and precisions.  Returns (ll, L, cell_off): CUDA float64 (rows, K) tensors -- region r's cells are the
    rows cell_off[r] .. cell_off[r + 1] - 1 -- with L = exp_lib(ll - its row maximum).  Synchronises the device."""
    L_ = _lib.load()
    C, G, ld = _check_matrix_ld(x)
    K = len(mu)
    g0, g0p = i32([r[0] for r in regions])
    ng, ngp = i32([r[1] for r in regions])
    off, offp = _bayes_offsets([r[2] for r in regions])
    cidx = (np.concatenate([np.asarray(r[2], dtype=np.int32).ravel() for r in regions]) if len(regions) else np.zeros(0, dtype=np.int32))
    cidx, cp = i32(cidx if cidx.size else np.zeros(1, dtype=np.int32))
    m, mp = f64(mu)
    t, tp = f64(tau)
    rows = int(off[-1])
    ll = torch.empty((rows, K), dtype=torch.float64, device=x.device)
    Lk = torch.empty_like(ll)
    check(L_.icnv_bayes_loglik_dev(_ptr(x), G, C, ld, g0p, ngp, cp, offp, len(regions), K, mp, tp, _ptr(ll), _ptr(Lk), _stream()))
    return ll, Lk, off


def bayes_loglik_arrays(x, gene_start, gene_count, cell_idx, cell_off, mu, tau):
    """bayes_loglik for regions that already are arrays (the table route of bayes_net, DESIGN K25): gene_start, gene_count
    (one per region), cell_idx (the concatenated cell columns) and cell_off (int64, regions + 1) go to the same C entry
    without a Python object per region.  Returns (ll, L, cell_off as the int64 array the sampler takes)."""
    L_ = _lib.load()
    C, G, ld = _check_matrix_ld(x)
    K = len(mu)
    g0, g0p = i32(gene_start)
    ng, ngp = i32(gene_count)
    off = np.ascontiguousarray(cell_off, dtype=np.int64)
    if g0.ndim != 1 or ng.shape != g0.shape or off.shape != (g0.size + 1,):
        raise ValueError("one gene_start and gene_count per region, and regions + 1 offsets")
    cidx = np.ascontiguousarray(cell_idx, dtype=np.int32).ravel()
    if off.size and int(off[-1]) != cidx.size:
        raise ValueError("cell_off does not match cell_idx")
    cidx, cp = i32(cidx if cidx.size else np.zeros(1, dtype=np.int32))
    m, mp = f64(mu)
    t, tp = f64(tau)
    rows = int(off[-1])
    ll = torch.empty((rows, K), dtype=torch.float64, device=x.device)
    Lk = torch.empty_like(ll)
    check(L_.icnv_bayes_loglik_dev(_ptr(x), G, C, ld, g0p, ngp, cp, off.ctypes.data_as(ct.POINTER(ct.c_int64)), g0.size, K, mp, tp,
                                   _ptr(ll), _ptr(Lk), _stream()))
    return ll, Lk, off


def bayes_sample(L, cell_off, tokens, n_adapt=500, n_burn=200, n_keep=1000, seed=0, want_samples=False):
    """The Gibbs sampler of every region's mixture model in one call (icnv_bayes_sample_dev, DESIGN K13): K chains per region,
    n_adapt + n_burn discarded and n_keep kept iterations.  L, cell_off: as bayes_loglik returns them; tokens: one uint64
    per region (fnv1a64 of its name).  Returns (theta_sum (R, K, K) float64: per chain the sum of its kept theta,
    theta_samples (R, K, n_keep, K) or None, freq (rows, K) int32: how often each cell was in each state over all chains).
    Synchronises the device."""
    L_ = _lib.load()
    if not (isinstance(L, torch.Tensor) and L.is_cuda and L.dtype == torch.float64 and L.dim() == 2 and L.is_contiguous()):
        raise TypeError("L must be a contiguous (rows, K) CUDA float64 tensor")
    K = L.shape[1]
    off = np.ascontiguousarray(cell_off, dtype=np.int64)
    R = off.size - 1
    if int(off[-1]) != L.shape[0]:
        raise ValueError("cell_off does not match the rows of L")
    tok, tokp = _u64(tokens)
    if tok.size != R:
        raise ValueError("one token per region")
    theta_sum = torch.empty((R, K, K), dtype=torch.float64, device=L.device)
    samples = torch.empty((R, K, int(n_keep), K), dtype=torch.float64, device=L.device) if want_samples else None
    freq = torch.empty((L.shape[0], K), dtype=torch.int32, device=L.device)
    check(L_.icnv_bayes_sample_dev(_ptr(L), off.ctypes.data_as(ct.POINTER(ct.c_int64)), tokp, R,
                                   K, int(n_adapt), int(n_burn), int(n_keep), int(seed) & (2**64 - 1), _ptr(theta_sum), _ptr(samples),
                                   _ptr(freq), _stream()))
    return theta_sum, samples, freq


BAYES_STATS = ("calls", "regions", "rows", "undecided_rows", "regions_lds", "regions_streamed", "us", "loglik_us", "regions_packed")


def bayes_stats(reset=False):
    """icnv_bayes_stats as a dict (`us` / `loglik_us`: wall microseconds of the sample / likelihood calls); reset=True zeroes it."""
    return _counters("bayes", BAYES_STATS, reset)


MCMC_CHAIN_FIELDS = ("mean", "var", "spec0", "order", "geweke", "acf1", "acf5", "acf10", "acf50")
MCMC_POOLED_FIELDS = ("mean", "sd", "q2.5", "q50", "q97.5", "psrf", "ess")


def mcmc_diag(theta_samples):
    """Convergence diagnostics of the sampler's chains (icnv_mcmc_diag_dev, DESIGN K31; the library's own contract, modelled on
    coda).  theta_samples: contiguous (regions, n_chains, n_keep, K) CUDA float64 tensor as bayes_sample(want_samples=True)
    returns it.  Returns (chain_stats (regions, K, n_chains, 9): MCMC_CHAIN_FIELDS per region, state and chain; pooled
    (regions, K, 7): MCMC_POOLED_FIELDS per region and state) as CUDA float64 tensors.  Synchronises the device."""
    L = _lib.load()
    t = theta_samples
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.dim() == 4 and t.is_contiguous()):
        raise TypeError("theta_samples must be a contiguous (regions, n_chains, n_keep, K) CUDA float64 tensor")
    R, m, n, K = (int(v) for v in t.shape)
    chain_stats = torch.empty((R, K, m, len(MCMC_CHAIN_FIELDS)), dtype=torch.float64, device=t.device)
    pooled = torch.empty((R, K, len(MCMC_POOLED_FIELDS)), dtype=torch.float64, device=t.device)
    if R:
        check(L.icnv_mcmc_diag_dev(_ptr(t), R, m, n, K, _ptr(chain_stats), _ptr(pooled), _stream()))
    return chain_stats, pooled


def mcmc_diag_host(theta_samples):
    """mcmc_diag for a host array (icnv_mcmc_diag: the library uploads the samples and downloads both results)."""
    L = _lib.load()
    t = np.ascontiguousarray(theta_samples, dtype=np.float64)
    if t.ndim != 4:
        raise TypeError("theta_samples must have the shape (regions, n_chains, n_keep, K)")
    R, m, n, K = t.shape
    chain_stats = np.empty((R, K, m, len(MCMC_CHAIN_FIELDS)))
    pooled = np.empty((R, K, len(MCMC_POOLED_FIELDS)))
    if R:
        check(L.icnv_mcmc_diag(ct.c_void_p(t.ctypes.data), R, m, n, K, ct.c_void_p(chain_stats.ctypes.data), ct.c_void_p(pooled.ctypes.data)))
    return chain_stats, pooled


def fill_regions(states, gene_first, gene_count, cell_off, cell_idx, value):
    """The rectangle rewrite of the Bayesian filter in one launch (icnv_state_fill_regions_dev, DESIGN K25), IN PLACE: states
    (C, G) uint8 CUDA tensor, rows `ld` apart; region r = the genes gene_first[r] .. + gene_count[r] - 1 of the cells
    cell_idx[cell_off[r] : cell_off[r + 1]] becomes value[r], 0 leaves it alone.  The region arrays are CUDA tensors (int32,
    int32, int64, int32, uint8) or anything numpy converts, which is uploaded.  The rectangles must be disjoint.  ValueError
    (states untouched) when an index is out of range."""
    L = _lib.load()
    C, G, ld = _check_matrix_ld(states, torch.uint8)

    def dev(a, dtype):
        if isinstance(a, torch.Tensor):
            if not (a.is_cuda and a.dtype == dtype and a.dim() == 1 and a.is_contiguous()):
                raise TypeError(f"region arrays must be contiguous one-dimensional CUDA tensors ({dtype})")
            return a
        np_dtype = {torch.int32: np.int32, torch.int64: np.int64, torch.uint8: np.uint8}[dtype]
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np_dtype).ravel()).to(states.device)

    g0, ng, off = dev(gene_first, torch.int32), dev(gene_count, torch.int32), dev(cell_off, torch.int64)
    idx, val = dev(cell_idx, torch.int32), dev(value, torch.uint8)
    n = int(g0.numel())
    if ng.numel() != n or val.numel() != n or off.numel() != n + 1:
        raise ValueError("one gene_first, gene_count and value per region, and regions + 1 offsets")
    rc = L.icnv_state_fill_regions_dev(_ptr(states), G, C, ld, n, _ptr(g0), _ptr(ng), _ptr(off), _ptr(idx) if idx.numel() else None,
                                       int(idx.numel()), _ptr(val), _stream())
    if rc == _lib.ERR_ARG:
        raise ValueError(L.icnv_last_error().decode("utf-8", "replace"))
    check(rc)
    return states


def paint_regions(out, gene_first, gene_count, cell_off, cell_idx, value):
    """postProbNormal's matrix in one call (icnv_paint_regions_dev, DESIGN K33), IN PLACE: out (C, G) float64 CUDA tensor, rows
    `ld` apart, becomes +0.0 everywhere and then value[r] over region r = the genes gene_first[r] .. + gene_count[r] - 1 of the
    cells cell_idx[cell_off[r] : cell_off[r + 1]], regions in order: where they overlap the highest r stays.  The region arrays
    are CUDA tensors (int32, int32, int64, int32, float64) or anything numpy converts, which is uploaded.  ValueError (out
    untouched) when an index is out of range."""
    L = _lib.load()
    C, G, ld = _check_matrix_ld(out)

    def dev(a, dtype):
        if isinstance(a, torch.Tensor):
            if not (a.is_cuda and a.dtype == dtype and a.dim() == 1 and a.is_contiguous()):
                raise TypeError(f"region arrays must be contiguous one-dimensional CUDA tensors ({dtype})")
            return a
        np_dtype = {torch.int32: np.int32, torch.int64: np.int64, torch.float64: np.float64}[dtype]
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np_dtype).ravel()).to(out.device)

    g0, ng, off = dev(gene_first, torch.int32), dev(gene_count, torch.int32), dev(cell_off, torch.int64)
    idx, val = dev(cell_idx, torch.int32), dev(value, torch.float64)
    n = int(g0.numel())
    if ng.numel() != n or val.numel() != n or off.numel() != n + 1:
        raise ValueError("one gene_first, gene_count and value per region, and regions + 1 offsets")
    rc = L.icnv_paint_regions_dev(_ptr(out), G, C, ld, n, _ptr(g0), _ptr(ng), _ptr(off), _ptr(idx) if idx.numel() else None,
                                  int(idx.numel()), _ptr(val), _stream())
    if rc == _lib.ERR_ARG:
        raise ValueError(L.icnv_last_error().decode("utf-8", "replace"))
    check(rc)
    return out


BOX_FIELDS = ("ymin", "lower", "middle", "upper", "ymax", "n_low", "n_high")


def theta_box(theta_samples):
    """The box statistics of every (region, state) over its pooled kept theta draws (icnv_theta_box_dev, DESIGN K33; the
    library's own contract, modelled on ggplot2's stat_boxplot).  theta_samples: contiguous (regions, n_chains, n_keep, K) CUDA
    float64 tensor as bayes_sample(want_samples=True) returns it.  Returns the (regions, K, 7) CUDA float64 tensor of
    BOX_FIELDS.  Synchronises the device."""
    L = _lib.load()
    t = theta_samples
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.dim() == 4 and t.is_contiguous()):
        raise TypeError("theta_samples must be a contiguous (regions, n_chains, n_keep, K) CUDA float64 tensor")
    R, m, n, K = (int(v) for v in t.shape)
    box = torch.empty((R, K, len(BOX_FIELDS)), dtype=torch.float64, device=t.device)
    check(L.icnv_theta_box_dev(_ptr(t) if t.numel() else _ptr(box.new_empty(1)), R, m, n, K,
                               _ptr(box) if box.numel() else _ptr(box.new_empty(1)), _stream()))
    return box


def state_consensus(states, groups, overwrite=False):
    """.get_state_consensus (R/inferCNV_HMM.R:977-987) per group -> (n_groups, G) uint8; with
    overwrite=True also returns the state matrix with every member cell set to its group's consensus."""
    L = _lib.load()
    C, G = _check_matrix(states, torch.uint8)
    idx, off = pack_groups(groups)
    idx, ip = i32(idx)
    off, op = i32(off)
    cons = torch.empty((len(groups), G), dtype=torch.uint8, device=states.device)
    out = torch.empty_like(states) if overwrite else None
    check(L.icnv_state_consensus_dev(_ptr(states), G, C, ip, op, len(groups), _ptr(cons), _ptr(out), _stream()))
    return (cons, out) if overwrite else cons


def _chr_start(chr_start, G):
    cs, cp = i32(chr_start)
    if cs.ndim != 1 or cs.size < 2 or cs[0] != 0 or cs[-1] != G:
        raise ValueError("chr_start must run from 0 to the gene count")
    return cs, cp


def cnv_features(states, chr_start, K, s0, want_run_counts=False):
    """The four integers behind add_to_seurat's per-chromosome features (icnv_cnv_features_dev; .get_features,
    R/seurat_interaction.R:244-353): states (columns, G) uint8, rows `ld` apart -> int32 (n_chr, columns, 4) tensor of n_loss,
    n_gain, d_loss, d_gain; with want_run_counts also the (columns, 2) int32 tensor of runs / non-neutral runs per column.
    ValueError when a byte is outside 1 .. K."""
    L = _lib.load()
    C, G, ld = _check_matrix_ld(states, torch.uint8)
    cs, cp = _chr_start(chr_start, G)
    counts = torch.empty((cs.size - 1, C, 4), dtype=torch.int32, device=states.device)
    runs = torch.empty((C, 2), dtype=torch.int32, device=states.device)
    rc = L.icnv_cnv_features_dev(_ptr(states), G, C, ld, cp, cs.size - 1, int(K), int(s0), _ptr(counts), _ptr(runs), _stream())
    if rc == _lib.ERR_ARG:
        raise ValueError(L.icnv_last_error().decode("utf-8", "replace"))
    check(rc)
    return (counts, runs) if want_run_counts else counts


CNV_RUN_FIELDS = ("col", "chr", "gene_first", "gene_last", "state", "ordinal")


def cnv_runs(states, chr_start, neutral=0, K=0, col_idx=None, run_counts=None):
    """Run-length segmentation of state columns into CNV regions (icnv_cnv_runs_dev; .define_cnv_gene_regions,
    R/inferCNV_HMM.R:1005-1057): one record per run whose state is not `neutral` (0: every run), ordered by (position in
    col_idx, gene) -> (records, n_runs): records an int32 (6, n) tensor in the order of CNV_RUN_FIELDS (`col` is the position
    in col_idx, `ordinal` the 1-based counter of the region name), n_runs the number of runs of every state.  run_counts:
    the (columns, 2) tensor cnv_features returned for s0 == neutral, which saves the counting pass.  K > 0 refuses bytes
    outside 1 .. K with ValueError."""
    L = _lib.load()
    C, G, ld = _check_matrix_ld(states, torch.uint8)
    cs, cp = _chr_start(chr_start, G)
    if col_idx is None:
        idx, ip, n_cols = None, None, C
    else:
        idx, ip = i32(col_idx)
        n_cols = idx.size
    have = run_counts is not None
    if not have:
        run_counts = torch.empty((C, 2), dtype=torch.int32, device=states.device)
    n_rec, n_runs = ct.c_int64(), ct.c_int64()

    def call(valid, cap, rec):
        rc = L.icnv_cnv_runs_dev(_ptr(states), G, C, ld, cp, cs.size - 1, ip, n_cols, int(K), int(neutral), _ptr(run_counts), valid,
                                 cap, _ptr(rec), ct.byref(n_rec), ct.byref(n_runs), _stream())
        if rc == _lib.ERR_ARG:
            raise ValueError(L.icnv_last_error().decode("utf-8", "replace"))
        check(rc)

    if not have:
        call(0, 0, None)                                    # the count-only call fills run_counts
    else:
        n_rec.value = int(run_counts[:, 1].sum().item()) if idx is None else int(
            run_counts[torch.as_tensor(idx.astype(np.int64), device=states.device), 1].sum().item())
    cap = n_rec.value
    rec = torch.empty((6, max(cap, 1)), dtype=torch.int32, device=states.device)
    call(1, max(cap, 1), rec)
    return rec[:, :n_rec.value], n_runs.value


def states_to_proxy(states, K):
    """assign_HMM_states_to_proxy_expr_vals (R/inferCNV_HMM.R:1191-1206) / i3 (R/inferCNV_i3HMM.R:405-417)."""
    L = _lib.load()
    _check_matrix(states, torch.uint8)
    out = torch.empty(states.shape, dtype=torch.float64, device=states.device)
    check(L.icnv_states_to_proxy_dev(_ptr(states), _ptr(out), states.numel(), int(K), _stream()))
    return out


def cells_mean_sd(x, cell_idx):
    """mean and sd over ALL values of the listed cells (R/inferCNV_i3HMM.R:17-80)."""
    L = _lib.load()
    C, G = _check_matrix(x)
    idx, ip = i32(cell_idx)
    out = (ct.c_double * 2)()
    check(L.icnv_cells_mean_sd_dev(_ptr(x), G, C, ip, idx.size, out, _stream()))
    return out[0], out[1]


# ------------------------------------------------------------------ ingest from integer counts (steps 2-4)
ERR_SPARSE_VALUES = "the sparse route wants integer counts in 0 .. 2^31 - 1; pass sparse=False for other data"   # K22's, and K34's


class DeviceCounts:
    """The raw count matrix on the device: dense int32 (C, G) tensor -- row-major (C, G) is R's column-major G x C -- or
    CSC (colptr int64 [C + 1], rowidx int32 [nnz], vals int32 [nnz]) tensors."""

    def __init__(self, G, C, dense=None, colptr=None, rowidx=None, vals=None):
        self.G, self.C = int(G), int(C)
        self.t = (dense, colptr, rowidx, vals)          # keeps the tensors alive
        if dense is not None:
            assert dense.is_cuda and dense.dtype == torch.int32 and dense.is_contiguous() and tuple(dense.shape) == (C, G)
            self.c = _lib.Counts(dense.data_ptr(), None, None, None, 0)
        else:
            assert colptr.dtype == torch.int64 and rowidx.dtype == torch.int32 and vals.dtype == torch.int32
            assert colptr.numel() == C + 1 and rowidx.numel() == vals.numel()
            self.c = _lib.Counts(None, colptr.data_ptr(), rowidx.data_ptr() if rowidx.numel() else None,
                                 vals.data_ptr() if vals.numel() else None, int(vals.numel()))

    @property
    def device(self):
        return next(t for t in self.t if t is not None).device

    @property
    def nnz(self):
        """Stored entries of the CSC form (None for the dense form)."""
        return None if self.t[0] is not None else int(self.t[3].numel())

    @classmethod
    def from_scipy(cls, m, device=None):
        """Upload a scipy sparse matrix (genes x cells, anything with tocsc) as CSC in its canonical form: tocsc(),
        sum_duplicates(), sort_indices().  The values must be integers in 0 .. 2^31 - 1, as ops.ingest_counts asks (ValueError)."""
        m = m.tocsc().copy()
        m.sum_duplicates()
        m.sort_indices()
        vals = np.ascontiguousarray(m.data)
        if not np.array_equal(vals, np.rint(vals)) or (vals.size and (vals.min() < 0 or vals.max() > 0x7fffffff)):
            raise ValueError(ERR_SPARSE_VALUES)
        G, C = m.shape
        if G < 1 or C < 1:
            raise ValueError("the matrix must have at least one gene and one cell")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        return cls(G, C, colptr=torch.from_numpy(np.ascontiguousarray(m.indptr, dtype=np.int64)).to(dev),
                   rowidx=torch.from_numpy(np.ascontiguousarray(m.indices, dtype=np.int32)).to(dev),
                   vals=torch.from_numpy(vals.astype(np.int32)).to(dev))

    def to_scipy(self, dtype=np.float64):
        """Download to a scipy.sparse.csc_matrix, genes x cells (float64 data by default, as a dgCMatrix holds).  The entries of
        a column keep their stored order."""
        from scipy.sparse import csc_matrix
        if self.t[0] is not None:
            return csc_matrix(self.t[0].cpu().numpy().T.astype(dtype))
        _, colptr, rowidx, vals = self.t
        return csc_matrix((vals.cpu().numpy().astype(dtype), rowidx.cpu().numpy(), colptr.cpu().numpy()), shape=(self.G, self.C))

    def to_dense(self):
        """The (C, G) CUDA float64 tensor of the counts, expanded on the device (icnv_ingest_apply_dev with normalise and log2
        off)."""
        L = _lib.load()
        keep = torch.arange(self.G, dtype=torch.int32, device=self.device)
        out = torch.empty((self.C, self.G), dtype=torch.float64, device=self.device)
        check(L.icnv_ingest_apply_dev(ct.byref(self.c), self.G, self.C, _ptr(keep), self.G, None, 1.0, 0, 0, _ptr(out), _stream()))
        torch.cuda.current_stream().synchronize()
        return out


def ingest_gene_stats(counts):
    """[G sums | G counts of cells with a positive count] as one float64 tensor (all-reduce it in a sharded run)."""
    L = _lib.load()
    out = torch.empty(2 * counts.G, dtype=torch.float64, device=counts.device)
    check(L.icnv_ingest_gene_stats_dev(ct.byref(counts.c), counts.G, counts.C, _ptr(out), _stream()))
    return out


def ingest_select(stats_host, G, C_total, min_mean_expr_cutoff=None, min_cells_per_gene=0):
    """Step 2's decision from the gene statistics (R/inferCNV_ops.R:2128-2213) -> kept gene indices."""
    L = _lib.load()
    st, sp = f64(stats_host)
    keep = np.empty(G, dtype=np.int32)
    n = ct.c_int64()
    check(L.icnv_ingest_select(sp, G, int(C_total), float("nan") if min_mean_expr_cutoff is None else float(min_mean_expr_cutoff),
                               int(min_cells_per_gene), keep.ctypes.data_as(ct.POINTER(ct.c_int32)), ct.byref(n)))
    return keep[:n.value].copy()


def ingest_col_sums(counts, keep_idx):
    L = _lib.load()
    mask = torch.zeros(counts.G, dtype=torch.uint8, device=counts.device)
    mask[torch.as_tensor(np.asarray(keep_idx, dtype=np.int64), device=counts.device)] = 1
    out = torch.empty(counts.C, dtype=torch.float64, device=counts.device)
    check(L.icnv_ingest_col_sums_dev(ct.byref(counts.c), counts.G, counts.C, _ptr(mask), _ptr(out), _stream()))
    torch.cuda.current_stream().synchronize()           # (the mask is released when this returns)
    return out


def ingest_apply(counts, keep_idx, col_sums, factor):
    """log2(count / colSum * factor + 1) of the kept genes -> (C, G_out) float64 tensor."""
    L = _lib.load()
    keep = torch.as_tensor(np.asarray(keep_idx, dtype=np.int32), device=counts.device)
    out = torch.empty((counts.C, int(keep.numel())), dtype=torch.float64, device=counts.device)
    check(L.icnv_ingest_apply_dev(ct.byref(counts.c), counts.G, counts.C, _ptr(keep), int(keep.numel()), _ptr(col_sums), float(factor),
                                  1, 1, _ptr(out), _stream()))
    torch.cuda.current_stream().synchronize()
    return out


def ingest_counts(counts, min_mean_expr_cutoff=None, min_cells_per_gene=0, normalize_factor=None):
    """Steps 2-4 of run() in one call on one device -> (expr (C, G_out) float64, kept gene indices, factor used)."""
    L = _lib.load()
    keep = np.empty(counts.G, dtype=np.int32)
    n, used = ct.c_int64(), ct.c_double()
    buf = torch.empty((counts.C * counts.G,), dtype=torch.float64, device=counts.device)
    check(L.icnv_ingest_counts_dev(ct.byref(counts.c), counts.G, counts.C,
                                   float("nan") if min_mean_expr_cutoff is None else float(min_mean_expr_cutoff), int(min_cells_per_gene),
                                   float("nan") if normalize_factor is None else float(normalize_factor),
                                   keep.ctypes.data_as(ct.POINTER(ct.c_int32)), ct.byref(n), _ptr(buf), ct.byref(used), _stream()))
    g_out = n.value
    return buf[: counts.C * g_out].view(counts.C, g_out), keep[:g_out].copy(), used.value


# ------------------------------------------------------------------ sparse count matrices (DESIGN K22)
READ_MTX_CHUNK = 64 << 20          # bytes of one chunk of read_mtx; ICNV_READ_MTX_CHUNK (developer switch) overrides it
_MM_FIELDS = {"integer": _lib.MM_INTEGER, "real": _lib.MM_REAL, "pattern": _lib.MM_PATTERN}


def _mtx_header(f):
    """The banner, the % comment lines and the size line of a MatrixMarket file open for reading bytes: (field code, G, C,
    nnz, lines read, bytes read).  Only `%%MatrixMarket matrix coordinate {integer|real|pattern} general` is accepted."""
    line = f.readline()
    n_lines, n_bytes = 1, len(line)
    toks = line.decode("latin-1").split()
    if not toks or toks[0].lower() != "%%matrixmarket":
        raise ValueError("read_mtx: the banner line must start with %%MatrixMarket")
    if len(toks) != 5:
        raise ValueError(f"read_mtx: the banner has {len(toks)} fields, 5 are expected")
    obj, fmt, field, symmetry = (t.lower() for t in toks[1:])
    if obj != "matrix":
        raise ValueError(f"read_mtx: banner object '{toks[1]}': only 'matrix' is read")
    if fmt != "coordinate":
        raise ValueError(f"read_mtx: banner format '{toks[2]}': only 'coordinate' is read")
    if field not in _MM_FIELDS:
        raise ValueError(f"read_mtx: banner field '{toks[3]}': only 'integer', 'real' and 'pattern' are read")
    if symmetry != "general":
        raise ValueError(f"read_mtx: banner symmetry '{toks[4]}': only 'general' is read")
    while True:
        line = f.readline()
        if not line:
            raise ValueError("read_mtx: the size line is missing")
        n_lines, n_bytes = n_lines + 1, n_bytes + len(line)
        if line.startswith(b"%") or not line.strip():
            continue
        toks = line.split()
        if len(toks) != 3 or not all(t.isdigit() and len(t) <= 18 for t in toks):
            raise ValueError(f"read_mtx: size line '{line.decode('latin-1').strip()}': three integers G C nnz are expected")
        G, C, nnz = (int(t) for t in toks)
        if not (1 <= G <= 0x7fffffff and 1 <= C <= 0x7fffffff):
            raise ValueError("read_mtx: size line: G and C must be 1 .. 2147483647")
        if nnz > G * C:
            raise ValueError(f"read_mtx: size line: {nnz} entries do not fit a {G} x {C} matrix")
        return _MM_FIELDS[field], G, C, nnz, n_lines, n_bytes


def _triplet_slots(row, col, val, offset):
    """The argument checks the triplet entries share: (the addresses of slot `offset` of row / col / val, the slots from there
    on)."""
    offset = int(offset)
    for t in (row, col, val):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.dim() == 1 and t.is_contiguous()
                and t.numel() == row.numel()):
            raise TypeError("row, col and val must be contiguous CUDA int32 vectors of one length")
    if offset < 0 or offset > row.numel():
        raise ValueError("offset must be 0 .. the length of the arrays")
    capacity = row.numel() - offset
    at = [ct.c_void_p(t.data_ptr() + 4 * offset) if capacity else ct.c_void_p(0) for t in (row, col, val)]
    return at, capacity


def parse_triplets_into(text_dev, text_host, n_bytes, field, G, C, row, col, val, offset, line0=1, col_map=None, n_cols_out=None):
    """icnv_parse_triplets_dev: the first n_bytes of `text_dev` (contiguous CUDA uint8) and of `text_host` (uint8 numpy array
    with the same bytes) are whole lines of the body of a coordinate file of a G x C matrix; entry k of them goes to slot
    offset + k of row / col / val (CUDA int32 of one length).  Returns the entries found.  On an IcnvError the arrays are as they
    were.  Synchronises the stream.
    With col_map and n_cols_out (parse_triplets_cols_into), icnv_parse_triplets_cols_dev: returns (kept, seen)."""
    L = _lib.load()
    if col_map is not None and not (isinstance(col_map, torch.Tensor) and col_map.is_cuda and col_map.dtype == torch.int32 and col_map.dim() == 1
                                    and col_map.is_contiguous() and col_map.numel() == int(C)):
        raise TypeError("col_map must be a contiguous CUDA int32 vector with one entry per column of the matrix")
    if col_map is not None and n_cols_out is None:
        raise TypeError("n_cols_out must be given with col_map")
    host = _check_text(text_dev, text_host, n_bytes)
    at, capacity = _triplet_slots(row, col, val, offset)
    n, seen = ct.c_int64(0), ct.c_int64(0)
    args = (_ptr(text_dev), _host_text_ptr(host), int(n_bytes), int(field), int(G), int(C), int(line0), at[0], at[1], at[2], capacity, ct.byref(n))
    if col_map is None:
        check(L.icnv_parse_triplets_dev(*args, _stream()))
        return int(n.value)
    check(L.icnv_parse_triplets_cols_dev(*args, _ptr(col_map), int(n_cols_out), ct.byref(seen), _stream()))
    return int(n.value), int(seen.value)


def parse_triplets_cols_into(text_dev, text_host, n_bytes, field, G, C, row, col, val, offset, col_map, n_cols_out, line0=1):
    """icnv_parse_triplets_cols_dev (DESIGN K26): parse_triplets_into for the columns a map selects.  col_map: a contiguous CUDA
    int32 vector of C entries, the new column (0 .. n_cols_out - 1) of each matrix column or -1.  Every entry of the chunk is validated; the kept ones
    go, in file order and with their new column, to the slots from `offset` on.  Returns (kept, seen).  When the arrays are
    too short for the kept entries the IcnvError's text holds their number ("N entries are kept")."""
    if col_map is None:
        raise TypeError("col_map must be a contiguous CUDA int32 vector with one entry per column of the matrix")
    return parse_triplets_into(text_dev, text_host, n_bytes, field, G, C, row, col, val, offset, line0=line0, col_map=col_map,
                               n_cols_out=n_cols_out)


def csc_from_sorted_triplets(row, col, G, C):
    """icnv_csc_from_sorted_triplets_dev: (colptr, -1, CSC_SORTED) for triplets in strictly ascending (col, row) order -- row
    and the values are then the CSC's arrays as they are --, or (None, k, CSC_DUPLICATE | CSC_DESCENT) with k the first entry
    whose key does not exceed its predecessor's."""
    L = _lib.load()
    nnz = int(row.numel())
    colptr = torch.empty(int(C) + 1, dtype=torch.int64, device=row.device)
    first, kind = ct.c_int64(-1), ct.c_int32(0)
    check(L.icnv_csc_from_sorted_triplets_dev(_ptr(row) if nnz else None, _ptr(col) if nnz else None, nnz, int(G), int(C), _ptr(colptr),
                                              ct.byref(first), ct.byref(kind), _stream()))
    return (colptr if kind.value == _lib.CSC_SORTED else None), int(first.value), int(kind.value)


def _count_entries(path, skip_bytes):
    """The lines after the first skip_bytes of the (decompressed) file that are not blank: the error path of read_mtx."""
    count = 0
    with _open_text(path) as f:
        f.read(skip_bytes)
        for line in f:
            count += bool(line.strip(b" \t\r\n"))
    return count


def _mtx_result(row, col, val, filled, seen, nnz, G, C, sel, offset, stats, t_start):
    """read_mtx behind its chunk loop: the entry count against the size line, the CSC arrays, the sort where it is needed."""
    import time
    if sel is None:
        seen = filled
    if seen != nnz:
        raise ValueError(f"read_mtx: the size line says {nnz} entries, the body has {seen}")
    stats["bytes"], stats["entries"] = offset, seen
    if sel is not None:
        stats["entries_kept"] = filled
        row, col, val = (t[:filled].clone() if t.numel() > filled else t for t in (row, col, val))
        C = int(sel.size)
    colptr, first, kind = csc_from_sorted_triplets(row, col, G, C)
    if kind == _lib.CSC_DESCENT:
        key, perm = torch.sort(col.to(torch.int64) * G + row)
        del key
        row, col, val = row[perm], col[perm], val[perm]
        del perm
        stats["sorted_on_device"] = 1
        colptr, first, kind = csc_from_sorted_triplets(row, col, G, C)
        if kind == _lib.CSC_DESCENT:
            raise RuntimeError("read_mtx: the sorted triplets are not in order (internal error)")
    if kind == _lib.CSC_DUPLICATE:
        column = int(col[first]) if sel is None else int(sel[int(col[first])])         # the file's column
        raise ValueError(f"duplicate entry for row {int(row[first]) + 1}, column {column + 1}")
    del col
    counts = DeviceCounts(G, C, colptr=colptr, rowidx=row, vals=val)
    torch.cuda.synchronize()
    stats["wall_s"] = time.perf_counter() - t_start
    return counts, stats


def read_mtx(path, chunk_bytes=None, cells=None):
    """A MatrixMarket coordinate file (10x: matrix.mtx, or .gz) to a CSC DeviceCounts, parsed on the device
    (icnv_parse_triplets_dev, icnv_csc_from_sorted_triplets_dev; DESIGN K22; the grammar and what is refused: include/icnv.h
    "sparse count matrices").  Returns (DeviceCounts, stats).

    The banner, the % comment lines and the size line `G C nnz` are read here; only `%%MatrixMarket matrix coordinate
    {integer|real|pattern} general` is accepted (ValueError names the banner field otherwise).  The body is streamed in chunks
    of whole lines through two pinned buffers and a device buffer while a thread (text_stream.LineChunks) reads ahead.  A .gz path is first offered to
    gunzip.gunzip (DESIGN K30): a one-member gzip file of at least gunzip.GUNZIP_MIN_BYTES is inflated on the device, its header
    lines are fetched, and the body goes to the same parse entries in chunks of whole lines that are views or device-to-device
    copies of the inflated tensor -- it does not cross PCIe (a chunk's last newline is looked for in 64 KiB pieces; a refused
    chunk is fetched for the refusal's text).  stats["source"] is then "device_gunzip"; any other .gz -- stats["source"] "host",
    stats["source_reason"] why -- goes through Python's gzip.  Both routes return the same values and the same refusals.
    The triplet arrays are allocated once from the size line, every chunk parses into its offset, and an entry count other than
    the size line's is a ValueError with both numbers.  A refused byte raises IcnvError with the file line and the field.

    A file in column-major order (what 10x and scipy.io.mmwrite of a CSC matrix write) needs no sort: its rows and values are
    the CSC's arrays as parsed.  Any other order is sorted by the 64-bit key col * G + row with torch.sort and gathered --
    PyTorch as plumbing on the cold path; there is no hand-written device sort --, stats["sorted_on_device"] = 1.  A (row,
    column) pair stored twice raises ValueError("duplicate entry for row R, column C"), 1-based.

    stats: bytes (of the body), chunks, entries, sorted_on_device, read_s / parse_s / stall_s / wall_s.

    cells (DESIGN K26): a list of 0-based matrix columns, in any order, without repeats (ValueError before the file is opened
    for an empty list, a repeat or a negative entry; once the size line is read for an entry that is no column, with the entry
    and the count).  The result is the G x len(cells) DeviceCounts whose column k is file column cells[k], through
    icnv_parse_triplets_cols_dev: every entry of the file is still validated, and a refusal in a column that is not selected
    reads as it does without `cells`.  The triplet arrays hold the kept entries only; they GROW: they start at the selection's
    share of the size line's count (plus an eighth) and, when a chunk keeps more than is left, are reallocated to twice the
    need and the chunk is parsed again.  The entry count that must equal the size line's is the number of entries seen;
    stats["entries"] is that number, stats["entries_kept"] the entries of the result and stats["arrays_grown"] the reallocations.  A selection that is ascending keeps
    a column-major file sorted; any other one goes through the torch.sort path."""
    import io
    import re
    import time
    path = os.fspath(path)
    sel = None if cells is None else _selected_columns(cells, "read_mtx")
    cap0 = max(64, int(chunk_bytes if chunk_bytes is not None else os.environ.get("ICNV_READ_MTX_CHUNK", READ_MTX_CHUNK)))
    dev = torch.device("cuda", torch.cuda.current_device())
    stats = {"bytes": 0, "chunks": 0, "entries": 0, "sorted_on_device": 0, "read_s": 0.0, "parse_s": 0.0, "stall_s": 0.0}
    t_start = time.perf_counter()
    text = _gunzip_text(path, stats)
    if text is not None:                                           # K30: the header lines are fetched, growing the window if need be
        window = 1 << 16
        while True:
            f = io.BytesIO(text[:window].cpu().numpy().tobytes())
            whole = window >= text.numel()
            try:
                header = _mtx_header(f)
                if whole or header[5] < window:
                    break
            except ValueError:
                if whole:
                    raise
            window *= 2
        field, G, C, nnz, header_lines, header_bytes = header
    else:
        f = _open_text(path)
        try:
            field, G, C, nnz, header_lines, header_bytes = _mtx_header(f)
        except BaseException:
            f.close()
            raise
    col_map, seen = None, 0                                        # K26: the device map of the selection; entries seen
    try:
        if sel is not None:
            col_map = _column_map(sel, C, "read_mtx", dev)
            stats["arrays_grown"] = 0
    except BaseException:
        f.close()
        raise
    first_capacity = nnz if sel is None else min(nnz, nnz * sel.size // C + nnz // 8 + 1024)
    row, col, val = (torch.empty(first_capacity, dtype=torch.int32, device=dev) for _ in range(3))
    dbuf, offset, filled = None, 0, 0                              # bytes of the body before this chunk; entries so far

    def parse_selected(text, host, n, line0=1):
        """One chunk through the column-selected entry, the arrays grown when they are too short for what it keeps."""
        nonlocal row, col, val
        while True:
            try:
                return parse_triplets_cols_into(text, host, n, field, G, C, row, col, val, filled, col_map, sel.size, line0=line0)
            except _lib.IcnvError as exc:
                need = re.search(r"parse_triplets_cols: (\d+) entries are kept", str(exc))
                if exc.code != _lib.ERR_ARG or need is None:
                    raise
                grown = [torch.empty(2 * (filled + int(need.group(1))), dtype=torch.int32, device=dev) for _ in range(3)]
                for new, old in zip(grown, (row, col, val)):
                    new[:filled].copy_(old[:filled])
                row, col, val = grown
                stats["arrays_grown"] += 1

    def consume(chunk, host, n):
        """One chunk of whole lines (on the device; host: the same bytes, or None) into the triplet arrays."""
        nonlocal filled, seen
        try:
            if sel is None:
                filled += parse_triplets_into(chunk, host, n, field, G, C, row, col, val, filled)
            else:
                kept, in_chunk = parse_selected(chunk, host, n)
                filled, seen = filled + kept, seen + in_chunk
        except _lib.IcnvError as exc:
            if exc.code != _lib.ERR_ARG or not ("capacity" in str(exc) or "line " in str(exc)):
                raise
            if "capacity" in str(exc):
                raise ValueError(f"read_mtx: the size line says {nnz} entries, the body has "
                                 f"{_count_entries(path, header_bytes)}") from None
            line0 = 1 + _count_newlines(path, header_bytes + offset)      # the refusal again, with the file's line number
            if sel is None:
                parse_triplets_into(chunk, host, n, field, G, C, row, col, val, filled, line0=line0)
            else:
                parse_selected(chunk, host, n, line0=line0)
            raise

    if text is not None:                                           # K30: the body stays on the device
        stage = None
        try:
            for a, b in _dev_line_chunks(text, header_bytes, cap0, stats):
                t0 = time.perf_counter()
                chunk, stage = _dev_aligned(text, a, b, stage)
                offset = a - header_bytes
                consume(chunk, None, b - a)
                stats["parse_s"] += time.perf_counter() - t0
                stats["chunks"] += 1
            offset = int(text.numel()) - header_bytes
        finally:
            f.close()
        del text, stage
        return _mtx_result(row, col, val, filled, seen, nnz, G, C, sel, offset, stats, t_start)
    with f, LineChunks(f, cap0, stats) as chunks:
        try:
            job = chunks.get()
            while job is not None:
                slot, buf, n = job
                if n > 0:
                    if dbuf is None or dbuf.numel() < n:
                        dbuf = torch.empty(max(cap0, n), dtype=torch.uint8, device=dev)
                    t0 = time.perf_counter()
                    dbuf[:n].copy_(buf[:n], non_blocking=True)
                    consume(dbuf, buf.numpy()[:n], n)
                    stats["parse_s"] += time.perf_counter() - t0
                    stats["chunks"] += 1
                offset += n
                chunks.release(slot)
                t0 = time.perf_counter()
                job = chunks.get()
                stats["stall_s"] += time.perf_counter() - t0
        finally:
            torch.cuda.synchronize()                               # the last copy may still read a pinned buffer
    return _mtx_result(row, col, val, filled, seen, nnz, G, C, sel, offset, stats, t_start)


def csc_select(counts, genes, cells):
    """.order_reduce and the cell filter on a CSC DeviceCounts (icnv_csc_select_dev): the rows `genes` (0-based, in their new
    order, no repeats) and the columns `cells` (0-based, any order, repeats allowed) as a new CSC DeviceCounts.  The entries
    of an output column keep the order they have in the source column."""
    L = _lib.load()
    if counts.t[0] is not None:
        raise ValueError("csc_select wants the counts in CSC form")
    genes = np.asarray(genes, dtype=np.int64).ravel()
    cells = np.ascontiguousarray(np.asarray(cells, dtype=np.int64).ravel())
    if genes.size < 1 or genes.min() < 0 or genes.max() >= counts.G:
        raise ValueError("genes must list at least one row of the matrix, and only rows of it")
    if cells.size < 1 or cells.min() < 0 or cells.max() >= counts.C:
        raise ValueError("cells must list at least one column of the matrix, and only columns of it")
    gene_map = np.full(counts.G, -1, dtype=np.int32)
    gene_map[genes] = np.arange(genes.size, dtype=np.int32)
    if np.count_nonzero(gene_map >= 0) != genes.size:
        raise ValueError("genes lists a row twice")
    dev = counts.device
    gm, cl = torch.from_numpy(gene_map).to(dev), torch.from_numpy(cells.astype(np.int32)).to(dev)
    colptr = torch.empty(cells.size + 1, dtype=torch.int64, device=dev)
    nnz = ct.c_int64(0)
    check(L.icnv_csc_select_dev(ct.byref(counts.c), counts.G, counts.C, _ptr(gm), int(genes.size), _ptr(cl), int(cells.size), _ptr(colptr),
                                None, None, 0, ct.byref(nnz), _stream()))
    rowidx = torch.empty(nnz.value, dtype=torch.int32, device=dev)
    vals = torch.empty(nnz.value, dtype=torch.int32, device=dev)
    if nnz.value:
        check(L.icnv_csc_select_dev(ct.byref(counts.c), counts.G, counts.C, _ptr(gm), int(genes.size), _ptr(cl), int(cells.size),
                                    _ptr(colptr), _ptr(rowidx), _ptr(vals), nnz.value, ct.byref(nnz), _stream()))
    return DeviceCounts(int(genes.size), int(cells.size), colptr=colptr, rowidx=rowidx, vals=vals)


# ------------------------------------------------------------------ count matrices out of R's serialisation (DESIGN K34)
RDS_COUNTS_STATS = ("columns_calls", "columns", "elements", "check_calls", "entries_checked", "checks_refused", "fill_calls",
                    "entries_written")
RDS_KINDS = {"real": _lib.RDS_REAL, "int": _lib.RDS_INT}               # ICNV_RDS_* of include/icnv.h
READ_RDS_CHUNK = 64 << 20          # bytes of one uploaded chunk of read_rds_counts
_RDS_CSC_WHAT = {_lib.RDS_P_FIRST: "p does not start with 0", _lib.RDS_P_DESCENT: "p decreases", _lib.RDS_P_LAST: "the last entry of p is not the length of x",
                 _lib.RDS_ROW_RANGE: "a row index in i is no row of the matrix", _lib.RDS_ROW_ORDER: "the row indices of a column do not strictly increase (an entry stored twice?)"}


def rds_counts_stats(reset=False):
    """The counters of icnv_rds_counts_stats since the last reset, as a dict keyed by RDS_COUNTS_STATS."""
    return _counters("rds_counts", RDS_COUNTS_STATS, reset)


def _dev_list(a, dtype, dev):
    return a.to(device=dev, dtype=dtype).contiguous() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype={torch.int64: np.int64, torch.int32: np.int32}[dtype])).to(dev)


def rds_columns(stream, col_off, col_kind, rows, *, out=None):
    """icnv_rds_columns_dev: output row j is the `rows` big-endian elements of kind col_kind[j] (RDS_KINDS' values) that start at
    byte col_off[j] of the CUDA uint8 vector `stream`, as doubles.  stream may be a view at any address; the offsets need no
    alignment.  out: a CUDA float64 matrix (n_out, >= rows) with contiguous rows -- a view with a larger leading dimension is
    fine, its padding is not written -- or None for a new (n_out, rows) tensor."""
    L = _lib.load()
    _bytes_vector(stream, "stream")
    dev = stream.device
    off, kind = _dev_list(col_off, torch.int64, dev), _dev_list(col_kind, torch.int32, dev)
    n_out = int(off.numel())
    if kind.numel() != n_out:
        raise ValueError("col_off and col_kind list the same columns")
    if out is None:
        out = torch.empty((n_out, int(rows)), dtype=torch.float64, device=dev)
    if not (out.is_cuda and out.dtype == torch.float64 and out.dim() == 2 and out.shape[0] == n_out and out.shape[1] >= rows and
            (out.stride(1) == 1 or out.shape[1] == 1)):
        raise ValueError("out must be a CUDA float64 matrix (n_out, >= rows) with contiguous rows")
    ld = int(out.stride(0)) if n_out > 1 else max(int(out.stride(0)), int(rows))
    check(L.icnv_rds_columns_dev(_ptr(stream), int(stream.numel()), _ptr(off), _ptr(kind), n_out, int(rows), _ptr(out), ld, _stream()))
    torch.cuda.current_stream().synchronize()                       # (the lists are released when this returns)
    return out


def rds_csc_check(stream, i_off, p_off, x_off, G, C, nnz, cells=None, *, colptr=None):
    """icnv_rds_csc_check_dev on the CUDA uint8 vector `stream`: ((code, file column, index), colptr, nnz_out).  code is
    _lib.RDS_OK -- colptr (CUDA int64 [n_out + 1], allocated unless passed) then holds the selected columns' pointer and nnz_out
    their entries -- or the violation with the smallest index; colptr is then untouched and nnz_out None."""
    L = _lib.load()
    _bytes_vector(stream, "stream")
    dev = stream.device
    cl = None if cells is None else _dev_list(cells, torch.int32, dev)
    n_out = int(C) if cl is None else int(cl.numel())
    if colptr is None:
        colptr = torch.empty(n_out + 1, dtype=torch.int64, device=dev)
    if not (_is_vector(colptr, torch.int64) and colptr.numel() == n_out + 1):
        raise ValueError("colptr must be a CUDA int64 vector of n_out + 1 entries")
    status, nnz_out = (ct.c_int64 * 3)(), ct.c_int64(0)
    check(L.icnv_rds_csc_check_dev(_ptr(stream), int(stream.numel()), int(i_off), int(p_off), int(x_off), int(G), int(C), int(nnz),
                                   None if cl is None else _ptr(cl), n_out, _ptr(colptr), status, ct.byref(nnz_out), _stream()))
    st = (int(status[0]), int(status[1]), int(status[2]))
    return st, colptr, (int(nnz_out.value) if st[0] == _lib.RDS_OK else None)


def rds_csc_fill(stream, i_off, p_off, x_off, G, C, nnz, colptr, out_nnz, cells=None, *, rowidx=None, vals=None):
    """icnv_rds_csc_fill_dev after a check that found no violation, with its colptr and nnz_out: (rowidx, vals), CUDA int32."""
    L = _lib.load()
    _bytes_vector(stream, "stream")
    dev = stream.device
    cl = None if cells is None else _dev_list(cells, torch.int32, dev)
    n_out = int(C) if cl is None else int(cl.numel())
    rowidx = torch.empty(int(out_nnz), dtype=torch.int32, device=dev) if rowidx is None else rowidx
    vals = torch.empty(int(out_nnz), dtype=torch.int32, device=dev) if vals is None else vals
    for t in (rowidx, vals):
        if not (_is_vector(t, torch.int32) and t.numel() >= out_nnz):
            raise ValueError("rowidx and vals must be CUDA int32 vectors of out_nnz entries")
    check(L.icnv_rds_csc_fill_dev(_ptr(stream), int(stream.numel()), int(i_off), int(p_off), int(x_off), int(G), int(C), int(nnz),
                                  None if cl is None else _ptr(cl), n_out, _ptr(colptr), _ptr(rowidx) if out_nnz else None,
                                  _ptr(vals) if out_nnz else None, int(out_nnz), _stream()))
    return rowidx, vals


def _upload_ranges(buf, ranges, pin, dev, stats, at=None, size=None):
    """The byte ranges [(start, end)] of the host buffer `buf` as one CUDA uint8 vector, through the two pinned buffers `pin`
    (K21's pattern): a range larger than a buffer goes up in pieces.  The ranges lie back to back, or, with `at` and `size`,
    range k at byte at[k] of a vector of `size` bytes whose other bytes are left as allocated.  Returns (tensor, offset of
    every range)."""
    src = np.frombuffer(buf, dtype=np.uint8)
    total = sum(e - s for s, e in ranges)
    if at is None:
        at, size = (np.cumsum([0] + [e - s for s, e in ranges])[:-1]).tolist(), total
    out = torch.empty(max(size, 1), dtype=torch.uint8, device=dev)
    cap, events, k = int(pin[0].numel()), [None, None], 0
    for (s, e), d in zip(ranges, at):
        while s < e:
            slot, n = k % 2, min(cap, e - s)
            if events[slot] is not None:
                events[slot].synchronize()                             # the copy out of this pinned buffer has finished
            pin[slot].numpy()[:n] = src[s:s + n]
            out[d:d + n].copy_(pin[slot][:n], non_blocking=True)
            events[slot] = torch.cuda.Event()
            events[slot].record()
            s, d, k = s + n, d + n, k + 1
    torch.cuda.synchronize()
    del src                                                            # (no view of the buffer outlives the call: a mapping can be closed)
    stats["uploaded_bytes"] += total
    stats["chunks"] += k
    return out[:size], list(at)


def _upload_csc(buf, loc, sel, pin, dev, stats):
    """A host-side dgCMatrix on the device as [i | p | x]: (tensor, i_off, p_off, x_off).  Without a selection the three payloads
    whole; with one, p whole and only the entry ranges of the selected columns, each at its own place -- the bytes between them
    are never written and never read, because the kernels look at no entry of a column that is not selected.  Which bytes those
    are is read off p here, clamped exactly as the kernels clamp it (this plans the upload and decides nothing: p is validated
    on the device, and every value of the result is decoded there)."""
    i, p, x = loc.payloads
    i_off, p_off, x_off = 0, i.nbytes, i.nbytes + p.nbytes
    size = x_off + x.nbytes
    if sel is None:
        return (_upload_ranges(buf, [(q.offset, q.offset + q.nbytes) for q in (i, p, x)], pin, dev, stats)[0], i_off, p_off, x_off)
    pv = np.clip(np.frombuffer(buf, dtype=">i4", count=loc.C + 1, offset=p.offset).astype(np.int64), 0, loc.nnz)
    lo, hi = pv[sel], np.maximum(pv[sel + 1], pv[sel])
    runs = []
    for k in np.argsort(lo, kind="stable"):                            # the selected columns' entry ranges, adjoining ones merged
        if hi[k] > lo[k]:
            if runs and lo[k] <= runs[-1][1]:
                runs[-1][1] = max(runs[-1][1], int(hi[k]))
            else:
                runs.append([int(lo[k]), int(hi[k])])
    ranges = [(i.offset + 4 * a, i.offset + 4 * b) for a, b in runs] + [(p.offset, p.offset + p.nbytes)] + [(x.offset + 8 * a, x.offset + 8 * b) for a, b in runs]
    at = [i_off + 4 * a for a, _ in runs] + [p_off] + [x_off + 8 * a for a, _ in runs]
    return _upload_ranges(buf, ranges, pin, dev, stats, at=at, size=size)[0], i_off, p_off, x_off


def read_rds_counts(path, *, cells=None, chunk_bytes=None, gene_names=None, cell_names=None, opened=None):
    """The count matrix readRDS(path) hands CreateInfercnvObject (R/inferCNV.R:151-162), decoded on the device from the
    serialised stream (DESIGN K34): a numeric or integer matrix, a data.frame of numeric / integer columns, or a dgCMatrix;
    .rds, or an .rda / .RData container with exactly one such variable (rds.locate_counts says what is accepted and what each
    refusal names).  Returns (gene names, ALL cell names, x, stats), the shape of read_table's result:
        dense kinds   x is the (len(cells) or C, G) CUDA float64 tensor, as from read_table (icnv_rds_columns_dev: REALSXP bytes
                      reversed and nothing else, so NA_real_ and every NaN payload survive; INTSXP converted exactly, NA_integer_
                      becoming NA_real_)
        dgCMatrix     x is the G x (len(cells) or C) CSC DeviceCounts, as from read_mtx (icnv_rds_csc_check_dev, then
                      icnv_rds_csc_fill_dev).  The file is untrusted: p, and every entry of the selected columns, is validated
                      on the device, and a violation raises ValueError with the rule, the column and the entry (1-based); a
                      value that is no integer in 0 .. 2^31 - 1 raises K22's message (ERR_SPARSE_VALUES).
    The slot order of a dgCMatrix is the Matrix package's documented one, as rds.py writes it; no R-written dgCMatrix was
    available where this was built, so that layout is believed, not verified.

    Opening: an uncompressed file is mapped; a gzip file is offered to rds._open_on_device (K29, then K30) and the payloads are
    then consumed device to device from the inflated tensor, at their byte offsets, without a staging copy; gzip turned away
    there, and bzip2 / xz, are inflated by Python.  A host-side stream goes up through two pinned buffers in pieces of at most
    chunk_bytes (READ_RDS_CHUNK): for the dense kinds chunks of whole requested columns, each converted as it arrives; for a
    dgCMatrix p and the ranges of i and x that hold the requested columns' entries (they go, each at its place, into one device
    buffer of 12 bytes per entry of the file, which the check and the fill read: the transfer is chunked and selective, the
    buffer is whole).  Only requested columns are uploaded.  The decode is always on the device; there is no NumPy route.
    The mapping of an uncompressed file is closed before this returns (not one passed in through `opened`).

    cells: 0-based file columns, any order, no repeats (as read_table / read_mtx).  Entries of dgCMatrix columns that are not
    selected are not examined (K26's rule); p is always validated whole.  opened: what rds.open_counts(path) returned, for a
    caller that has opened the file already (ShardedCreate reads the column count first).

    stats: kind, inflate ("none", "device_k29", "device_k30" or "host", with inflate_reason), stream_bytes, payload_bytes,
    uploaded_bytes (host to device), chunks, the counters of rds_counts_stats for this call, open_s / locate_s / decode_s /
    wall_s."""
    import time
    from . import rds
    path = os.fspath(path)
    sel = None if cells is None else _selected_columns(cells, "read_rds_counts")
    cap = max(64, int(chunk_bytes if chunk_bytes is not None else READ_RDS_CHUNK))
    dev = torch.device("cuda", torch.cuda.current_device())
    before = rds_counts_stats()
    t0 = time.perf_counter()
    buf, route, reason = rds.open_counts(path) if opened is None else opened
    t1 = time.perf_counter()
    loc = rds.locate_counts(buf, gene_names=gene_names, cell_names=cell_names)
    t2 = time.perf_counter()
    stats = {"kind": loc.kind, "inflate": route, "inflate_reason": reason, "stream_bytes": len(buf), "uploaded_bytes": 0, "chunks": 0,
             "payload_bytes": int(sum(p.nbytes for p in loc.payloads))}
    if sel is not None and int(sel.max()) >= loc.C:
        bad = int(sel[sel >= loc.C][0])
        raise ValueError(f"read_rds_counts: cells entry {bad} is not a column of the file, which has {loc.C}")
    stream = buf.tensor if isinstance(buf, rds._DeviceStream) else None
    pin = None if stream is not None else [_pinned(max(64, min(cap, stats["payload_bytes"]))) for _ in range(2)]
    G = loc.G
    if loc.kind == "dgCMatrix":
        i, p, x = loc.payloads
        if stream is None:
            stream, i_off, p_off, x_off = _upload_csc(buf, loc, sel, pin, dev, stats)
        else:
            i_off, p_off, x_off = i.offset, p.offset, x.offset
        (code, column, index), colptr, out_nnz = rds_csc_check(stream, i_off, p_off, x_off, G, loc.C, loc.nnz, sel)
        if code == _lib.RDS_VALUE:
            raise ValueError(f"{ERR_SPARSE_VALUES} (entry {index + 1} of x, column {column + 1})")
        if code != _lib.RDS_OK:
            raise ValueError(f"read_rds_counts: the dgCMatrix is not valid: {_RDS_CSC_WHAT[code]} (column {column + 1}, " +
                             (f"entry {index + 1} of p)" if code <= _lib.RDS_P_LAST else f"entry {index + 1} of i)"))
        rowidx, vals = rds_csc_fill(stream, i_off, p_off, x_off, G, loc.C, loc.nnz, colptr, out_nnz, sel)
        result = DeviceCounts(G, loc.C if sel is None else int(sel.size), colptr=colptr, rowidx=rowidx, vals=vals)
    else:
        want = np.arange(loc.C, dtype=np.int64) if sel is None else sel
        if loc.kind == "data_frame":
            off = np.array([loc.payloads[j].offset for j in want], dtype=np.int64)
            es = np.array([loc.payloads[j].elem_size for j in want], dtype=np.int64)
        else:
            es = np.full(want.size, loc.payloads[0].elem_size, dtype=np.int64)
            off = loc.payloads[0].offset + want * G * es
        kind = np.where(es == 8, _lib.RDS_REAL, _lib.RDS_INT).astype(np.int32)
        result = torch.empty((want.size, G), dtype=torch.float64, device=dev)
        if stream is not None:
            rds_columns(stream, off, kind, G, out=result)
        else:                                                          # chunks of whole requested columns, merged where they adjoin
            k0 = 0
            while k0 < want.size:
                k1, size = k0 + 1, int(G * es[k0])
                while k1 < want.size and size + int(G * es[k1]) <= cap:
                    size, k1 = size + int(G * es[k1]), k1 + 1
                ranges = []
                for k in range(k0, k1):
                    a, b = int(off[k]), int(off[k] + G * es[k])
                    if ranges and ranges[-1][1] == a:
                        ranges[-1][1] = b
                    else:
                        ranges.append([a, b])
                chunk, starts = _upload_ranges(buf, ranges, pin, dev, stats)
                rel, r = np.empty(k1 - k0, dtype=np.int64), 0           # every column's offset in the chunk
                for n, k in enumerate(range(k0, k1)):
                    while not ranges[r][0] <= off[k] < ranges[r][1]:
                        r += 1
                    rel[n] = starts[r] + int(off[k]) - ranges[r][0]
                rds_columns(chunk, rel, kind[k0:k1], G, out=result[k0:k1])
                k0 = k1
    torch.cuda.synchronize()
    if opened is None:
        rds.close_counts(buf)
    t3 = time.perf_counter()
    after = rds_counts_stats()
    stats.update({k: after[k] - before[k] for k in RDS_COUNTS_STATS})
    stats.update(open_s=t1 - t0, locate_s=t2 - t1, decode_s=t3 - t2, wall_s=t3 - t0)
    return loc.genes, loc.cells, result, stats


def cells_moments_partial(x, cell_idx, phase, mean=0.0):
    """One rank's share of the split-phase mean / sd over all values of the listed cells (icnv_cells_moments_partial_dev):
    phase 0 -> (sum of values, number of values), phase 1 -> (sum of (x - mean)^2, number of values)."""
    L = _lib.load()
    C, G = _check_matrix(x)
    idx, ip = i32(cell_idx)
    out = (ct.c_double * 3)()
    check(L.icnv_cells_moments_partial_dev(_ptr(x), G, C, ip, idx.size, int(phase), float(mean), out, _stream()))
    return out[0], out[1]


# ------------------------------------------------------------------ median filter
def median_filter(x, chr_start, tiles, window_size=7, out=None, na_aware=False, return_na_count=False):
    """apply_median_filtering (R/noise_reduction.R:43-113) on device tensors.  The plain entry does not look for NaN;
    na_aware=True takes icnv_median_filter_na_dev: an output whose window holds a NaN is R's NA_real_, every other output is
    the plain entry's bit for bit (one extra read of the matrix and one host wait for the NA count).  return_na_count=True
    (with na_aware) returns (out, number of NA elements of x)."""
    if return_na_count and not na_aware:
        raise ValueError("return_na_count needs na_aware=True: the plain entry does not look for NaN")
    L = _lib.load()
    C, G = _check_matrix(x)
    cs, cp = i32(chr_start)
    idx, off = pack_groups(tiles)
    idx, ip = i32(idx)
    off, op = i32(off)
    if out is None:
        out = torch.empty_like(x)
    if na_aware:
        n_na = ct.c_int64(0)
        check(L.icnv_median_filter_na_dev(_ptr(x), _ptr(out), G, C, cp, cs.size - 1, ip, op, len(tiles), int(window_size),
                                          ct.byref(n_na), _stream()))
        return (out, n_na.value) if return_na_count else out
    check(L.icnv_median_filter_dev(_ptr(x), _ptr(out), G, C, cp, cs.size - 1, ip, op, len(tiles), int(window_size),
                                   _stream()))
    return out


# ------------------------------------------------------------------ R's XDR stream of a matrix (DESIGN K27)
XDR_LAYOUTS = {"cols": _lib.XDR_COLS, "rows": _lib.XDR_ROWS}
_XDR_DTYPES = {torch.float64: 8, torch.int32: 4}


def _xdr_matrix(x, layout):
    """(rows, cols, ld, elem_size, layout code) of a CUDA float64 / int32 vector or matrix with contiguous rows, R's dim being
    (rows, cols): a "cols" matrix has the shape (cols, rows), a "rows" matrix (rows, cols); a vector is rows = n, cols = 1."""
    code = XDR_LAYOUTS[layout] if isinstance(layout, str) else int(layout)
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype in _XDR_DTYPES and x.dim() in (1, 2)):
        raise TypeError("expected a CUDA float64 or int32 vector or matrix")
    if x.dim() == 1:
        if x.numel() > 1 and x.stride(0) != 1:
            raise TypeError("expected a contiguous vector")
        if code != _lib.XDR_COLS:
            raise ValueError('a vector is rows = n, cols = 1 of layout "cols"')
        return int(x.numel()), 1, int(x.numel()), _XDR_DTYPES[x.dtype], code
    if (x.shape[1] > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        raise TypeError("expected a matrix with contiguous rows")
    ld = int(x.stride(0)) if x.shape[0] > 1 else int(x.shape[1])
    rows, cols = (int(x.shape[1]), int(x.shape[0])) if code == _lib.XDR_COLS else (int(x.shape[0]), int(x.shape[1]))
    return rows, cols, ld, _XDR_DTYPES[x.dtype], code


def xdr_encode(x, *, layout="cols", e0=0, e1=None, out=None):
    """The elements [e0, e1) of R's big-endian, column-major stream of a matrix (icnv_xdr_encode_dev, DESIGN K27) as a CUDA
    uint8 tensor.  x: a CUDA float64 or int32 tensor with contiguous rows -- layout "cols": shape (cols, rows) of R's
    rows x cols matrix, the (cells, genes) device matrix of genes x cells expr.data; layout "rows": shape (rows, cols); a
    one-dimensional tensor is a vector.  out: a contiguous CUDA uint8 tensor that receives the bytes from its start (default:
    a new one); the returned tensor is its first (e1 - e0) * elem_size bytes.  Does not synchronise."""
    L = _lib.load()
    rows, cols, ld, es, code = _xdr_matrix(x, layout)
    e0, e1 = int(e0), rows * cols if e1 is None else int(e1)
    nbytes = max(e1 - e0, 0) * es
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and out.dim() == 1 and out.is_contiguous()):
        raise TypeError("out must be a contiguous one-dimensional CUDA uint8 tensor")
    if out.numel() < nbytes:
        raise ValueError(f"out holds {out.numel()} bytes, the segment needs {nbytes}")
    if x.numel() == 0:
        return out[:0]
    check(L.icnv_xdr_encode_dev(_ptr(x), es, rows, cols, ld, code, e0, e1, _ptr(out), _stream()))
    return out[:nbytes]


def xdr_decode(src, out, *, layout="cols", e0=0, e1=None):
    """The inverse (icnv_xdr_decode_dev): src, a contiguous CUDA uint8 tensor holding the elements [e0, e1) of the stream
    from its start, into the matrix `out` (as x of xdr_encode; only the segment's elements are written).  Returns out.  Does
    not synchronise."""
    L = _lib.load()
    rows, cols, ld, es, code = _xdr_matrix(out, layout)
    e0, e1 = int(e0), rows * cols if e1 is None else int(e1)
    if not (isinstance(src, torch.Tensor) and src.is_cuda and src.dtype == torch.uint8 and src.dim() == 1 and src.is_contiguous()):
        raise TypeError("src must be a contiguous one-dimensional CUDA uint8 tensor")
    if src.numel() < max(e1 - e0, 0) * es:
        raise ValueError(f"src holds {src.numel()} bytes, the segment needs {max(e1 - e0, 0) * es}")
    if out.numel() == 0:
        return out
    check(L.icnv_xdr_decode_dev(_ptr(src), es, rows, cols, ld, code, e0, e1, _ptr(out), _stream()))
    return out


# ------------------------------------------------------------------ DEFLATE in independent pieces (DESIGN K28)
DEFLATE_PIECE = 16384                                  # the default piece_bytes
DEFLATE_PIECE_MIN, DEFLATE_PIECE_MAX = 256, 16384      # the range icnv_deflate_pieces_dev takes
_CRC_POLY = 0xEDB88320


def deflate_bound(piece_bytes):
    """icnv_deflate_bound: the most bytes one compressed piece takes (the piece stored: 5 bytes of header per 65 535)."""
    piece_bytes = int(piece_bytes)
    if not DEFLATE_PIECE_MIN <= piece_bytes <= DEFLATE_PIECE_MAX:
        raise ValueError(f"piece_bytes must lie in [{DEFLATE_PIECE_MIN}, {DEFLATE_PIECE_MAX}]")
    return piece_bytes + 5 * ((piece_bytes + 65534) // 65535)


def _is_bytes_tensor(t, dim):
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == dim


def deflate_pieces(src, piece_bytes=DEFLATE_PIECE, *, dst=None):
    """icnv_deflate_pieces_dev (DESIGN K28): the contiguous CUDA uint8 vector src as independent DEFLATE pieces of piece_bytes
    of input each.  Returns (dst, piece_len, piece_crc): dst a (pieces, >= deflate_bound) CUDA uint8 tensor with piece i at the
    start of row i (dst=: a caller's tensor of that shape, rows of contiguous bytes at any row stride), piece_len int32, and
    piece_crc the CRC-32 of every piece's input as int32 bit patterns (`.cpu().numpy().view(np.uint32)`).  Does not
    synchronise."""
    L = _lib.load()
    bound = deflate_bound(piece_bytes)
    if not (_is_bytes_tensor(src, 1) and (src.numel() <= 1 or src.stride(0) == 1)):
        raise TypeError("src must be a contiguous one-dimensional CUDA uint8 tensor")
    n = int(src.numel())
    n_pieces = -(-n // int(piece_bytes))
    if dst is None:
        dst = torch.empty((n_pieces, bound), dtype=torch.uint8, device=src.device)
    if not (_is_bytes_tensor(dst, 2) and dst.shape[0] >= n_pieces and dst.shape[1] >= bound and (dst.shape[1] <= 1 or dst.stride(1) == 1)
            and (dst.shape[0] <= 1 or dst.stride(0) >= dst.shape[1])):
        raise TypeError(f"dst must be a CUDA uint8 tensor of at least ({n_pieces}, {bound}) with contiguous rows")
    stride = int(dst.stride(0)) if dst.shape[0] > 1 else int(dst.shape[1])
    piece_len = torch.empty(n_pieces, dtype=torch.int32, device=src.device)
    piece_crc = torch.empty(n_pieces, dtype=torch.int32, device=src.device)
    if n:
        check(L.icnv_deflate_pieces_dev(_ptr(src), n, int(piece_bytes), _ptr(dst), stride, _ptr(piece_len), _ptr(piece_crc), _stream()))
    return dst[:n_pieces], piece_len, piece_crc


def deflate_pack(dst, piece_len, *, out=None, out_cap=None):
    """icnv_deflate_pack_dev: the pieces of deflate_pieces one behind the other.  out: a contiguous CUDA uint8 vector that
    receives them from its start (default: a new one that holds the worst case); out_cap: the bytes of it that may be written
    (default: all).  Returns out[:packed size].  Waits for the stream."""
    L = _lib.load()
    n_pieces = int(piece_len.numel())
    if not (_is_bytes_tensor(dst, 2) and dst.shape[0] >= n_pieces and (dst.shape[1] <= 1 or dst.stride(1) == 1)):
        raise TypeError("dst must be the tensor deflate_pieces returned")
    if not (isinstance(piece_len, torch.Tensor) and piece_len.is_cuda and piece_len.dtype == torch.int32 and piece_len.is_contiguous()):
        raise TypeError("piece_len must be a contiguous CUDA int32 tensor")
    stride = int(dst.stride(0)) if dst.shape[0] > 1 else int(dst.shape[1])
    if out is None:
        out = torch.empty(n_pieces * int(dst.shape[1]), dtype=torch.uint8, device=dst.device)
    if not (_is_bytes_tensor(out, 1) and out.is_contiguous()):
        raise TypeError("out must be a contiguous one-dimensional CUDA uint8 tensor")
    cap = int(out.numel()) if out_cap is None else int(out_cap)
    if cap > out.numel():
        raise ValueError("out_cap is beyond out")
    total = ct.c_int64(0)
    check(L.icnv_deflate_pack_dev(_ptr(dst), stride, _ptr(piece_len), n_pieces, _ptr(out), cap, ct.byref(total), _stream()))
    return out[:total.value]


def _crc_mul(a, b):
    """a(x) * b(x) mod P over GF(2) in the CRC's reflected form (bit 31 is x^0): Python ints, or numpy uint32 arrays."""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.broadcast_arrays(np.asarray(a, dtype=np.uint32), np.asarray(b, dtype=np.uint32))
        b, p = b.copy(), np.zeros(a.shape, dtype=np.uint32)
        for i in range(32):
            p ^= np.where(a & np.uint32(0x80000000 >> i), b, np.uint32(0))
            b = np.where(b & np.uint32(1), (b >> np.uint32(1)) ^ np.uint32(_CRC_POLY), b >> np.uint32(1))
        return p
    p = 0
    for i in range(32):
        if a & (0x80000000 >> i):
            p ^= b
        b = (b >> 1) ^ _CRC_POLY if b & 1 else b >> 1
    return p


@functools.lru_cache(maxsize=256)
def crc32_shift_operator(n_bytes):
    """x^(8 * n_bytes) mod P: the operator that moves a CRC-32 across n_bytes of data (zlib's crc32_combine_gen).  Square and
    multiply on the bits of n_bytes: any length, nothing allocated.  (Cached: a stream's chunks ask for the same few.)"""
    n_bytes = int(n_bytes)
    if n_bytes < 0:
        raise ValueError("negative length")
    r, b = 0x80000000, 0x00800000            # x^0, x^8
    while n_bytes:
        if n_bytes & 1:
            r = _crc_mul(r, b)
        b = _crc_mul(b, b)
        n_bytes >>= 1
    return r


def crc32_combine(crc_a, crc_b, len_b):
    """zlib's crc32_combine: the CRC-32 of A + B from crc32(A), crc32(B) and len(B), as a pure function on the host."""
    return _crc_mul(crc32_shift_operator(len_b), int(crc_a) & 0xFFFFFFFF) ^ (int(crc_b) & 0xFFFFFFFF)


def crc32_combine_pieces(crcs, piece_bytes, last_bytes=None):
    """The CRC-32 of the concatenation of pieces of one common length: crcs[i] = crc32(piece i), every piece piece_bytes long
    but the last, which holds last_bytes (default piece_bytes).  A pairwise tree over numpy vectors: level k combines
    neighbours with the one operator x^(8 * piece_bytes * 2^k), so a payload of tens of thousands of pieces costs
    log2(pieces) operators, not one per piece.  An empty list gives 0, the CRC of no bytes."""
    c = (np.asarray(crcs).astype(np.int64).ravel() & 0xFFFFFFFF).astype(np.uint32)      # (int32 bit patterns are taken as they are)
    if c.size == 0:
        return 0
    last = int(c[-1])
    last_bytes = int(piece_bytes) if last_bytes is None else int(last_bytes)
    head = c[:-1]
    acc, span = 0, int(piece_bytes)
    if head.size:
        m = 1 << (int(head.size) - 1).bit_length()
        v = np.zeros(m, dtype=np.uint32)
        v[m - head.size:] = head             # leading zeros are neutral: 0 * x^k = 0
        while v.size > 1:
            v = _crc_mul(v[0::2], np.uint32(crc32_shift_operator(span))) ^ v[1::2]
            span *= 2
        acc = int(v[0])
    return crc32_combine(acc, last, last_bytes)


# ------------------------------------------------------------------ INFLATE in independent units (DESIGN K29)
def _is_vector(t, dtype):
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.dim() == 1 and t.is_contiguous()


def _bytes_vector(t, name):
    if not (_is_bytes_tensor(t, 1) and (t.numel() <= 1 or t.stride(0) == 1)):
        raise TypeError(f"{name} must be a contiguous one-dimensional CUDA uint8 tensor")
    return int(t.numel())


def inflate_scan(src, *, cand=None):
    """icnv_inflate_scan_dev (DESIGN K29): the offsets p in [4, n] of the CUDA uint8 vector src with src[p - 4:p] = 00 00 FF FF,
    ascending, as a CUDA int64 vector.  cand: a caller's int64 vector to fill (too small a one raises IcnvError, untouched);
    by default one is sized from the count.  Waits for the stream."""
    L = _lib.load()
    n = _bytes_vector(src, "src")
    own = cand is None
    if own:
        cand = torch.empty(max(1024, n >> 12), dtype=torch.int64, device=src.device)
    if not _is_vector(cand, torch.int64):
        raise TypeError("cand must be a contiguous CUDA int64 vector")
    count = ct.c_int64(0)
    rc = L.icnv_inflate_scan_dev(_ptr(src), n, _ptr(cand), int(cand.numel()), ct.byref(count), _stream())
    if own and rc == _lib.ERR_ARG and count.value > cand.numel():          # nothing was written: once more with room for all
        cand = torch.empty(count.value, dtype=torch.int64, device=src.device)
        rc = L.icnv_inflate_scan_dev(_ptr(src), n, _ptr(cand), int(cand.numel()), ct.byref(count), _stream())
    check(rc)
    return cand[:count.value]


def inflate_measure(src, start, max_in):
    """icnv_inflate_measure_dev: the units that start at the offsets `start` (CUDA int64) of src, parsed without producing
    bytes.  Returns (end, out_len, status): CUDA int64, int64, int32 (the INFLATE_* codes of _lib)."""
    L = _lib.load()
    n = _bytes_vector(src, "src")
    if not _is_vector(start, torch.int64):
        raise TypeError("start must be a contiguous CUDA int64 vector")
    k = int(start.numel())
    end = torch.empty(k, dtype=torch.int64, device=src.device)
    out_len = torch.empty(k, dtype=torch.int64, device=src.device)
    status = torch.empty(k, dtype=torch.int32, device=src.device)
    check(L.icnv_inflate_measure_dev(_ptr(src), n, _ptr(start), k, int(max_in), _ptr(end), _ptr(out_len), _ptr(status), _stream()))
    return end, out_len, status


def inflate_units(src, start, end, out_off, out_len, out):
    """icnv_inflate_units_dev: unit i, src[start[i]:end[i]], decoded into out[out_off[i]:out_off[i] + out_len[i]] (all CUDA
    int64 vectors of one length; out a CUDA uint8 vector).  Returns the status vector (CUDA int32)."""
    L = _lib.load()
    n, cap = _bytes_vector(src, "src"), _bytes_vector(out, "out")
    k = int(start.numel())
    for name, t in (("start", start), ("end", end), ("out_off", out_off), ("out_len", out_len)):
        if not (_is_vector(t, torch.int64) and t.numel() == k):
            raise TypeError(f"{name} must be a contiguous CUDA int64 vector of {k} elements")
    status = torch.empty(k, dtype=torch.int32, device=src.device)
    check(L.icnv_inflate_units_dev(_ptr(src), n, _ptr(start), _ptr(end), _ptr(out_off), _ptr(out_len), k, _ptr(out), cap, _ptr(status), _stream()))
    return status


def crc32_pieces(src, piece_bytes):
    """icnv_crc32_pieces_dev: the CRC-32 of every piece_bytes-sized piece of the CUDA uint8 vector src (the last one shorter), as
    int32 bit patterns like deflate_pieces' -- what crc32_combine_pieces folds.  Does not synchronise."""
    L = _lib.load()
    n = _bytes_vector(src, "src")
    piece_bytes = int(piece_bytes)
    if piece_bytes < 1:
        raise ValueError("piece_bytes must be at least 1")
    crc = torch.empty(-(-n // piece_bytes), dtype=torch.int32, device=src.device)
    check(L.icnv_crc32_pieces_dev(_ptr(src), n, piece_bytes, _ptr(crc), _stream()))
    return crc


# ------------------------------------------------------------------ INFLATE with unknown history (DESIGN K30)
def _int64_vectors(k, **named):
    for name, t in named.items():
        if not (_is_vector(t, torch.int64) and (k is None or t.numel() == k)):
            raise TypeError(f"{name} must be a contiguous CUDA int64 vector" + ("" if k is None else f" of {k} elements"))


def gunzip_find(src, *, cand=None):
    """icnv_gunzip_find_dev (DESIGN K30): every bit offset of the CUDA uint8 vector src (a raw DEFLATE stream) at which a
    non-final dynamic block's header parses, ascending, as a CUDA int64 vector.  cand: a caller's int64 vector to fill (too
    small a one raises IcnvError, untouched); by default one is sized from the count.  Waits for the stream."""
    L = _lib.load()
    n = _bytes_vector(src, "src")
    own = cand is None
    if own:
        cand = torch.empty(max(1024, n >> 10), dtype=torch.int64, device=src.device)
    _int64_vectors(None, cand=cand)
    count = ct.c_int64(0)
    rc = L.icnv_gunzip_find_dev(_ptr(src), n, _ptr(cand), int(cand.numel()), ct.byref(count), _stream())
    if own and rc == _lib.ERR_ARG and count.value > cand.numel():          # nothing was written: once more with room for all
        cand = torch.empty(count.value, dtype=torch.int64, device=src.device)
        rc = L.icnv_gunzip_find_dev(_ptr(src), n, _ptr(cand), int(cand.numel()), ct.byref(count), _stream())
    check(rc)
    return cand[:count.value]


def gunzip_measure(src, cand, start, max_in):
    """icnv_gunzip_measure_dev: the units that start at the BIT offsets `start` (CUDA int64) of src and stop on an offset of
    the ascending list `cand` or behind BFINAL, parsed without producing symbols.  Returns (end, out_len, status): CUDA int64
    (bits), int64, int32 (the GUNZIP_* codes of _lib)."""
    L = _lib.load()
    n = _bytes_vector(src, "src")
    _int64_vectors(None, cand=cand, start=start)
    k = int(start.numel())
    end = torch.empty(k, dtype=torch.int64, device=src.device)
    out_len = torch.empty(k, dtype=torch.int64, device=src.device)
    status = torch.empty(k, dtype=torch.int32, device=src.device)
    check(L.icnv_gunzip_measure_dev(_ptr(src), n, _ptr(cand), int(cand.numel()), _ptr(start), k, int(max_in), _ptr(end), _ptr(out_len),
                                    _ptr(status), _stream()))
    return end, out_len, status


def _is_symbols(sym):
    return _is_vector(sym, torch.int16)


def gunzip_symbols(src, cand, start, end, out_off, out_len, sym):
    """icnv_gunzip_symbols_dev: unit i, from bit start[i] to bit end[i] of src, decoded into the 16-bit symbols
    sym[out_off[i]:out_off[i] + out_len[i]] (sym: a CUDA int16 vector holding the uint16 bit patterns: below 256 a byte,
    0x8000 | w a marker; the int64 vectors of one length, out_off the prefix sums of out_len).  Returns the status vector."""
    L = _lib.load()
    n = _bytes_vector(src, "src")
    k = int(start.numel())
    _int64_vectors(None, cand=cand)
    _int64_vectors(k, start=start, end=end, out_off=out_off, out_len=out_len)
    if not _is_symbols(sym):
        raise TypeError("sym must be a contiguous CUDA int16 vector")
    status = torch.empty(k, dtype=torch.int32, device=src.device)
    check(L.icnv_gunzip_symbols_dev(_ptr(src), n, _ptr(cand), int(cand.numel()), _ptr(start), _ptr(end), _ptr(out_off), _ptr(out_len), k,
                                    _ptr(sym), int(sym.numel()), _ptr(status), _stream()))
    return status


def _gunzip_places(sym, out_off, out_len, out):
    cap = _bytes_vector(out, "out")
    k = int(out_off.numel())
    _int64_vectors(k, out_off=out_off, out_len=out_len)
    if not (_is_symbols(sym) and sym.numel() == cap):
        raise TypeError(f"sym must be a contiguous CUDA int16 vector of out's {cap} elements")
    return k, cap


def gunzip_tails(sym, out_off, out_len, out):
    """icnv_gunzip_tails_dev: the last min(32 768, out_len[i]) symbols of every unit resolved into out, unit after unit.
    Returns (bad, markers): CUDA int32 [1] (1: a marker pointed in front of byte 0) and CUDA int64 [1] (markers met)."""
    L = _lib.load()
    k, cap = _gunzip_places(sym, out_off, out_len, out)
    bad = torch.zeros(1, dtype=torch.int32, device=out.device)
    markers = torch.zeros(1, dtype=torch.int64, device=out.device)
    check(L.icnv_gunzip_tails_dev(_ptr(sym), _ptr(out_off), _ptr(out_len), k, _ptr(out), cap, _ptr(bad), _ptr(markers), _stream()))
    return bad, markers


def gunzip_resolve(sym, out_off, out_len, out):
    """icnv_gunzip_resolve_dev: every symbol in front of the units' tails resolved into out (after gunzip_tails).  Returns bad:
    CUDA int32 [1]."""
    L = _lib.load()
    k, cap = _gunzip_places(sym, out_off, out_len, out)
    bad = torch.zeros(1, dtype=torch.int32, device=out.device)
    check(L.icnv_gunzip_resolve_dev(_ptr(sym), _ptr(out_off), _ptr(out_len), k, _ptr(out), cap, _ptr(bad), _stream()))
    return bad


# ------------------------------------------------------------------ timing hooks
def timing_enable(on=True):
    """on: False / 0 off, True / 1 every kernel family, 2 only the hot launches "chain_apply" and "viterbi"."""
    _lib.load().icnv_timing_enable(2 if on == 2 and on is not True else int(bool(on)))


def timing_reset():
    _lib.load().icnv_timing_reset()


def timing_get(kernel):
    ms, n = ct.c_double(), ct.c_int64()
    check(_lib.load().icnv_timing_get(kernel.encode(), ct.byref(ms), ct.byref(n)))
    return ms.value, n.value
