"""plot_cnv (R/inferCNV_heatmap.R:90-470): the heatmap's data layer on the GPU (DESIGN K17) and the files R writes.

What is arithmetic on the matrix runs in libicnv_hip.so: the "auto" x.range quantiles (device.quantiles_excluding), the
colour key's counts (device.heatmap_bins), the binned panels (device.heatmap_raster) and the trees that order the cells
(device.hclust_cells, K9).  torch gathers and clamps; the host formats text and composes the page.  Drawing text, axes and
dendrograms is left out: the PNG holds the panels only and `<name>.heatmap_layout.json` says where they are and what
they show.

Believed, not verified against an R run (R is not installed where this was written):
  - seq(from, to, length.out = 16) is from + i * ((to - from) / 15) with the last element set to `to`
  - colorRampPalette interpolates linearly in RGB and rounds each channel half up
  - layout() uses the first ncol(lmat) of heatmap.cnv's widths (plot_cnv forces lmat and lhei, not lwid)
  - image(useRaster = TRUE) at device resolution samples nearest-neighbour
  - mean(expr.data), the default x.center, is taken as the correctly rounded sum divided by the count
"""
from __future__ import annotations

import json
import locale
import math
import os
import struct
import zlib

import numpy as np
import torch

from . import device
from .infercnv_object import DeviceMatrix, InfercnvObject
from .text_stream import stream_chunks
from .tumor_subclusters import HClust

NB_BREAKS = 16
SET3 = ("#8DD3C7", "#FFFFB3", "#BEBADA", "#FB8072", "#80B1D3", "#FDB462", "#B3DE69", "#FCCDE5", "#D9D9D9", "#BC80BD", "#CCEBC5",
        "#FFED6F")                                  # RColorBrewer::brewer.pal(12, "Set3")
R_COLORS = {"darkblue": (0, 0, 139), "white": (255, 255, 255), "darkred": (139, 0, 0), "purple3": (125, 38, 205),
            "darkorange2": (238, 118, 0), "black": (0, 0, 0)}


# ------------------------------------------------------------------ R's number formatting
def r_num(x):
    """A number as write.table / as.character print it: 15 significant digits, trailing zeros dropped, fixed notation unless
    scientific is strictly narrower, a two-digit exponent (formatReal with R_dec_min_exponent, scipen = 0)."""
    if isinstance(x, (int, np.integer)):
        return str(int(x))
    x = float(x)
    if x != x:
        return "NaN"
    if math.isinf(x):
        return "Inf" if x > 0 else "-Inf"
    if x == 0.0:
        return "0"
    mant, exp = ("%.14e" % abs(x)).split("e")
    e = int(exp)
    digits = mant.replace(".", "").rstrip("0") or "0"
    nsig = len(digits)
    neg = "-" if x < 0 else ""
    w_sci = len(neg) + (nsig + 1 if nsig > 1 else 1) + (4 if abs(e) < 100 else 5)
    rgt = max(0, nsig - e - 1)
    w_fix = len(neg) + (e + 1 if e >= 0 else 1) + (rgt + 1 if rgt else 0)
    if w_fix <= w_sci:
        if e >= 0:
            whole = (digits + "0" * (e + 1 - nsig))[:e + 1]
            frac = digits[e + 1:]
        else:
            whole, frac = "0", "0" * (-e - 1) + digits
        return neg + whole + ("." + frac if frac else "")
    return neg + digits[0] + ("." + digits[1:] if nsig > 1 else "") + ("e+" if e >= 0 else "e-") + "%02d" % abs(e)


# ------------------------------------------------------------------ palettes
def _hex(rgb):
    return "#%02X%02X%02X" % tuple(int(v) for v in rgb)


def _rgb(color):
    if isinstance(color, str) and color.startswith("#") and len(color) == 7:
        return tuple(int(color[i:i + 2], 16) for i in (1, 3, 5))
    if color in R_COLORS:
        return R_COLORS[color]
    raise ValueError(f"colour {color!r}: use '#RRGGBB' or one of {sorted(R_COLORS)}")


def color_ramp(stops, n):
    """colorRampPalette(stops)(n): n colours at equal steps along the stops, linear in RGB, each channel rounded half up."""
    rgb = [_rgb(c) for c in stops]
    m = len(rgb)
    out = []
    for i in range(n):
        pos = (i * (m - 1)) / (n - 1) if n > 1 and m > 1 else 0.0
        k = min(int(math.floor(pos)), m - 2) if m > 1 else 0
        f = pos - k
        a, b = rgb[k], rgb[min(k + 1, m - 1)]
        out.append(_hex(tuple(math.floor(a[c] + (b[c] - a[c]) * f + 0.5) for c in range(3))))
    return out


def group_colors(n):
    """get_group_color_palette()(n) = colorRampPalette(brewer.pal(12, "Set3"))(n)  (R/inferCNV_heatmap.R:8-10)."""
    return color_ramp(SET3, n)


def color_palette(steps, between):
    """color.palette(steps, between) (R/inferCNV_ops.R:1808-1835): `between[i]` colours interpolated between steps i and
    i + 1, then colorRampPalette over all of them.  Returns the function n -> colours."""
    rgb = [_rgb(c) for c in steps]
    full = [_hex(rgb[0])]
    for i, extra in enumerate(between):
        a, b = rgb[i], rgb[i + 1]
        for t in range(1, extra + 1):            # seq(a, b, length.out = extra + 2)[2 .. extra + 1]
            full.append(_hex(tuple(math.floor(a[c] + t * ((b[c] - a[c]) / (extra + 1)) + 0.5) for c in range(3))))
        full.append(_hex(b))
    return lambda n: color_ramp(full, n)


# ------------------------------------------------------------------ trees
def cutree_k(merge, k):
    """cutree(tree, k = k): the groups after the first n - k merges, numbered 1.. in order of first appearance among the
    cells (in label order, not dendrogram order)."""
    merge = np.asarray(merge)
    n = merge.shape[0] + 1
    k = int(k)
    if not 1 <= k <= n:
        raise ValueError("elements of 'k' must be between 1 and %d" % n)
    parent = list(range(2 * n - 1))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for step in range(n - k):
        for v in merge[step]:
            parent[find(-int(v) - 1 if v < 0 else n + int(v) - 1)] = n + step
    seen, labels = {}, np.zeros(n, dtype=np.int64)
    for c in range(n):
        labels[c] = seen.setdefault(find(c), len(seen) + 1)
    return labels


def _seq(lo, hi, n):
    by = (hi - lo) / (n - 1)
    out = [lo + i * by for i in range(n)]
    out[-1] = hi
    return np.array(out, dtype=np.float64)


# ------------------------------------------------------------------ write.table
def _q(s):
    return '"' + str(s).replace('"', '\\"') + '"'


def write_table(path, rows, row_names=None, col_names=None, quote=True, sep=" "):
    """write.table: a header of column names (none for the row names), then one line per row.  Strings are quoted when
    `quote`; numbers are printed by r_num, each by itself."""
    fmt = lambda v: (_q(v) if quote else str(v)) if isinstance(v, str) else r_num(v)
    with open(path, "w", newline="\n") as f:
        if col_names is not None:
            f.write(sep.join(fmt(str(c)) for c in col_names) + "\n")
        for i, row in enumerate(rows):
            cells = [fmt(v) for v in row]
            if row_names is not None:
                cells.insert(0, fmt(str(row_names[i])))
            f.write(sep.join(cells) + "\n")



TABLE_TEXT_CHUNK = 256 << 20       # bytes of one chunk of write_matrix; ICNV_TABLE_TEXT_CHUNK (developer switch) overrides it


def write_matrix(path, x, cells, orientation, row_names=None, col_names=None, quote=True, sep=" "):
    """write.table of a matrix that lives on the device (DESIGN K20): the file write_table writes for the same names, with the
    numbers formatted by device.format_table_into instead of r_num.  x: (C, G) CUDA float64 with contiguous rows.
    orientation "gene_rows": one line per gene, its numbers over `cells` in the order given (expr.<name>.dat, the
    observations / references files, the one-member General_HCL file); "cell_rows": one line per listed cell, its numbers
    over all genes (the other members files).  row_names: one per line, or None.

    The header line is written here.  The body is streamed in chunks of whole rows through two device buffers and two pinned
    host buffers (text_stream.stream_chunks): while the library formats chunk i + 1, chunk i is copied to the host on a second
    stream and a writer thread hands chunk i - 1 to the file.  Returns a dict of counts and seconds (format_s: inside the
    library; copy_wait_s and write_s: the writer thread waiting for a copy and inside f.write; stall_s: this thread waiting
    for a free buffer; wall_s: from the first chunk to the last write, the buffers' allocation left out)."""
    code = device.TABLE_ORIENTATIONS[orientation]
    C, G = x.shape
    cells = np.ascontiguousarray(cells, dtype=np.int32)
    n_rows, n_fields = (G, cells.size) if code == device._lib.TABLE_GENE_ROWS else (cells.size, G)
    enc = locale.getpreferredencoding(False)
    fmt = lambda v: _q(v) if quote else str(v)
    packed = None
    if row_names is not None:
        if len(row_names) != n_rows:
            raise ValueError("one row name per line")
        packed = device.pack_labels([fmt(str(r)).encode(enc) for r in row_names])
    worst = n_rows * n_fields * 23 + (int(packed[1][-1]) + n_rows if packed else 0)
    cap = max(1, min(int(os.environ.get("ICNV_TABLE_TEXT_CHUNK", TABLE_TEXT_CHUNK)), worst))
    rows = {"next": 0}

    def fill(buf):
        if rows["next"] >= n_rows:
            return None
        done, nbytes, _ = device.format_table_into(x, buf, rows["next"], n_rows - rows["next"], cells, code, packed, sep)
        rows["next"] += done
        return nbytes

    with open(path, "wb") as f:
        if col_names is not None:
            f.write((sep.join(fmt(str(c)) for c in col_names) + "\n").encode(enc))
        return stream_chunks(f, cap, x.device, fill)


# ------------------------------------------------------------------ PNG
def write_png(path, rgb):
    """An (H, W, 3) uint8 array as an 8-bit RGB PNG (filter 0 on every row), with zlib from the standard library."""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    H, W, _ = rgb.shape
    raw = np.concatenate([np.zeros((H, 1), dtype=np.uint8), rgb.reshape(H, W * 3)], axis=1).tobytes()

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


# ------------------------------------------------------------------ page geometry
def _half_up(v):
    return int(math.floor(v + 0.5))


def page_geometry(obs_names, ref_names, nobs, png_res, dynamic_resize):
    """The page of plot_cnv in pixels (R/inferCNV_heatmap.R:254-306, .plot_observations_layout :926-958, the widths of
    heatmap.cnv :1961-2011): the edges of the 16 layout rows and 14 layout columns and the boxes of the panels."""
    dyn = dynamic_resize * 3.6 * (nobs - 200) / 200 if nobs > 200 else 0
    coln1 = max(1, int(math.floor(123 / (max(len(s) for s in obs_names) + 6))))
    coln2 = max(1, int(math.floor(123 / (max(len(s) for s in ref_names) + 6)))) if ref_names else 1
    rown1, rown2 = int(math.ceil(len(obs_names) / coln1)), int(math.ceil(len(ref_names) / coln2))
    gk = ((rown2 + 2) * 0.175, (rown1 + 3) * 0.175)
    height = 8.22 + (gk[0] + gk[1]) + dyn
    if height > 32768 / png_res:                                  # cairo's limit (:295-301)
        height = math.floor(((32767 / png_res) - 5e-3) * 100 + 0.5) / 100
        dyn = height - 8.22 - (gk[0] + gk[1])
    lhei = [1.125, 2.215, 0.15] + [0.5] * 8 + [0.5 + dyn, 0.1, gk[0], gk[1], 0.13]
    lwid = [1.5, 0.2, 0.2, 0.02] + [9 / 12] * 10
    W, H = _half_up(10 * png_res), _half_up(height * png_res)
    ys, acc = [0], 0.0
    for h in lhei:
        acc += h
        ys.append(min(H, _half_up(acc / sum(lhei) * H)))
    xs, acc = [0], 0.0
    for w in lwid:
        acc += w
        xs.append(min(W, _half_up(acc / sum(lwid) * W)))
    ys[-1], xs[-1] = H, W
    box = lambda c0, c1, r0, r1: [xs[c0], ys[r0], xs[c1], ys[r1]]          # x0, y0, x1, y1 (exclusive)
    panels = {"observations": box(4, 14, 3, 12), "references": box(4, 14, 1, 2), "contigs": box(4, 14, 2, 3),
              "observation_dendrogram_colors": box(1, 2, 3, 12), "observation_annotation_colors": box(2, 3, 3, 12),
              "reference_annotation_colors": box(2, 3, 1, 2), "key": box(0, 1, 1, 2)}
    return {"width": W, "height": H, "height_in": height, "dynamic_extension": dyn, "panels": panels}


# ------------------------------------------------------------------ cell orders
def _tree_cells(tree, index_of):
    return [index_of[str(l)] for l in np.asarray(tree.labels)[np.asarray(tree.order, dtype=np.int64) - 1]]


def _group_order_from_subclusters(ts, name, index_of):
    """The cells of annotation group `name` as its stored tree(s) order them (:586-617)."""
    hc = ts["hc"].get(name)
    subs = ts["subclusters"][name]
    if isinstance(hc, HClust):
        return _tree_cells(hc, index_of)
    if isinstance(hc, (list, tuple)):        # the Leiden branch: partition by partition, each by its own tree
        trees, out = list(hc), []
        for cells in subs.values():
            cells = [int(c) for c in np.asarray(cells).ravel()]
            out += _tree_cells(trees.pop(0), index_of) if len(cells) >= 2 else cells
        return out
    cells = [int(c) for v in subs.values() for c in np.asarray(v).ravel()]
    if len(cells) not in (1, 2):
        raise ValueError(f"group {name!r} has no tree and {len(cells)} cells (R: 'Unexpected error, should not happen.')")
    return cells


def _subcluster_of(ts, name):
    return {int(c): sub for sub, cells in ts["subclusters"][name].items() for c in np.asarray(cells).ravel()}


def _hclust_orders(x, groups, method):
    """hclust(parallelDist(cells x all genes), method)$order for every group of >= 2 cells, in one K9 call."""
    G = x.shape[1]
    genes = np.arange(G, dtype=np.int32)
    res = device.hclust_cells(x, [(genes, np.asarray(g, dtype=np.int32)) for g in groups], method)
    return [(m.cpu().numpy(), np.asarray(g)[o.cpu().numpy().astype(np.int64) - 1].tolist()) for g, (m, _, o) in zip(groups, res)]


def observation_order(obj, x, obs_cells, obs_group_of, obs_names, cluster_by_groups, k_obs_groups, hclust_method):
    """.plot_cnv_observations' ordering (:581-796).  Returns (ordered cells, split group per ordered cell, annotation group
    per ordered cell (1-based), separator positions counted in ordered cells, whether the route writes member files)."""
    names = [str(s) for s in obj.cells()]
    index_of = {s: i for i, s in enumerate(names)}
    ts = obj.tumor_subclusters
    ordered, split, seps = [], [], []
    if ts is not None and cluster_by_groups:
        ann = []
        for i, name in enumerate(obs_names):
            cells = _group_order_from_subclusters(ts, name, index_of)
            sub = _subcluster_of(ts, name)
            ordered += cells
            split += [sub[c] for c in cells]
            ann += [i + 1] * len(cells)
            seps.append(len(ordered))
        return ordered, split, ann, seps, False
    if ts is not None:
        hc = ts["hc"].get("all_observations")
        if not isinstance(hc, HClust):
            raise ValueError("cluster_by_groups = False needs tumor_subclusters$hc$all_observations to be one tree")
        ordered = _tree_cells(hc, index_of)
        if k_obs_groups > 1:
            by_label = dict(zip((index_of[str(l)] for l in hc.labels), cutree_k(hc.merge, k_obs_groups).tolist()))
            split = [by_label[c] for c in ordered]
        else:
            sub = _subcluster_of(ts, "all_observations")
            split = [sub[c] for c in ordered]
    elif cluster_by_groups:
        groups = [[c for c in obs_cells if obs_group_of[c] == i + 1] for i in range(max(obs_group_of.values()))]
        trees = iter(_hclust_orders(x, [g for g in groups if len(g) >= 2], hclust_method))
        ann = []
        for i, g in enumerate(groups):
            ordered += next(trees)[1] if len(g) >= 2 else g
            ann += [i + 1] * len(g)
            seps.append(len(ordered))
        return ordered, [1] * len(ordered), ann, seps, False
    elif len(obs_cells) > 1:
        (merge, ordered), = _hclust_orders(x, [obs_cells], hclust_method)
        by_cell = dict(zip(obs_cells, cutree_k(merge, k_obs_groups).tolist()))
        split = [by_cell[c] for c in ordered]
    else:
        return list(obs_cells), [1], [obs_group_of[obs_cells[0]]], [1], False
    acc = 0
    for grp in dict.fromkeys(split):             # unique(split_groups), in order of appearance
        acc += sum(1 for s in split if s == grp)
        seps.append(acc)
    return ordered, split, [obs_group_of[c] for c in ordered], seps, True


def reference_order(x, ref_groups, cluster_references, hclust_method):
    """.plot_cnv_references' ordering (:1058-1090): (ordered cells, group per ordered cell (1-based), separators)."""
    groups = [[int(c) for c in np.asarray(g).ravel()] for g in ref_groups]
    if len(groups) > 1:
        todo = [g for g in groups if cluster_references and len(g) > 2]
        trees = iter(_hclust_orders(x, todo, hclust_method)) if todo else iter(())
        groups = [next(trees)[1] if cluster_references and len(g) > 2 else g for g in groups]
        seps = np.cumsum([len(g) for g in groups])[:-1].tolist()
    else:
        if cluster_references and len(groups[0]) > 1:    # (one cell: R's hclust would stop; the cell is shown as it is)
            (_, o), = _hclust_orders(x, groups, hclust_method)
            groups = [o]
        seps = []
    return [c for g in groups for c in g], [i + 1 for i, g in enumerate(groups) for _ in g], seps


# ------------------------------------------------------------------ the page
def _runs(values):
    """[(value, first index, one past the last)] of the runs of equal neighbours."""
    out, start = [], 0
    for i in range(1, len(values) + 1):
        if i == len(values) or values[i] != values[start]:
            out.append((values[start], start, i))
            start = i
    return out


def _sample(n, size):
    return [((2 * i + 1) * n) // (2 * size) for i in range(size)]


def _fill(img, box, rgb):
    img[box[1]:box[3], box[0]:box[2]] = rgb


def compose_page(geo, colors, obs, ref, contig_of_gene, contig_colors, counts):
    """The RGB page and the pixel spans of its labels.  obs / ref: dicts with `bins` ((h, w) uint8 from heatmap_raster, rows
    top-down), `rows` (per raster cell position top-down: (dendrogram colour, annotation colour, annotation name)), `seps`
    (boundaries in raster cell positions).  ref may be None."""
    img = np.full((geo["height"], geo["width"], 3), 255, dtype=np.uint8)
    lut = np.array([_rgb(c) for c in colors], dtype=np.uint8)
    G = len(contig_of_gene)
    spans = {}
    for key, part in (("observations", obs), ("references", ref)):
        if part is None:
            continue
        x0, y0, x1, y1 = geo["panels"][key]
        h, w = y1 - y0, x1 - x0
        n = len(part["rows"])
        panel = lut[part["bins"]]
        gene_of_px, cell_of_px = _sample(G, w), _sample(n, h)
        for j in range(1, w):                     # a contig border: the first pixel column of the next contig
            if contig_of_gene[gene_of_px[j]] != contig_of_gene[gene_of_px[j - 1]]:
                panel[:, j] = 0
        for s in part["seps"]:
            if 0 < s < n:
                i = next((i for i in range(h) if cell_of_px[i] >= s), None)
                if i is not None:
                    panel[i, :] = 0
        img[y0:y1, x0:x1] = panel
        bars = (("observation_dendrogram_colors", 0), ("observation_annotation_colors", 1)) if key == "observations" else \
            (("reference_annotation_colors", 1),)
        for bar, col in bars:
            bx0, _, bx1, _ = geo["panels"][bar]
            for i in range(h):
                img[y0 + i, bx0:bx1] = _rgb(part["rows"][cell_of_px[i]][col])
        spans[key] = [{"name": v[2], "color": v[1], "y0": y0 + a, "y1": y0 + b}
                      for v, a, b in _runs([part["rows"][c] for c in cell_of_px])]
        if key == "observations":
            cx0, cy0, cx1, cy1 = geo["panels"]["contigs"]
            for j in range(w):
                img[cy0:cy1, x0 + j] = _rgb(contig_colors[contig_of_gene[gene_of_px[j]]])
            spans["contigs"] = [{"name": v, "color": contig_colors[v], "x0": x0 + a, "x1": x0 + b}
                                for v, a, b in _runs([contig_of_gene[g] for g in gene_of_px])]
    kx0, ky0, kx1, ky1 = geo["panels"]["key"]
    top, nbin = max(int(c) for c in counts), len(counts)
    for b in range(nbin):
        bar_h = (int(counts[b]) * (ky1 - ky0)) // top if top else 0
        img[ky1 - bar_h:ky1, kx0 + (b * (kx1 - kx0)) // nbin:kx0 + ((b + 1) * (kx1 - kx0)) // nbin] = lut[b]
    return img, spans


# ------------------------------------------------------------------ plot_cnv
def plot_cnv(infercnv_obj: InfercnvObject, out_dir=".", title="inferCNV", obs_title="Observations (Cells)",
             ref_title="References (Cells)", cluster_by_groups=True, cluster_references=True, plot_chr_scale=False,
             chr_lengths=None, k_obs_groups=1, contig_cex=1, x_center=None, x_range="auto", hclust_method="ward.D",
             custom_color_pal=None, color_safe_pal=False, output_filename="infercnv", output_format="png", png_res=300,
             dynamic_resize=0, ref_contig=None, write_expr_matrix=False, write_phylo=False, useRaster=True):
    """plot_cnv (R/inferCNV_heatmap.R:90-470) with the reference's formals (x.center / x.range spelt x_center / x_range; NA
    is None) and its return value, a dict of the settings used.

    Written into out_dir, with R's names and layouts: `<name>.heatmap_thresholds.txt`, `<name>.observation_groupings.txt`,
    `General_HCL_<g>_members.txt` on the cluster_by_groups = False routes, and with write_expr_matrix `expr.<name>.dat`,
    `<name>.observations.txt`, `<name>.references.txt` (the clamped matrices, genes x cells in plotted order).  With
    output_format "png": `<name>.heatmap.png` -- the observation and reference panels, black separators at contig and group
    borders, the row colour bars, the contig colour bar and the colour key with the bin counts as bars, at the pixel sizes of
    R's page -- and `<name>.heatmap_layout.json` with what a front end needs to label it.  The PNG has no text and is not
    named infercnv.png: it does not claim to be R's page.

    x_range: "auto" (the 1 % / 99 % quantiles of the values that differ from x_center, :159-165), a (low, high) pair
    (validated as :175-177), or None: no clamping, and the breaks span the data's minimum and maximum (R's seq(NA, NA) would
    stop).  x_center defaults to the mean of the matrix.  custom_color_pal: a function n -> '#RRGGBB' colours.

    Cells: observations as .plot_cnv_observations orders them (:581-796), first cell at the bottom of the panel; from
    tumor_subclusters when present, else by K9 (hclust_method).  A Leiden group's `hc` is, in this library, the list of its
    partitions' trees: its cells are ordered partition by partition in subcluster order, each by its own tree -- ape's
    binding of them into one tree is not mirrored.  References as :1058-1090, first cell at the top.

    ref_contig, plot_chr_scale = True, write_phylo = True and output_format "pdf" raise NotImplementedError."""
    return _plot_cnv(infercnv_obj, None, out_dir, title, obs_title, ref_title, cluster_by_groups, cluster_references, plot_chr_scale,
                     chr_lengths, k_obs_groups, contig_cex, x_center, x_range, hclust_method, custom_color_pal, color_safe_pal,
                     output_filename, output_format, png_res, dynamic_resize, ref_contig, write_expr_matrix, write_phylo, useRaster)


def _plot_cnv(infercnv_obj, x_dev, out_dir, title, obs_title, ref_title, cluster_by_groups, cluster_references, plot_chr_scale,
              chr_lengths, k_obs_groups, contig_cex, x_center, x_range, hclust_method, custom_color_pal, color_safe_pal,
              output_filename, output_format, png_res, dynamic_resize, ref_contig, write_expr_matrix, write_phylo, useRaster):
    """plot_cnv's body.  x_dev: the object's matrix as a contiguous (C, G) CUDA float64 tensor when the caller holds it on
    the device already (plot_per_group's gathers; expr_data is then not read), or None: expr_data is uploaded."""
    if hclust_method not in device.HCLUST_METHODS:
        raise ValueError(f"Error, hclust_method: {hclust_method} is not supported")
    if output_format not in ("png", "pdf", None):
        raise ValueError(f"Error, output_format: {output_format} is not supported")
    if ref_contig is not None:
        raise NotImplementedError("ref_contig needs a contig-restricted reclustering")
    if plot_chr_scale:
        raise NotImplementedError("plot_chr_scale = TRUE needs image() on uneven cells")
    if write_phylo:
        raise NotImplementedError("write_phylo = TRUE needs ape's Newick writer")
    if output_format == "pdf":
        raise NotImplementedError("output_format 'pdf': only the PNG panels are produced")
    obj = infercnv_obj
    os.makedirs(out_dir, exist_ok=True)
    if x_dev is not None:
        x = x_dev
    elif isinstance(obj.expr_data, DeviceMatrix):            # a resident object (DESIGN K32): drawn from where it lives
        x = obj.expr_data.float_tensor()
    else:
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(obj.expr_data, dtype=np.float64).T)).cuda()
    C, G = x.shape
    genes, cells = [str(g) for g in obj.genes()], [str(c) for c in obj.cells()]
    if x_center is None:
        x_center = device.matrix_mean(x)         # (K23: math.fsum's bits, without the host's seconds per 10^8 values)
    x_center = float(x_center)
    out = lambda name: os.path.join(out_dir, name)

    if write_expr_matrix:                        # (the matrix as it came, before the clamp)
        write_matrix(out(f"expr.{output_filename}.dat"), x, np.arange(C), "gene_rows", genes, cells, quote=False, sep="\t")

    if x_range is None:
        mm = device.quantiles_excluding(x, float("nan"), (0.0, 1.0))
        low, high = mm["min"], mm["max"]
    else:
        if isinstance(x_range, str):
            if x_range != "auto":
                raise ValueError("x_range: 'auto', a (low, high) pair or None")
            q = device.quantiles_excluding(x, x_center, (0.01, 0.99))["quantiles"]
            delta = max(abs(x_center - float(q[0])), abs(float(q[1]) - x_center))
            low, high = x_center - delta, x_center + delta
        else:
            low, high = float(x_range[0]), float(x_range[1])
            if low > x_center or high < x_center or low >= high:
                raise ValueError(f"Error, problem with relative values of x.range: {x_range}, and x.center: {x_center}")
        x = torch.clamp(x, low, high)
    breaks = _seq(low, high, NB_BREAKS)

    contigs = [str(c) for c in np.asarray(obj.gene_order.chr)]
    unique_contigs = list(dict.fromkeys(contigs))
    contig_colors = dict(zip(unique_contigs, group_colors(len(unique_contigs))))
    if custom_color_pal is not None:
        pal = custom_color_pal
    elif not color_safe_pal:
        pal = color_palette(("darkblue", "white", "darkred"), (2, 2))
    else:
        pal = color_palette(("purple3", "white", "darkorange2"), (2, 2))
    colors = list(pal(NB_BREAKS - 1))

    obs_names = list(obj.observation_grouped_cell_indices)
    ref_names = list(obj.reference_grouped_cell_indices)
    ref_set = {int(c) for g in obj.reference_grouped_cell_indices.values() for c in np.asarray(g).ravel()}
    obs_group_of = {c: -1 for c in range(C)}
    for i, g in enumerate(obj.observation_grouped_cell_indices.values()):
        for c in np.asarray(g).ravel():
            obs_group_of[int(c)] = i + 1
    obs_cells = [c for c in range(C) if c not in ref_set]
    nobs = sum(len(np.asarray(g).ravel()) for g in obj.observation_grouped_cell_indices.values())

    ordered, split, ann, seps, members = observation_order(obj, x, obs_cells, obs_group_of, obs_names, cluster_by_groups,
                                                           int(k_obs_groups), hclust_method)
    if members:                                  # (x: the clamped matrix, on the device)
        for grp in dict.fromkeys(split):
            memb = [c for c, s in zip(ordered, split) if s == grp]
            path = out(f"General_HCL_{r_num(grp) if not isinstance(grp, str) else grp}_members.txt")
            if len(memb) == 1:                   # obs_data[one name, ] drops to a vector: as.matrix makes it a column "V1"
                write_matrix(path, x, memb, "gene_rows", genes, ["V1"])
            else:
                write_matrix(path, x, memb, "cell_rows", [cells[c] for c in memb], genes)

    split_idx = {g: i for i, g in enumerate(dict.fromkeys(split))}
    dend_pal = group_colors(len(split_idx))
    ann_pal = group_colors(len(set(ann)))
    ann_color = lambda a: ann_pal[a - 1] if 1 <= a <= len(ann_pal) else "NA"
    rows = [(str(s) if isinstance(s, str) else r_num(s), dend_pal[split_idx[s]], r_num(a), ann_color(a))
            for s, a in zip(split, ann)]
    write_table(out(f"{output_filename}.observation_groupings.txt"), [list(r) for r in rows], [cells[c] for c in ordered],
                ["Dendrogram Group", "Dendrogram Color", "Annotation Group", "Annotation Color"])
    write_table(out(f"{output_filename}.heatmap_thresholds.txt"), [[float(b)] for b in breaks])

    ref_ordered, ref_split, ref_seps = [], [], []
    if ref_names:
        ref_ordered, ref_split, ref_seps = reference_order(x, list(obj.reference_grouped_cell_indices.values()),
                                                           cluster_references, hclust_method)
    if write_expr_matrix:
        write_matrix(out(f"{output_filename}.observations.txt"), x, ordered, "gene_rows", genes, [cells[c] for c in ordered])
        if ref_names:
            write_matrix(out(f"{output_filename}.references.txt"), x, ref_ordered, "gene_rows", genes, [cells[c] for c in ref_ordered])

    if output_format == "png":
        geo = page_geometry(obs_names, ref_names, nobs, png_res, 0 if dynamic_resize is None or dynamic_resize < 0 else dynamic_resize)
        counts = device.heatmap_bins(x, breaks, ordered)
        group_name = lambda a: obs_names[a - 1] if 1 <= a <= len(obs_names) else "NA"
        top_down = list(range(len(ordered) - 1, -1, -1))          # the first ordered cell is drawn at the bottom
        bx = geo["panels"]["observations"]
        obs = {"bins": device.heatmap_raster(x, breaks, [ordered[i] for i in top_down], bx[3] - bx[1], bx[2] - bx[0]).cpu().numpy(),
               "rows": [(rows[i][1], rows[i][3], group_name(ann[i])) for i in top_down],
               "seps": [len(ordered) - s for s in seps]}
        ref, ref_counts = None, None
        if ref_names:
            ref_pal = group_colors(len(set(ref_split)))
            bx = geo["panels"]["references"]
            ref = {"bins": device.heatmap_raster(x, breaks, ref_ordered, bx[3] - bx[1], bx[2] - bx[0]).cpu().numpy(),
                   "rows": [("NA", ref_pal[s - 1], ref_names[s - 1]) for s in ref_split], "seps": ref_seps}
            ref_counts = device.heatmap_bins(x, breaks, ref_ordered)
        img, spans = compose_page(geo, colors, obs, ref, contigs, contig_colors, counts)
        write_png(out(f"{output_filename}.heatmap.png"), img)
        layout = {"width": geo["width"], "height": geo["height"], "png_res": png_res, "title": title, "obs_title": obs_title,
                  "ref_title": ref_title, "contig_cex": contig_cex, "panels": geo["panels"], "contigs": spans["contigs"],
                  "observation_groups": spans["observations"], "reference_groups": spans.get("references", []),
                  "breaks": [float(b) for b in breaks], "colors": colors, "counts": [int(c) for c in counts],
                  "reference_counts": None if ref_counts is None else [int(c) for c in ref_counts]}
        with open(out(f"{output_filename}.heatmap_layout.json"), "w") as f:
            json.dump(layout, f, indent=1)
    return {"cluster_by_groups": cluster_by_groups, "k_obs_groups": k_obs_groups, "contig_cex": contig_cex, "x.center": x_center,
            "x.range": None if x_range is None else (low, high), "hclust_method": hclust_method, "color_safe_pal": color_safe_pal,
            "output_format": output_format, "png_res": png_res, "dynamic_resize": dynamic_resize}
