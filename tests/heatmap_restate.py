"""Sequential NumPy restatement of the data layer of plot_cnv (include/icnv.h "data layer of plot_cnv", DESIGN K17;
infercnv_amd/heatmap.py), written from R/inferCNV_heatmap.R and R's own sources:

  - quantiles_excluding: quantile(x[x != exclude], probs, type = 7) on np.sort of the kept values
  - bincode:             .bincode(v, breaks, right = TRUE, include.lowest = TRUE) after the clamp of :1934-1935
  - raster:              the nearest-neighbour panel of bin indices
  - cutree_k, the observation and reference orders (.plot_cnv_observations :581-796, .plot_cnv_references :1058-1090),
    with tests/hclust_restate.py for the trees
  - brewer_set3 / color_ramp / color_palette, r_num (R's number formatting), the write.table writers, the page geometry
  - plot_cnv: every file of the product's plot_cnv, built one value at a time
  - png_decode: a PNG reader on zlib.decompress
"""
import json
import math
import os
import struct
import zlib

import numpy as np

import hclust_restate as hr


# ---------------------------------------------------------------- device entry points
def quantiles_excluding(x, exclude, probs):
    v = np.asarray(x, dtype=np.float64).ravel()
    s = np.sort(v[v != exclude] + 0.0)          # -0.0 + 0.0 = +0.0
    n = s.size
    q, lo_v, hi_v = [], [], []
    for p in np.asarray(probs, dtype=np.float64).ravel():
        index = np.float64(n - 1) * p
        lo, hi = math.floor(index), math.ceil(index)
        xl, xh = s[lo], s[hi]
        h = index - lo
        q.append(xl if (index == lo or xh == xl) else (1.0 - h) * xl + h * xh)
        lo_v.append(xl)
        hi_v.append(xh)
    allv = v + 0.0
    return {"quantiles": np.array(q), "lo": np.array(lo_v), "hi": np.array(hi_v), "n_kept": int(n), "n_excluded": int(v.size - n),
            "min": float(allv.min()), "max": float(allv.max())}


def bincode(v, breaks):
    breaks = np.asarray(breaks, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    v = np.where(v < breaks[0], breaks[0], v)
    v = np.where(v > breaks[-1], breaks[-1], v)
    return np.maximum(np.searchsorted(breaks, v, side="left") - 1, 0)      # first i with breaks[i] >= v, minus one


def bins(x_cg, breaks, rows):
    b = bincode(np.asarray(x_cg)[np.asarray(rows, dtype=np.int64)], breaks)
    return np.bincount(b.ravel(), minlength=len(breaks) - 1).astype(np.int64)


def raster(x_cg, breaks, order, H, W):
    x_cg = np.asarray(x_cg)
    order = np.asarray(order, dtype=np.int64)
    n, G = order.size, x_cg.shape[1]
    ri = order[[((2 * i + 1) * n) // (2 * H) for i in range(H)]]
    ci = np.array([((2 * j + 1) * G) // (2 * W) for j in range(W)], dtype=np.int64)
    return bincode(x_cg[ri][:, ci], breaks).astype(np.uint8)


# ---------------------------------------------------------------- R's number formatting
def r_num(x):
    """15 significant digits, trailing zeros dropped, fixed unless scientific is strictly narrower, two-digit exponent."""
    if isinstance(x, (int, np.integer)):
        return "%d" % x
    from decimal import Decimal
    x = float(x)
    if x == 0:
        return "0"
    sign, digits, exp = Decimal(format(abs(x), ".15g")).normalize().as_tuple()
    nsig = len(digits)
    e10 = exp + nsig - 1                        # the value is d.ddd x 10^e10
    ds = "".join(str(d) for d in digits)
    sci = ds[0] + ("." + ds[1:] if nsig > 1 else "") + "e" + ("-" if e10 < 0 else "+") + str(abs(e10)).rjust(2, "0")
    if e10 < 0:
        fixed = "0." + "0" * (-e10 - 1) + ds
    elif nsig <= e10 + 1:
        fixed = ds + "0" * (e10 + 1 - nsig)
    else:
        fixed = ds[:e10 + 1] + "." + ds[e10 + 1:]
    return ("-" if x < 0 else "") + (fixed if len(fixed) <= len(sci) else sci)


# ---------------------------------------------------------------- palettes
BREWER_SET3 = ["#8DD3C7", "#FFFFB3", "#BEBADA", "#FB8072", "#80B1D3", "#FDB462", "#B3DE69", "#FCCDE5", "#D9D9D9", "#BC80BD",
               "#CCEBC5", "#FFED6F"]
NAMED = {"darkblue": "#00008B", "white": "#FFFFFF", "darkred": "#8B0000", "purple3": "#7D26CD", "darkorange2": "#EE7600"}


def _channels(c):
    c = NAMED.get(c, c)
    return [int(c[1:3], 16), int(c[3:5], 16), int(c[5:7], 16)]


def _to_hex(ch):
    return "#" + "".join("%02X" % v for v in ch)


def color_ramp(stops, n):
    m = len(stops)
    out = []
    for i in range(n):
        pos = 0.0 if (n == 1 or m == 1) else (i * (m - 1)) / (n - 1)
        k = int(pos)
        if k > m - 2:
            k = max(m - 2, 0)
        f = pos - k
        a, b = _channels(stops[k]), _channels(stops[min(k + 1, m - 1)])
        out.append(_to_hex([int(math.floor(a[c] + (b[c] - a[c]) * f + 0.5)) for c in range(3)]))
    return out


def brewer_set3(n):
    return color_ramp(BREWER_SET3, n)


def color_palette(steps, between, n):
    full = [_to_hex(_channels(steps[0]))]
    for i in range(len(between)):
        a, b = _channels(steps[i]), _channels(steps[i + 1])
        for t in range(1, between[i] + 1):
            full.append(_to_hex([int(math.floor(a[c] + t * ((b[c] - a[c]) / (between[i] + 1)) + 0.5)) for c in range(3)]))
        full.append(_to_hex(b))
    return color_ramp(full, n)


# ---------------------------------------------------------------- trees and orders
def cutree_k(merge, k):
    """cutree(k): replay the first n - k merges on explicit member sets; number the groups by first appearance."""
    n = len(merge) + 1
    ident = [-(i + 1) for i in range(n)]        # the cluster every cell is in, as merge names it: -(i + 1), then the step
    for step in range(n - k):
        a, b = int(merge[step][0]), int(merge[step][1])
        for c in range(n):
            if ident[c] == a or ident[c] == b:
                ident[c] = step + 1
    seen, out = [], []
    for c in range(n):
        if ident[c] not in seen:
            seen.append(ident[c])
        out.append(seen.index(ident[c]) + 1)
    return np.array(out, dtype=np.int64)


def tree_order(x_cg, cells, method):
    """(merge, the cells in hclust order) of hclust(dist(rows `cells` of x_cg), method)."""
    merge, _, order = hr.hclust(hr.seq_dist(np.asarray(x_cg)[list(cells)]), method)
    return merge, [cells[int(o) - 1] for o in order]


def _stored_order(tree, index_of):
    return [index_of[str(tree.labels[int(o) - 1])] for o in tree.order]


def observation_order(obj, x_cg, obs_cells, group_of, obs_names, by_groups, k, method):
    index_of = {str(s): i for i, s in enumerate(obj.cells())}
    ts = obj.tumor_subclusters
    ordered, split, ann, seps = [], [], [], []
    if ts is not None and by_groups:
        for gi, name in enumerate(obs_names):
            hc, subs = ts["hc"].get(name), ts["subclusters"][name]
            sub_of = {}
            for sname, members in subs.items():
                for c in np.asarray(members).ravel():
                    sub_of[int(c)] = sname
            if hc is None:
                cells = [int(c) for members in subs.values() for c in np.asarray(members).ravel()]
                assert len(cells) in (1, 2)
            elif isinstance(hc, (list, tuple)):
                cells, nxt = [], 0
                for members in subs.values():
                    members = [int(c) for c in np.asarray(members).ravel()]
                    if len(members) >= 2:
                        cells += _stored_order(hc[nxt], index_of)
                        nxt += 1
                    else:
                        cells += members
            else:
                cells = _stored_order(hc, index_of)
            ordered += cells
            split += [sub_of[c] for c in cells]
            ann += [gi + 1] * len(cells)
            seps.append(len(ordered))
        return ordered, split, ann, seps, False
    if ts is not None:
        hc = ts["hc"]["all_observations"]
        ordered = _stored_order(hc, index_of)
        if k > 1:
            cut = cutree_k(hc.merge, k)
            lab = {index_of[str(l)]: int(cut[i]) for i, l in enumerate(hc.labels)}
        else:
            lab = {int(c): sname for sname, members in ts["subclusters"]["all_observations"].items() for c in np.asarray(members).ravel()}
        split = [lab[c] for c in ordered]
    elif by_groups:
        for gi in range(max(group_of.values())):
            cells = [c for c in obs_cells if group_of[c] == gi + 1]
            if len(cells) >= 2:
                cells = tree_order(x_cg, cells, method)[1]
            ordered += cells
            ann += [gi + 1] * len(cells)
            seps.append(len(ordered))
        return ordered, [1] * len(ordered), ann, seps, False
    elif len(obs_cells) > 1:
        merge, ordered = tree_order(x_cg, list(obs_cells), method)
        cut = cutree_k(merge, k)
        lab = {c: int(cut[i]) for i, c in enumerate(obs_cells)}
        split = [lab[c] for c in ordered]
    else:
        return list(obs_cells), [1], [group_of[obs_cells[0]]], [1], False
    uniq = []
    for s in split:
        if s not in uniq:
            uniq.append(s)
    total = 0
    for u in uniq:
        total += split.count(u)
        seps.append(total)
    return ordered, split, [group_of[c] for c in ordered], seps, True


def reference_order(x_cg, ref_groups, cluster, method):
    groups = [[int(c) for c in np.asarray(g).ravel()] for g in ref_groups]
    seps = []
    if len(groups) > 1:
        groups = [tree_order(x_cg, g, method)[1] if (cluster and len(g) > 2) else g for g in groups]
        total = 0
        for g in groups[:-1]:
            total += len(g)
            seps.append(total)
    elif cluster and len(groups[0]) > 1:
        groups = [tree_order(x_cg, groups[0], method)[1]]
    ordered, split = [], []
    for gi, g in enumerate(groups):
        ordered += g
        split += [gi + 1] * len(g)
    return ordered, split, seps


# ---------------------------------------------------------------- write.table
def write_table(path, rows, row_names=None, col_names=None, quote=True, sep=" "):
    def cell(v):
        if isinstance(v, str):
            return '"%s"' % v if quote else v
        return r_num(v)
    lines = []
    if col_names is not None:
        lines.append(sep.join(cell(str(c)) for c in col_names))
    for i, row in enumerate(rows):
        lead = [cell(str(row_names[i]))] if row_names is not None else []
        lines.append(sep.join(lead + [cell(v) for v in row]))
    with open(path, "wb") as f:
        f.write(("\n".join(lines) + "\n").encode())


# ---------------------------------------------------------------- PNG
def png_decode(path):
    """(H, W, 3) uint8 of an 8-bit RGB, non-interlaced PNG; all five filter types."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, W = 8, b"", None
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        if tag == b"IHDR":
            W, H, depth, ctype, _, _, interlace = struct.unpack(">IIBBBBB", body)
            assert (depth, ctype, interlace) == (8, 2, 0)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(H, 1 + 3 * W)
    out = np.zeros((H, 3 * W), dtype=np.uint8)
    for y in range(H):
        f, line = int(raw[y, 0]), raw[y, 1:].astype(np.int64)
        if f == 0:
            out[y] = line
            continue
        up = out[y - 1].astype(np.int64) if y else np.zeros(3 * W, dtype=np.int64)
        cur = np.zeros(3 * W, dtype=np.int64)
        for i in range(3 * W):
            a = cur[i - 3] if i >= 3 else 0
            b = up[i]
            c = up[i - 3] if i >= 3 else 0
            if f == 1:
                pred = a
            elif f == 2:
                pred = b
            elif f == 3:
                pred = (a + b) // 2
            else:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
            cur[i] = (line[i] + pred) & 255
        out[y] = cur
    return out.reshape(H, W, 3)


# ---------------------------------------------------------------- the page
def page_geometry(obs_names, ref_names, nobs, res, dynamic_resize):
    dyn = dynamic_resize * 3.6 * (nobs - 200) / 200 if nobs > 200 else 0
    coln1 = max(1, math.floor(123 / (max(len(s) for s in obs_names) + 6)))
    coln2 = max(1, math.floor(123 / (max(len(s) for s in ref_names) + 6))) if ref_names else 1
    gk = ((math.ceil(len(ref_names) / coln2) + 2) * 0.175, (math.ceil(len(obs_names) / coln1) + 3) * 0.175)
    height = 8.22 + (gk[0] + gk[1]) + dyn
    if height > 32768 / res:
        height = math.floor(((32767 / res) - 5e-3) * 100 + 0.5) / 100
        dyn = height - 8.22 - (gk[0] + gk[1])
    lhei = [1.125, 2.215, .15, .5, .5, .5, .5, .5, .5, .5, .5, .5 + dyn, 0.1, gk[0], gk[1], 0.13]
    lwid = [1.5, 0.2, 0.2, 0.02] + [9 / 12] * 10
    W, H = math.floor(10 * res + 0.5), math.floor(height * res + 0.5)
    ys, xs, acc = [0], [0], 0.0
    for v in lhei:
        acc += v
        ys.append(min(H, math.floor(acc / sum(lhei) * H + 0.5)))
    acc = 0.0
    for v in lwid:
        acc += v
        xs.append(min(W, math.floor(acc / sum(lwid) * W + 0.5)))
    ys[-1], xs[-1] = H, W
    return W, H, xs, ys


def plot_cnv(obj, out_dir, cluster_by_groups=True, cluster_references=True, k_obs_groups=1, x_center=None, x_range="auto",
             hclust_method="ward.D", color_safe_pal=False, output_filename="infercnv", output_format="png", png_res=300,
             dynamic_resize=0, write_expr_matrix=False, title="inferCNV", obs_title="Observations (Cells)",
             ref_title="References (Cells)", contig_cex=1):
    """Writes every text file of the product's plot_cnv into out_dir; returns (RGB page or None, layout dict or None)."""
    os.makedirs(out_dir, exist_ok=True)
    expr = np.asarray(obj.expr_data, dtype=np.float64)
    G, C = expr.shape
    genes, cells = [str(g) for g in obj.genes()], [str(c) for c in obj.cells()]
    if x_center is None:
        x_center = math.fsum(float(v) for v in expr.ravel()) / expr.size
    x_cg = expr.T.copy()
    name = output_filename
    if write_expr_matrix:
        write_table(os.path.join(out_dir, "expr.%s.dat" % name), [list(r) for r in expr], genes, cells, quote=False, sep="\t")
    if x_range is None:
        low, high = float((x_cg + 0.0).min()), float((x_cg + 0.0).max())
    else:
        if isinstance(x_range, str):
            q = quantiles_excluding(x_cg, x_center, (0.01, 0.99))["quantiles"]
            delta = max(abs(x_center - q[0]), abs(q[1] - x_center))
            low, high = float(x_center - delta), float(x_center + delta)
        else:
            low, high = float(x_range[0]), float(x_range[1])
        x_cg = np.where(x_cg < low, low, x_cg)
        x_cg = np.where(x_cg > high, high, x_cg)
    by = (high - low) / 15
    breaks = [low + i * by for i in range(15)] + [high]

    contigs = [str(c) for c in obj.gene_order.chr]
    uniq_contigs = []
    for c in contigs:
        if c not in uniq_contigs:
            uniq_contigs.append(c)
    contig_color = dict(zip(uniq_contigs, brewer_set3(len(uniq_contigs))))
    colors = color_palette(("purple3", "white", "darkorange2") if color_safe_pal else ("darkblue", "white", "darkred"), (2, 2), 15)

    obs_names, ref_names = list(obj.observation_grouped_cell_indices), list(obj.reference_grouped_cell_indices)
    refs = sorted(int(c) for g in obj.reference_grouped_cell_indices.values() for c in np.asarray(g).ravel())
    group_of = {c: -1 for c in range(C)}
    for gi, g in enumerate(obj.observation_grouped_cell_indices.values()):
        for c in np.asarray(g).ravel():
            group_of[int(c)] = gi + 1
    obs_cells = [c for c in range(C) if c not in refs]
    nobs = sum(np.asarray(g).size for g in obj.observation_grouped_cell_indices.values())
    ordered, split, ann, seps, members = observation_order(obj, x_cg, obs_cells, group_of, obs_names, cluster_by_groups,
                                                           k_obs_groups, hclust_method)
    label = lambda s: s if isinstance(s, str) else r_num(s)
    uniq = []
    for s in split:
        if s not in uniq:
            uniq.append(s)
    if members:
        for u in uniq:
            memb = [c for c, s in zip(ordered, split) if s == u]
            path = os.path.join(out_dir, "General_HCL_%s_members.txt" % label(u))
            if len(memb) == 1:
                write_table(path, [[float(v)] for v in x_cg[memb[0]]], genes, ["V1"])
            else:
                write_table(path, [[float(v) for v in x_cg[c]] for c in memb], [cells[c] for c in memb], genes)
    dend_pal, ann_pal = brewer_set3(len(uniq)), brewer_set3(len(set(ann)))
    rows = []
    for s, a in zip(split, ann):
        rows.append([label(s), dend_pal[uniq.index(s)], r_num(a), ann_pal[a - 1] if 1 <= a <= len(ann_pal) else "NA"])
    write_table(os.path.join(out_dir, "%s.observation_groupings.txt" % name), rows, [cells[c] for c in ordered],
                ["Dendrogram Group", "Dendrogram Color", "Annotation Group", "Annotation Color"])
    write_table(os.path.join(out_dir, "%s.heatmap_thresholds.txt" % name), [[b] for b in breaks])
    ref_ordered, ref_split, ref_seps = [], [], []
    if ref_names:
        ref_ordered, ref_split, ref_seps = reference_order(x_cg, list(obj.reference_grouped_cell_indices.values()), cluster_references,
                                                           hclust_method)
    if write_expr_matrix:
        write_table(os.path.join(out_dir, "%s.observations.txt" % name), [[float(x_cg[c, g]) for c in ordered] for g in range(G)], genes,
                    [cells[c] for c in ordered])
        if ref_names:
            write_table(os.path.join(out_dir, "%s.references.txt" % name), [[float(x_cg[c, g]) for c in ref_ordered] for g in range(G)],
                        genes, [cells[c] for c in ref_ordered])
    if output_format != "png":
        return None, None

    W, H, xs, ys = page_geometry(obs_names, ref_names, nobs, png_res, dynamic_resize)
    page = np.full((H, W, 3), 255, dtype=np.uint8)
    rgb = np.array([_channels(c) for c in colors], dtype=np.uint8)
    px0, px1 = xs[4], xs[14]
    pw = px1 - px0
    gene_px = [((2 * j + 1) * G) // (2 * pw) for j in range(pw)]
    layout_groups = {}

    def panel(order_top_down, row_info, boundaries, y0, y1, bars):
        n, h = len(order_top_down), y1 - y0
        cell_px = [((2 * i + 1) * n) // (2 * h) for i in range(h)]
        tile = rgb[raster(x_cg, breaks, order_top_down, h, pw)]
        for j in range(1, pw):
            if contigs[gene_px[j]] != contigs[gene_px[j - 1]]:
                tile[:, j] = 0
        for s in boundaries:
            if 0 < s < n:
                hit = [i for i in range(h) if cell_px[i] >= s]
                if hit:
                    tile[hit[0], :] = 0
        page[y0:y1, px0:px1] = tile
        spans = []
        for i in range(h):
            info = row_info[cell_px[i]]
            for (bx0, bx1), which in bars:
                page[y0 + i, bx0:bx1] = _channels(info[which])
            if spans and spans[-1]["_k"] == info:
                spans[-1]["y1"] = y0 + i + 1
            else:
                spans.append({"_k": info, "name": info[2], "color": info[1], "y0": y0 + i, "y1": y0 + i + 1})
        for s in spans:
            del s["_k"]
        return spans

    n_obs = len(ordered)
    top_down = ordered[::-1]
    obs_info = [(rows[i][1], rows[i][3], obs_names[ann[i] - 1] if 1 <= ann[i] <= len(obs_names) else "NA") for i in range(n_obs)][::-1]
    obs_spans = panel(top_down, obs_info, [n_obs - s for s in seps], ys[3], ys[12], [((xs[1], xs[2]), 0), ((xs[2], xs[3]), 1)])
    ref_spans, ref_counts = [], None
    if ref_names:
        rpal = brewer_set3(len(set(ref_split)))
        ref_info = [("NA", rpal[s - 1], ref_names[s - 1]) for s in ref_split]
        ref_spans = panel(ref_ordered, ref_info, ref_seps, ys[1], ys[2], [((xs[2], xs[3]), 1)])
        ref_counts = [int(v) for v in bins(x_cg, breaks, ref_ordered)]
    contig_spans = []
    for j in range(pw):
        cname = contigs[gene_px[j]]
        page[ys[2]:ys[3], px0 + j] = _channels(contig_color[cname])
        if contig_spans and contig_spans[-1]["name"] == cname:
            contig_spans[-1]["x1"] = px0 + j + 1
        else:
            contig_spans.append({"name": cname, "color": contig_color[cname], "x0": px0 + j, "x1": px0 + j + 1})
    counts = [int(v) for v in bins(x_cg, breaks, ordered)]
    kx0, kx1, ky0, ky1 = xs[0], xs[1], ys[1], ys[2]
    for b in range(15):
        bar = (counts[b] * (ky1 - ky0)) // max(counts) if max(counts) else 0
        page[ky1 - bar:ky1, kx0 + (b * (kx1 - kx0)) // 15:kx0 + ((b + 1) * (kx1 - kx0)) // 15] = rgb[b]
    box = lambda c0, c1, r0, r1: [xs[c0], ys[r0], xs[c1], ys[r1]]
    layout = {"width": W, "height": H, "png_res": png_res, "title": title, "obs_title": obs_title, "ref_title": ref_title,
              "contig_cex": contig_cex,
              "panels": {"observations": box(4, 14, 3, 12), "references": box(4, 14, 1, 2), "contigs": box(4, 14, 2, 3),
                         "observation_dendrogram_colors": box(1, 2, 3, 12), "observation_annotation_colors": box(2, 3, 3, 12),
                         "reference_annotation_colors": box(2, 3, 1, 2), "key": box(0, 1, 1, 2)},
              "contigs": contig_spans, "observation_groups": obs_spans, "reference_groups": ref_spans,
              "breaks": [float(b) for b in breaks], "colors": colors, "counts": counts, "reference_counts": ref_counts}
    return page, layout
