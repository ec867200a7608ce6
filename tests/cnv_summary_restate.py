"""Sequential restatement of .get_features / .get_top_n_regions / the table writer of add_to_seurat
(R/seurat_interaction.R:167-211, 244-445, 463-553), written the reference's way: it works on the two REPORT TABLES
(pred_cnv_regions.dat, pred_cnv_genes.dat) as rows, filters them per cell group (or per cell), takes gene-level windows and
table() order.  It shares no code with infercnv_amd/seurat_interaction.py, which works from the state matrix.

A table is a dict of equally long lists / arrays, one per column of the file.  Ties of table() counts are taken in byte
order of the region name (the library's documented rule; R's own order depends on the locale)."""
import numpy as np

import oracle_np as onp

FEATS3 = ["has_cnv", "has_loss", "has_dupli", "proportion_cnv", "proportion_loss", "proportion_dupli"]
FEATS6 = FEATS3 + ["proportion_scaled_cnv", "proportion_scaled_loss", "proportion_scaled_dupli"]


def uniq(seq):
    return list(dict.fromkeys(seq))


def tables_from_states(states, groups, chrs, gene_names, start, end, ignore_neutral_state):
    """The two report tables of generate_cnv_region_reports(ignore_neutral_state) (R/inferCNV_HMM.R:790-869) for `groups`
    = [(cell group name, column indices)] in report order, from the consensus of each group's columns."""
    regions = {k: [] for k in ("cell_group_name", "cnv_name", "state", "chr", "start", "end")}
    genes = {k: [] for k in ("cell_group_name", "gene_region_name", "state", "gene", "chr", "start", "end")}
    counter = 0
    chrs = [str(c) for c in chrs]
    for name, idx in groups:
        idx = np.asarray(idx, dtype=np.int64)
        cons = states[:, idx[0]] if idx.size == 1 else onp.state_consensus(states, [idx])[:, 0]
        regs, counter = onp.define_cnv_gene_regions(cons, chrs, counter)
        for rn, state, rows in regs:
            if state == ignore_neutral_state:
                continue
            for col, v in zip(regions, (name, rn, int(state), chrs[rows[0]], min(start[r] for r in rows), max(end[r] for r in rows))):
                regions[col].append(v)
            for r in rows:
                for col, v in zip(genes, (name, rn, int(state), gene_names[r], chrs[r], start[r], end[r])):
                    genes[col].append(v)
    return regions, genes


def read_table(path):
    """read.table(sep = "\\t", header = TRUE) of a report: integer columns state / start / end."""
    with open(path) as fh:
        lines = fh.read().splitlines()
    header = lines[0].split("\t")
    tab = {h: [] for h in header}
    for ln in lines[1:]:
        for h, v in zip(header, ln.split("\t")):
            tab[h].append(int(v) if h in ("state", "start", "end") else v)
    return tab


def _arrays(tab):
    return {k: np.asarray(v) if len(v) else np.zeros(0, dtype=(np.int64 if k in ("state", "start", "end") else "<U1")) for k, v in tab.items()}


def sorted_regions(names):
    """sort(table(names), decreasing = TRUE): names in byte order, then a stable sort by decreasing count."""
    count = {}
    for n in names:
        count[n] = count.get(n, 0) + 1
    by_name = sorted(count, key=lambda n: n.encode())
    return [(n, count[n]) for n in sorted(by_name, key=lambda n: -count[n])]


def get_top_n_regions(hmm_genes, sorted_reg, top_n, bp_tolerance):
    """.get_top_n_regions (:463-553), statement by statement.  Returns [{subclust_names, regions_names}]."""
    if len(sorted_reg) < 1:
        return []
    g = _arrays(hmm_genes)
    name, chrom, start, end, group = g["gene_region_name"], g["chr"], g["start"], g["end"], g["cell_group_name"]
    top, used = [], []
    for reg, _ in sorted_reg:
        if reg in used:
            continue
        in_region = np.nonzero(name == reg)[0]
        region_chr = chrom[in_region[0]]
        region_start_low = region_start_high = start[in_region].min()
        region_end_low = region_end_high = end[in_region].max()
        same_chr = np.nonzero((chrom == region_chr) & ~np.isin(name, used))[0]
        initial_close = []
        for _ in range(100000):
            close_start = same_chr[(start[same_chr] <= region_start_high + bp_tolerance) & (start[same_chr] >= region_start_low - bp_tolerance)]
            close_end = same_chr[(end[same_chr] <= region_end_high + bp_tolerance) & (end[same_chr] >= region_end_low - bp_tolerance)]
            in_end = set(name[close_end].tolist())
            close_start_end = [n for n in uniq(name[close_start].tolist()) if n in in_end]
            if set(close_start_end) == set(initial_close):
                break
            initial_close = close_start_end
            starts = [start[name == regi].min() for regi in close_start_end]
            ends = [end[name == regi].max() for regi in close_start_end]
            region_start_low, region_start_high = min(starts), max(starts)
            region_end_low, region_end_high = min(ends), max(ends)
        else:
            raise RuntimeError("no fixed point")
        assert len(close_start_end) > 0, "Did not even find itself, error."
        top.append({"subclust_names": uniq(group[np.isin(name, close_start_end)].tolist()), "regions_names": close_start_end})
        used += close_start_end
        assert len(used) == len(set(used)), "Used the same region twice"
        if len(top) == top_n:
            break
    return top


def get_features(cells, chr_levels, chr_gene_count, subclusters, regions, hmm_genes, center_state, mode, by_cells, top_n,
                 bp_tolerance, scaling_factor=2):
    """.get_features (:244-445).  cells: colnames(expr.data); chr_levels: levels(gene_order$chr); chr_gene_count:
    {level: genes}; subclusters: [(clust, subclust, [member cell names])] in the order of the nested list.  Returns
    ({feature: {level: {cell: value}}}, [top_loss vectors], [top_dupli vectors], lines of top_losses.txt, of top_duplis.txt)."""
    feats = {f: {lv: {c: (False if f.startswith("has") else 0.0) for c in cells} for lv in chr_levels}
             for f in (FEATS6 if mode == "i6" else FEATS3)}
    r, g = _arrays(regions), _arrays(hmm_genes)

    def assign(group_name, members):
        res_chr = r["chr"][r["cell_group_name"] == group_name]
        sel = g["cell_group_name"] == group_name
        gchr, gstate = g["chr"][sel], g["state"][sel]
        if res_chr.size == 0:
            return
        for c in uniq(res_chr.tolist()):
            on_c = gstate[gchr == c]
            for m in members:
                feats["has_cnv"][c][m] = True
                feats["proportion_cnv"][c][m] = len(on_c) / chr_gene_count[c]
                if mode == "i6":
                    feats["proportion_scaled_cnv"][c][m] = float(np.abs(on_c - center_state).sum()) / (chr_gene_count[c] * scaling_factor)
        for what, keep in (("loss", gstate < center_state), ("dupli", gstate > center_state)):
            sub_chr, sub_state = gchr[keep], gstate[keep]
            for c in uniq(sub_chr.tolist()):
                on_c = sub_state[sub_chr == c]
                for m in members:
                    feats["has_" + what][c][m] = True
                    feats["proportion_" + what][c][m] = len(on_c) / chr_gene_count[c]
                    if mode == "i6":
                        feats["proportion_scaled_" + what][c][m] = abs(float((on_c - center_state).sum())) / (chr_gene_count[c] * scaling_factor)

    members_of = {}
    if not by_cells:
        for clust, subclust, members in subclusters:
            members_of[clust + "." + subclust] = members
            assign(clust + "." + subclust, members)
    else:
        for cell in cells:
            assign(cell, [cell])

    tops, files, merged = [], [], []
    for what, keep in (("loss", g["state"] < center_state), ("dupli", g["state"] > center_state)):
        top = get_top_n_regions(hmm_genes, sorted_regions(g["gene_region_name"][keep].tolist()), top_n, bp_tolerance)
        vecs, to_write = [], []
        for i, t in enumerate(top):
            v = {c: False for c in cells}
            for sub in t["subclust_names"]:
                for m in ([sub] if by_cells else members_of[sub]):
                    v[m] = True
                    to_write.append(f"top_{what}_{i + 1};{sub};{m}")
            vecs.append(v)
        tops.append(vecs)
        merged.append([t["regions_names"] for t in top])
        files.append(to_write if to_write else [""])
    return feats, tops[0], tops[1], files[0], files[1], merged


def as_character(v):
    """as.character of a logical-turned-double / double: 15 significant digits; fixed unless scientific is narrower."""
    x = float(np.float64("%.15g" % float(v)))
    if x == int(x):
        return str(int(x))
    fixed = np.format_float_positional(x, trim="-")
    sci = np.format_float_scientific(x, trim="-", exp_digits=2)
    return fixed if len(fixed) <= len(sci) else sci


def table_lines(cells, subcluster_of, chr_levels, feats, top_loss, top_dupli, mode):
    """The file write.table(out_mat, quote = FALSE, sep = "\\t") leaves (:167-211)."""
    header, cols = ["subcluster"], []
    for lv in chr_levels:
        for f in (FEATS6 if mode == "i6" else FEATS3):
            header.append(f + "_" + lv)
            cols.append(feats[f][lv])
    for what, vecs in (("loss", top_loss), ("dupli", top_dupli)):
        for i, v in enumerate(vecs):
            header.append(f"top_{what}_{i + 1}")
            cols.append(v)
    lines = ["\t".join(header)]
    for c in cells:
        sub = subcluster_of.get(c)
        lines.append("\t".join([c, "NA" if sub is None else sub] + [as_character(col[c]) for col in cols]))
    return lines


def run_on_object(obj, states, mode, by_cells, top_n=10, bp_tolerance=2000000, tables=None):
    """Everything above on an InfercnvObject-like `obj` (gene_order, cells(), genes(), tumor_subclusters, grouped indices) and
    a genes x cells state array; tables: (regions, hmm_genes) read from report files instead of built here."""
    s0 = 3 if mode == "i6" else 2
    cells = [str(c) for c in obj.cells()]
    chrs = [str(c) for c in obj.gene_order.chr]
    levels = uniq(chrs)
    count = {lv: chrs.count(lv) for lv in levels}
    subs = []
    for clust, d in obj.tumor_subclusters["subclusters"].items():
        for sub, idx in d.items():
            subs.append((clust, sub, [cells[i] for i in idx]))
    if tables is None:
        if by_cells:
            order = [i for d in (obj.reference_grouped_cell_indices, obj.observation_grouped_cell_indices) for v in d.values() for i in v]
            groups = [(cells[i], [i]) for i in order]
        else:
            groups = [(c + "." + s, [cells.index(m) for m in mem]) for c, s, mem in subs]
        tables = tables_from_states(np.asarray(states), groups, chrs, [str(x) for x in obj.genes()], obj.gene_order.start,
                                    obj.gene_order.stop, s0)
    feats, tl, td, fl, fd, merged = get_features(cells, levels, count, subs, tables[0], tables[1], s0, mode, by_cells, top_n, bp_tolerance)
    sub_of = {}
    for annot in list(obj.reference_grouped_cell_indices) + list(obj.observation_grouped_cell_indices) + ["all_observations"]:
        for sub, idx in obj.tumor_subclusters["subclusters"].get(annot, {}).items():
            for i in idx:
                sub_of[cells[i]] = sub
    return {"feats": feats, "top_loss": tl, "top_dupli": td, "top_losses.txt": fl, "top_duplis.txt": fd, "levels": levels,
            "top_loss_regions": merged[0], "top_dupli_regions": merged[1], "cells": cells, "tables": tables, "lines": table_lines(cells, sub_of, levels, feats, tl, td, mode)}


def assert_equal_to_library(want, got_features, got_lines=None):
    """Bit-equality of the library's get_features output (arrays) with the restatement's (dicts)."""
    cells, levels = want["cells"], want["levels"]
    assert [str(c) for c in got_features["chr_names"]] == levels
    for f, per_level in want["feats"].items():
        for k, lv in enumerate(levels):
            w = np.array([per_level[lv][c] for c in cells])
            g = np.asarray(got_features[f][k])
            if w.dtype == bool:
                assert g.dtype == bool and np.array_equal(g, w), (f, lv)
            else:
                assert g.dtype == np.float64 and np.array_equal(g.view(np.uint64), w.astype(np.float64).view(np.uint64)), (f, lv)
    for what in ("loss", "dupli"):
        w, g = want["top_" + what], got_features["top_" + what]
        assert len(w) == len(g), (what, len(w), len(g))
        for a, b in zip(w, g):
            assert np.array_equal(np.array([a[c] for c in cells]), np.asarray(b)), what
    if got_lines is not None:
        assert got_lines == want["lines"]


def counts_and_runs_np(states, chr_start, s0, order, neutral=None):
    """Plain NumPy stand-in for the device calls: (n_chr, columns, 4) counts of the matrix's columns and the non-neutral run
    records of the columns listed in `order` (neutral: the state left out of the records, default s0; 0: none)."""
    neutral = s0 if neutral is None else neutral
    st = np.asarray(states).astype(np.int64)
    n_chr = len(chr_start) - 1
    counts = np.zeros((n_chr, st.shape[1], 4), dtype=np.int64)
    rec = {k: [] for k in ("col", "chr", "gene_first", "gene_last", "state", "ordinal")}
    for k in range(n_chr):
        a, b = chr_start[k], chr_start[k + 1]
        if b - a < 2:
            continue
        s = st[a:b]
        counts[k, :, 0], counts[k, :, 1] = (s < s0).sum(0), (s > s0).sum(0)
        counts[k, :, 2], counts[k, :, 3] = np.where(s < s0, s0 - s, 0).sum(0), np.where(s > s0, s - s0, 0).sum(0)
    counter = 0
    for pos, c in enumerate(order):
        for k in range(n_chr):
            a, b = chr_start[k], chr_start[k + 1]
            if b - a < 2:
                continue
            s = st[a:b, c]
            cuts = np.concatenate([[0], np.nonzero(s[1:] != s[:-1])[0] + 1, [b - a]])
            for u, v in zip(cuts[:-1], cuts[1:]):
                counter += 1
                if neutral == 0 or s[u] != neutral:       # neutral = 0: no state is left out, a byte 0 included
                    for key, val in zip(rec, (pos, k, a + u, a + v - 1, s[u], counter)):
                        rec[key].append(int(val))
    return counts, {k: np.array(v, dtype=np.int64) for k, v in rec.items()}


def synthetic_object(n_cells, n_sub, seed, mode="i6", chr_sizes=(300, 1, 260, 240, 199)):
    """An object for the by-cell and subcluster cases: genes 500 kb apart, per subcluster 3 random runs of 20-60 genes whose
    starts are multiples of 4 genes (so runs of different subclusters often lie within the 2 Mb tolerance of each other), a
    one-gene chromosome with a non-neutral state, reference cells in the LAST columns, two cells in no subcluster."""
    from infercnv_amd.infercnv_object import GeneOrder, InfercnvObject
    rng = np.random.default_rng(seed)
    K, s0 = (6, 3) if mode == "i6" else (3, 2)
    G = int(sum(chr_sizes))
    chrs = np.concatenate([np.full(n, f"chr{k + 1}") for k, n in enumerate(chr_sizes)])
    pos = np.concatenate([np.arange(n) * 500000 + 1 for n in chr_sizes])
    states = np.full((G, n_cells), s0, dtype=np.int8)
    n_ref = max(n_cells // 10, 1)
    obs, ref = np.arange(n_cells - n_ref), np.arange(n_cells - n_ref, n_cells)
    member = rng.permutation(obs[:-2]) if obs.size > 4 else obs
    parts = np.array_split(member, n_sub)
    subs = {"tumor": {f"tumor_s{q + 1}": np.sort(p).astype(np.int32) for q, p in enumerate(parts)}, "normal": {"normal_s1": ref.astype(np.int32)}}
    other = [k for k in range(1, K + 1) if k != s0]
    for p in parts:
        for _ in range(3):
            n = int(rng.integers(20, 61))
            a = int(rng.integers(0, (G - n) // 4)) * 4
            states[a:a + n, p] = rng.choice(other)
    states[chr_sizes[0], obs[: obs.size // 2]] = other[0]                # the one-gene chromosome
    obj = InfercnvObject(expr_data=states.astype(np.float64), gene_order=GeneOrder(chr=chrs, start=pos, stop=pos + 1000),
                         reference_grouped_cell_indices={"normal": ref.astype(np.int32)},
                         observation_grouped_cell_indices={"tumor": obs.astype(np.int32)}, tumor_subclusters={"subclusters": subs},
                         gene_names=np.array([f"g{i}" for i in range(G)]), cell_names=np.array([f"c{i}" for i in range(n_cells)]))
    return obj, states
