"""Sequential restatement of the four files of generate_cnv_region_reports (R/inferCNV_HMM.R:706-869, 1005-1087; the
formatting rule of include/icnv.h "CNV region reports", DESIGN K24), written the reference's way: cell groups, per group the
consensus state of every gene, per chromosome the runs of equal states with one counter that runs on across groups, then one
text line per region and per gene of a region.  It shares no code with infercnv_amd/cnv_regions.py or the kernels.

Rules taken from the contract, not from R: a chromosome of fewer than two genes yields nothing and does not advance the
counter (:1013); by = "cell" reads a cell's own states, and a state outside 1 .. 6 is the invalid state there; the invalid
state (any negative number, or 255) is written as -1; positions are integers, written in plain decimal."""
import locale

import numpy as np


def cell_groups(obj, by):
    """:713-733 -> [(name, [0-based cell indices])] in report order."""
    if obj.tumor_subclusters is None:
        by = "consensus"
    if by == "consensus":
        merged = dict(obj.reference_grouped_cell_indices)
        merged.update(obj.observation_grouped_cell_indices)
        return [(str(k), [int(i) for i in v]) for k, v in merged.items()]
    if by == "subcluster":
        return [(f"{grp}.{sub}", [int(i) for i in idx]) for grp, subs in obj.tumor_subclusters["subclusters"].items() for sub, idx in subs.items()]
    assert by == "cell"
    cells = obj.cells()
    order = [int(i) for d in (obj.reference_grouped_cell_indices, obj.observation_grouped_cell_indices) for v in d.values() for i in v]
    return [(str(cells[i]), [i]) for i in order]


def group_states(states, idx, by_cell):
    """One integer per gene: the most frequent state of the group's cells, the smallest of equally frequent ones (:977-987);
    by cell the cell's own state, anything outside 1 .. 6 as -1.  A negative state or 255 is -1 throughout."""
    out = []
    for g in range(states.shape[0]):
        vals = [int(states[g, c]) for c in idx]
        vals = [-1 if (v < 0 or v == 255) else v for v in vals]
        if by_cell:
            out.append(vals[0] if 1 <= vals[0] <= 6 else -1)
            continue
        best, best_n = None, 0
        for v in sorted(set(vals), key=lambda v: 255 if v == -1 else v):      # the library orders the invalid state last
            if vals.count(v) > best_n:
                best, best_n = v, vals.count(v)
        out.append(best)
    return out


def regions_of(vec, chrs, counter):
    """:1005-1057 -> [(chr, ordinal, state, [gene indices])], counter."""
    out = []
    for c in dict.fromkeys(chrs):
        genes = [i for i, cc in enumerate(chrs) if cc == c]
        if len(genes) < 2:
            continue
        for k, i in enumerate(genes):
            if k == 0 or vec[i] != vec[genes[k - 1]]:
                counter += 1
                out.append((c, counter, vec[i], []))
            out[-1][3].append(i)
    return out, counter


def report_lines(obj, by, ignore_neutral_state=None):
    """(lines of pred_cnv_regions.dat, lines of pred_cnv_genes.dat) without the headers: two lists with one entry per written
    region; the genes entry is the list of that region's lines."""
    states = np.asarray(obj.expr_data)
    chrs = [str(c) for c in obj.gene_order.chr]
    genes = [str(g) for g in obj.genes()]
    n = len(chrs)
    start = [int(v) for v in (obj.gene_order.start if obj.gene_order.start is not None else range(n))]
    stop = [int(v) for v in (obj.gene_order.stop if obj.gene_order.stop is not None else range(n))]
    by_cell = by == "cell" and obj.tumor_subclusters is not None
    counter, region_lines, gene_lines = 0, [], []
    for name, idx in cell_groups(obj, by):
        regs, counter = regions_of(group_states(states, idx, by_cell), chrs, counter)
        for c, ordinal, state, rows in regs:
            if ignore_neutral_state is not None and state == ignore_neutral_state:
                continue
            rn = f"{c}-region_{ordinal}"
            region_lines.append("\t".join([name, rn, str(state), c, str(min(start[r] for r in rows)), str(max(stop[r] for r in rows))]) + "\n")
            gene_lines.append(["\t".join([name, rn, str(state), genes[r], c, str(start[r]), str(stop[r])]) + "\n" for r in rows])
    return region_lines, gene_lines


def report_files(obj, by, ignore_neutral_state=None):
    """{suffix: bytes} of the four files."""
    enc = locale.getpreferredencoding(False)
    region_lines, gene_lines = report_lines(obj, by, ignore_neutral_state)
    cells = obj.cells()
    chrs = [str(c) for c in obj.gene_order.chr]
    n = len(chrs)
    start = [int(v) for v in (obj.gene_order.start if obj.gene_order.start is not None else range(n))]
    stop = [int(v) for v in (obj.gene_order.stop if obj.gene_order.stop is not None else range(n))]
    groupings = "cell_group_name\tcell\n" + "".join(f"{name}\t{cells[i]}\n" for name, idx in cell_groups(obj, by) for i in idx)
    used = "chr\tstart\tstop\n" + "".join(f"{g}\t{c}\t{a}\t{b}\n" for g, c, a, b in zip(obj.genes(), chrs, start, stop))
    return {".cell_groupings": groupings.encode(enc),
            ".pred_cnv_regions.dat": ("cell_group_name\tcnv_name\tstate\tchr\tstart\tend\n" + "".join(region_lines)).encode(enc),
            ".pred_cnv_genes.dat": ("cell_group_name\tgene_region_name\tstate\tgene\tchr\tstart\tend\n" +
                                    "".join(l for ls in gene_lines for l in ls)).encode(enc),
            ".genes_used.dat": used.encode(enc)}


SUFFIXES = (".cell_groupings", ".pred_cnv_regions.dat", ".pred_cnv_genes.dat", ".genes_used.dat")


def read_files(out_dir, prefix):
    import os
    return {s: open(os.path.join(str(out_dir), prefix + s), "rb").read() for s in SUFFIXES}


# ------------------------------------------------------------------ the objects of the tests
def make_object(states, chrs, start, stop, ref, obs, subclusters, gene_names=None, cell_names=None):
    from infercnv_amd.infercnv_object import GeneOrder, InfercnvObject
    states = np.asarray(states)
    G, C = states.shape
    return InfercnvObject(expr_data=states.astype(np.float64), gene_order=GeneOrder(chr=np.asarray(chrs), start=np.asarray(start), stop=np.asarray(stop)),
                          reference_grouped_cell_indices={k: np.asarray(v, dtype=np.int32) for k, v in ref.items()},
                          observation_grouped_cell_indices={k: np.asarray(v, dtype=np.int32) for k, v in obs.items()},
                          tumor_subclusters=None if subclusters is None else {"subclusters": {g: {s: np.asarray(v, dtype=np.int32) for s, v in d.items()}
                                                                                                for g, d in subclusters.items()}},
                          gene_names=np.asarray(gene_names if gene_names is not None else [f"g{i}" for i in range(G)], dtype=object),
                          cell_names=np.asarray(cell_names if cell_names is not None else [f"c{i}" for i in range(C)], dtype=object))


EDGE_CHR_SIZES = (1, 2, 17, 17)            # the one-gene chromosome yields nothing and does not advance the counter


def edge_object(seed=3, all_neutral=False, odd_bytes=False):
    """37 genes on chromosomes of 1, 2, 17 and 17 genes; 12 cells in 1 reference and 2 observation groups with 3 subclusters;
    a run of one gene; odd_bytes puts the bytes 0, 7 and 255 (as -1) into single cells."""
    rng = np.random.default_rng(seed)
    G, C = sum(EDGE_CHR_SIZES), 12
    chrs = np.concatenate([np.full(n, f"chr{k + 1}") for k, n in enumerate(EDGE_CHR_SIZES)])
    start = np.arange(G) * 1000 + 1
    states = np.full((G, C), 3, dtype=np.int64)
    if not all_neutral:
        states[0, :] = 5                                   # the one-gene chromosome
        states[1:3, 4:8] = 4                               # a whole two-gene chromosome
        states[5:9, 4:12] = 1
        states[10, 2:8] = 6                                # a run of one gene
        states[20:37, 8:12] = 2                            # a run to the last gene
        states[25, rng.integers(0, C, 3)] = 4
        if odd_bytes:
            states[12, 1], states[13, 1], states[14, 5], states[30, 9] = 0, 7, -1, 7
    return make_object(states, chrs, start, start + 500, {"normal": [0, 1, 2, 3]}, {"tumA": [4, 5, 6, 7], "tumB": [8, 9, 10, 11]},
                       {"tumA": {"tumA_s1": [4, 5], "tumA_s2": [6, 7]}, "tumB": {"tumB_s1": [8, 9, 10, 11]}})


WIDTH_POSITIONS = (0, 9, 10, 99999999, 2 ** 31, 10 ** 15, -5)
WIDTH_NAME_BYTES = (1, 15, 16, 17, 255, 300, 5000)


def width_object(seed=11, C=64, G=3000, scramble=False):
    """64 cells x 3 000 genes with many short runs (the ordinals cross 9/10, 99/100 and 999/1000 by cell), positions of every
    width, cell names of 1 .. 5 000 bytes (one with multi-byte UTF-8), a gene name of 3 000 bytes; scramble: a gene order that
    is not contiguous by chromosome.  Smaller C and G keep what fits."""
    rng = np.random.default_rng(seed)
    sizes = (G * 7 // 30, 1, G * 11 // 30, G - 1 - G * 7 // 30 - G * 11 // 30)
    chrs = np.concatenate([np.full(n, f"chr{k + 1}") for k, n in enumerate(sizes)])
    if scramble:
        chrs = chrs[rng.permutation(G)]
    start = rng.integers(1, 10 ** 9, G)
    start[:len(WIDTH_POSITIONS)] = WIDTH_POSITIONS
    stop = start + rng.integers(0, 5000, G)
    stop[40:40 + len(WIDTH_POSITIONS)] = WIDTH_POSITIONS
    states = np.full((G, C), 3, dtype=np.int64)
    for c in range(C):
        for _ in range(12):
            a, n = int(rng.integers(0, G - 8)), int(rng.integers(1, 8))
            states[a:a + n, c] = int(rng.choice([1, 2, 4, 5, 6]))
    cell_names = [f"cell{c}" for c in range(C)]
    for k, nb in enumerate(WIDTH_NAME_BYTES):
        if 3 + 5 * k < C:
            cell_names[3 + 5 * k] = ("x" * nb)[:nb - 1] + str(k)
    long_cell = 3 + 5 * (len(WIDTH_NAME_BYTES) - 1)           # the 5 000-byte name: runs of at most 5 genes, so that a non-neutral
    if long_cell < C:                                         # record of it stays below 64 KiB
        states[:, long_cell] = 3
        for k, a in enumerate((3, sizes[0] - 2, sizes[0] + 2, G // 2, G - 10)):
            states[a:a + 1 + k, long_cell] = (1, 2, 4, 5, 6)[k]
    if C > 50:
        cell_names[50] = "zelle_äö€_50"
    gene_names = [f"gene{g}" for g in range(G)]
    gene_names[G // 2] = "G" * 3000
    ref = list(range(C - 8, C))
    obs = list(range(C - 8))
    cut = len(obs) // 3
    return make_object(states, chrs, start, stop, {"normal": ref}, {"tumor": obs},
                       {"normal": {"normal_s1": ref}, "tumor": {"tumor_s1": obs[:cut], "tumor_s2": obs[cut:]}}, gene_names, cell_names)
