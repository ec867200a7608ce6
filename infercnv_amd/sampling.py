"""sample_object and plot_per_group (R/infercnv_sampling.R): groups down- or up-sampled to one height, and one heat map per
group on a common colour scale.

`sample_plan` is the pure part: per group, the source cell of every output column, the new names and the new tree.
`sample_object` assembles the matrix from it -- NumPy for a host object, device.gather_matrix when it is handed the matrix on
the device.  `plot_per_group` uploads the matrix once, takes the centre (device.matrix_mean, DESIGN K23) and the range
(device.quantiles_excluding) from that copy and gathers every group's matrix from it.

Random draws.  R's sample() is unseeded.  Here a draw of `size` out of a vector v is v[gen.permutation(len(v))[:size]] with
gen = numpy.random.Generator(numpy.random.Philox(key=[seed, fnv1a64("sample_object/" + group_name)])): one fresh generator
per group, so a group's draw depends on the seed and its name only.

Trees.  There is no ape here: pruned and grown trees come from tumor_subclusters.prune_hclust / expand_hclust, whose stated
contracts are believed, not verified, to match as.hclust(drop.tip(as.phylo(hc), ...)) and the Newick gsub route.  A Leiden
group's `hc` is, in this library, the list of its partitions' trees (one per partition of two or more cells, in subcluster
order); its leaf order is the concatenation plot_cnv uses; each tree is pruned or grown by itself and a partition left
without a tree becomes None in the list.
"""
from __future__ import annotations

import math
import re
from dataclasses import dataclass, field

import numpy as np

from .infercnv_object import InfercnvObject
from .tumor_subclusters import HClust, expand_hclust, fnv1a64, prune_hclust


def make_filename(text):
    """make_filename (R/infercnv_sampling.R:663-665): gsub("[/\\\\:*?\\"<>|]", "_", text)."""
    return re.sub(r'[/\\:*?"<>|]', "_", str(text))


def _generator(seed, group_name):
    return np.random.Generator(np.random.Philox(key=[int(seed), fnv1a64("sample_object/" + str(group_name))]))


def _draw(seed, group_name, v, size):
    v = np.asarray(v, dtype=np.int64)
    return v[_generator(seed, group_name).permutation(v.size)[:int(size)]]


@dataclass
class SamplePlan:
    """What sample_object builds, without the matrix.  source[j]: the cell of the input object that output column j copies;
    cell_names[j]: its new name; the group dicts and tumor_subclusters index the output columns (0-based)."""
    source: np.ndarray
    cell_names: np.ndarray
    reference_grouped_cell_indices: dict = field(default_factory=dict)
    observation_grouped_cell_indices: dict = field(default_factory=dict)
    tumor_subclusters: dict = field(default_factory=dict)


def _check_args(n_cells, every_n, above_m):
    """R/infercnv_sampling.R:59-85.  Returns (do_every_n, n_cells)."""
    if every_n is not None and above_m is not None:
        if every_n < 2:
            raise ValueError("every_n < 2")
        if math.floor(every_n) != every_n:
            raise ValueError("every_n not an integer")
        if isinstance(above_m, bool) or not isinstance(above_m, (int, float, np.integer, np.floating)):
            raise ValueError("above_m not numeric")
        return True, None
    # (only one of every_n / above_m: R logs a hint and goes on with n_cells)
    if n_cells is None or n_cells < 1 or math.floor(n_cells) != n_cells:
        raise ValueError("invalid n_cells")
    return False, int(n_cells)


def _trees_of(hc):
    return [hc] if isinstance(hc, HClust) else [t for t in hc if t is not None]


def _leaf_order(hc, subs, names, index_of, group_name, line):
    """The cells of a group as its stored tree(s) order them (one tree: labels[order]; a list: plot_cnv's concatenation)."""
    if isinstance(hc, HClust):
        labels = [str(l) for l in np.asarray(hc.labels)[np.asarray(hc.order, dtype=np.int64) - 1]]
    else:
        trees, labels = list(hc), []
        for cells in (subs or {}).values():
            cells = [int(c) for c in np.asarray(cells).ravel()]
            if len(cells) >= 2:
                if not trees or trees[0] is None:
                    raise ValueError(f"sample_object: group {group_name!r} has a partition of {len(cells)} cells without a tree "
                                     f"(R/infercnv_sampling.R:{line})")
                t = trees.pop(0)
                labels += [str(l) for l in np.asarray(t.labels)[np.asarray(t.order, dtype=np.int64) - 1]]
            else:
                labels += [names[c] for c in cells]
    missing = [l for l in labels if l not in index_of]
    if missing:
        raise ValueError(f"sample_object: the tree of group {group_name!r} has the leaf {missing[0]!r}, which is not a cell of the "
                         f"object: match() gives NA (R/infercnv_sampling.R:{line})")
    return [index_of[l] for l in labels]


def _map_trees(hc, fn):
    """fn over the tree, or over every tree of a Leiden list."""
    if isinstance(hc, HClust):
        return fn(hc)
    return [None if t is None else fn(t) for t in hc]


def _every_n_cells(name, cells, hc, subs, length, every_n, names, index_of, line):
    """The every_n selection (:153-163, :273-282): every every_n-th leaf of the tree order, then the first cell of every
    subcluster that none of them represents."""
    if not isinstance(hc, (HClust, list, tuple)):
        raise ValueError(f"sample_object: every_n needs tumor_subclusters$hc[[{name!r}]], the tree of the group under its own name; "
                         f"R reads NULL$labels there and samples nothing (R/infercnv_sampling.R:{line})")
    order = _leaf_order(hc, subs, names, index_of, name, line)
    if length < 1:
        raise ValueError(f"sample_object: group {name!r} has no subclusters: seq(1, 0, every_n) stops (R/infercnv_sampling.R:{line - 2})")
    if len(order) != length:
        raise ValueError(f"sample_object: the tree of group {name!r} has {len(order)} leaves for {length} cells: R indexes past it "
                         f"and match() gives NA (R/infercnv_sampling.R:{line})")
    sampled = order[::int(every_n)]
    chosen = set(sampled)
    for sub_cells in (subs or {}).values():
        sub_cells = [int(c) for c in np.asarray(sub_cells).ravel()]
        if sub_cells and not chosen.intersection(sub_cells):
            sampled.append(sub_cells[0])
            chosen.add(sub_cells[0])
    return np.asarray(sampled, dtype=np.int64)


def _caterpillar(label, n_copies):
    """The hand-made tree of a one-cell group (:232-240, :386-394): merge (-1, -2), (1, -3), ... at height 1."""
    merge = np.array([[-1, -2]] + [[k, -(k + 2)] for k in range(1, n_copies - 1)], dtype=np.int32)
    return HClust(merge, np.ones(n_copies - 1), np.arange(1, n_copies + 1, dtype=np.int32),
                  np.array([f"{label}_{j}" for j in range(1, n_copies + 1)]), "hand-made")


def sample_plan(infercnv_obj: InfercnvObject, n_cells=100, every_n=None, above_m=None, on_references=True, on_observations=True, *,
                seed=0) -> SamplePlan:
    """The plan of sample_object (which see for the behaviour and the errors): everything but the matrix."""
    do_every_n, n_cells = _check_args(n_cells, every_n, above_m)
    obj = infercnv_obj
    names = [str(c) for c in obj.cells()]
    index_of = {}
    for i, s in enumerate(names):
        index_of.setdefault(s, i)                 # match(): the first of equal names
    ts = obj.tumor_subclusters or {}
    old_hc, old_subs = ts.get("hc") or {}, ts.get("subclusters") or {}
    new_hc, new_subs = dict(old_hc), {}
    source, new_names = [], []
    ref_idx, obs_idx = {}, {}

    def copy_through(name, cells, into):
        start = len(source)
        source.extend(cells.tolist())
        new_names.extend(names[c] for c in cells)
        into[name] = np.arange(start, start + cells.size, dtype=np.int64)
        if name in old_subs:                      # (R copies the indices as they are; here they follow the cells)
            where = {int(c): start + k for k, c in enumerate(cells)}
            new_subs[name] = {s: np.array([where[int(c)] for c in np.asarray(v).ravel()], dtype=np.int64) for s, v in old_subs[name].items()}

    def process(name, cells, into, is_ref):
        n = cells.size
        hc, subs = old_hc.get(name), old_subs.get(name)
        line = 155 if is_ref else 274
        if do_every_n or n >= n_cells:            # down-sample
            if not do_every_n:
                sampled = _draw(seed, name, cells, n_cells)
            elif n > above_m:
                length = sum(np.asarray(v).size for v in (subs or {}).values()) if is_ref else n
                sampled = _every_n_cells(name, cells, hc, subs, length, every_n, names, index_of, line)
            else:
                sampled = cells
            out_names = [names[c] for c in sampled]
            if hc is not None:                    # (R prunes observation trees only, :141; a reference tree is pruned alike here)
                kept = {names[c] for c in sampled}
                pruned = _map_trees(hc, lambda t: prune_hclust(t, np.array([str(l) in kept for l in t.labels], dtype=bool)))
                if pruned is None:
                    new_hc.pop(name, None)
                else:
                    new_hc[name] = pruned
            n_out = len(sampled)
        else:                                     # up-sample
            n_copies, to_sample = n_cells // n, n_cells % n
            pre = _draw(seed, name, np.arange(n), to_sample)
            copies = np.full(n, n_copies, dtype=np.int64)
            copies[pre] += 1
            if hc is not None:
                position = {names[c]: k for k, c in enumerate(cells)}
                for t in _trees_of(hc):
                    for l in t.labels:
                        if str(l) not in position:
                            raise ValueError(f"sample_object: the tree of group {name!r} has the leaf {str(l)!r}, which is not a cell of "
                                             f"the group (R/infercnv_sampling.R:{182 if is_ref else 316})")
                if is_ref:
                    sampled = cells[np.repeat(np.arange(n), copies)]          # sort(c(pre, rep(seq, n_copies)))
                    out_names = [f"{names[c]}_{j + 1}" for j, c in enumerate(sampled)]

                    def grow(t):
                        cp = np.array([copies[position[str(l)]] for l in t.labels])
                        g = expand_hclust(t, cp, t.labels)
                        single = np.repeat(cp == 1, cp)                        # (no "_1" on the reference route, :204-213)
                        g.labels = np.array([str(b) if s else l for l, s, b in zip(g.labels, single, np.repeat(np.asarray(t.labels), cp))])
                        return g
                else:
                    order = _leaf_order(hc, subs, names, index_of, name, 316)
                    if sorted(order) != sorted(cells.tolist()):
                        raise ValueError(f"sample_object: the tree of group {name!r} does not hold the group's {n} cells: R fills "
                                         f"n_cells columns from it (R/infercnv_sampling.R:370)")
                    sampled = np.array([c for c in order for _ in range(copies[position[names[c]]])], dtype=np.int64)
                    out_names = [f"{names[c]}_{j}" for c in order for j in range(1, copies[position[names[c]]] + 1)]
                    grow = lambda t: expand_hclust(t, np.array([copies[position[str(l)]] for l in t.labels]), t.labels)
                new_hc[name] = _map_trees(hc, grow)
            else:
                if subs is not None and len(subs) > 1:
                    raise ValueError("Missing clustering information")
                if n != 1:
                    raise ValueError(f"sample_object: group {name!r} has {n} cells and no tree: R repeats every cell of its subcluster "
                                     f"n_cells times into n_cells columns (R/infercnv_sampling.R:{225 if is_ref else 395})")
                sampled = np.repeat(cells, n_cells)
                out_names = [f"{names[cells[0]]}_{j}" for j in range(1, n_cells + 1)]
                new_hc[name] = _caterpillar(names[cells[0]], n_copies)
            n_out = n_cells                       # (R's stale sampled_indices at :403-405 has this length whenever R goes on)
        start = len(source)
        source.extend(int(c) for c in sampled)
        new_names.extend(out_names)
        into[name] = np.arange(start, start + n_out, dtype=np.int64)
        new_subs[name] = {f"{name}_s1": np.arange(start, start + n_out, dtype=np.int64)}

    for groups, into, on, is_ref in ((obj.reference_grouped_cell_indices, ref_idx, on_references, True),
                                     (obj.observation_grouped_cell_indices, obs_idx, on_observations, False)):
        for name, cells in groups.items():
            cells = np.asarray(cells, dtype=np.int64).ravel()
            if on:
                if cells.size < 1:
                    raise ValueError(f"sample_object: group {name!r} is empty: sample() and n_cells % 0 stop (R/infercnv_sampling.R:150)")
                process(name, cells, into, is_ref)
            else:
                copy_through(name, cells, into)
    new_ts = dict(ts, hc=new_hc, subclusters=new_subs)
    return SamplePlan(np.asarray(source, dtype=np.int64), np.asarray(new_names, dtype=object).astype(str) if new_names else np.zeros(0, dtype=str),
                      ref_idx, obs_idx, new_ts)


def _object_from_plan(infercnv_obj, plan, expr_data):
    return InfercnvObject(expr_data=expr_data, gene_order=infercnv_obj.gene_order,
                          reference_grouped_cell_indices=plan.reference_grouped_cell_indices,
                          observation_grouped_cell_indices=plan.observation_grouped_cell_indices, count_data=None,
                          tumor_subclusters=plan.tumor_subclusters, options={}, hspike=infercnv_obj.hspike,
                          gene_names=infercnv_obj.gene_names if infercnv_obj.gene_names is not None else np.asarray(infercnv_obj.genes()),
                          cell_names=plan.cell_names)


def sample_object(infercnv_obj: InfercnvObject, n_cells=100, every_n=None, above_m=None, on_references=True, on_observations=True, *,
                  seed=0, x_dev=None, return_device=False):
    """sample_object (R/infercnv_sampling.R:52-426): every processed group down-sampled (size >= n_cells) or up-sampled (size <
    n_cells) to n_cells cells, or, with every_n and above_m both set, thinned to every every_n-th cell of its tree order when
    it has more than above_m cells (plus the first cell of every subcluster left unrepresented).  Indices are 0-based.

    Kept from R: the argument checks (ValueError with R's stop() texts: "every_n < 2", "every_n not an integer", "above_m not
    numeric", "invalid n_cells"; only one of every_n / above_m falls through to n_cells); reference up-sampling in
    sort(c(pre, rep(seq, n_copies))) order with names `<cell>_<position>`; observation up-sampling in tree order with names
    `<cell>_<copy>`; the hand-made caterpillar at height 1 for a one-cell group; every processed group as one subcluster
    `<name>_s1`; untouched groups copied through; count_data empty (None); gene_order and hspike carried over; R's stale
    length at :403-405 is n_cells.

    Deviations: a down-sampled reference group's tree is pruned like an observation group's (R leaves the tree over cells
    that are no longer in the object, its comment at :141); the subcluster indices of a group that is copied through follow
    its cells to their new columns (R copies the old numbers); n_cells must be a whole number.

    ValueError where R stops or reads what cannot exist (the R line is named in the message):
      - every_n on a group whose tree is not stored under its own name in tumor_subclusters$hc (:155, :274) -- plot_per_group's
        per-group objects are such: their tree is under "all_observations";
      - every_n on a reference group without subclusters (:153), or whose tree has another number of leaves than the group has
        cells (:155, :274);
      - a tree leaf that is not a cell of the object / the group (:156, :182, :316), an observation tree that does not hold the
        group's cells (:370), a Leiden partition of two or more cells without a tree;
      - up-sampling a group without a tree that has more than one subcluster ("Missing clustering information", :218, :374) or
        more than one cell (:225, :395);
      - an empty group (:150).

    seed: the draws' first key word (module docstring).  x_dev: the object's matrix as a (C, G) CUDA float64 tensor; the new
    matrix is then a device.gather_matrix of it (bit for bit the host assembly), and with return_device the pair (object
    with expr_data None, new device matrix) is returned instead of an object with a host matrix."""
    plan = sample_plan(infercnv_obj, n_cells, every_n, above_m, on_references, on_observations, seed=seed)
    if x_dev is None:
        if return_device:
            raise ValueError("return_device needs x_dev")
        expr = np.asarray(infercnv_obj.expr_data)[:, plan.source]
        return _object_from_plan(infercnv_obj, plan, expr)
    from . import device
    new_dev = device.gather_matrix(x_dev, cells=plan.source)
    if return_device:
        return _object_from_plan(infercnv_obj, plan, None), new_dev
    return _object_from_plan(infercnv_obj, plan, np.ascontiguousarray(new_dev.cpu().numpy().T))


# ------------------------------------------------------------------ plot_per_group
def per_group_object(infercnv_obj: InfercnvObject, name, cells, expr_data=None) -> InfercnvObject:
    """The object plot_per_group makes of one group (R/infercnv_sampling.R:528-555, :598-621): the group is the only
    observation group; its tree and subclusters are re-keyed under "all_observations", the subcluster indices as positions
    within the group (match)."""
    cells = np.asarray(cells, dtype=np.int64).ravel()
    ts = infercnv_obj.tumor_subclusters
    new_ts = None
    if ts is not None:
        hc, subs = (ts.get("hc") or {}).get(name), (ts.get("subclusters") or {}).get(name) or {}
        position = {}
        for k, c in enumerate(cells):
            position.setdefault(int(c), k)
        for s, v in subs.items():
            for c in np.asarray(v).ravel():
                if int(c) not in position:
                    raise ValueError(f"plot_per_group: cell {int(c)} of subcluster {s!r} is not in group {name!r}: match() gives NA "
                                     f"(R/infercnv_sampling.R:550)")
        new_ts = {"hc": {} if hc is None else {"all_observations": hc},
                  "subclusters": {"all_observations": {s: np.array([position[int(c)] for c in np.asarray(v).ravel()], dtype=np.int64)
                                                       for s, v in subs.items()}} if subs else {}}
    return InfercnvObject(expr_data=expr_data, gene_order=infercnv_obj.gene_order, reference_grouped_cell_indices={},
                          observation_grouped_cell_indices={name: np.arange(cells.size, dtype=np.int64)}, count_data=None,
                          tumor_subclusters=new_ts, options={}, hspike=infercnv_obj.hspike,
                          gene_names=np.asarray(infercnv_obj.genes()), cell_names=np.asarray(infercnv_obj.cells())[cells])


def _check_sampled_tree(obj, name):
    """After sample_object, plot_cnv(cluster_by_groups = FALSE) reads hc$all_observations: sample_object stores the group's new
    tree under the group's name and leaves that one as it was."""
    ts = obj.tumor_subclusters or {}
    hc = (ts.get("hc") or {}).get("all_observations")
    have = set(str(c) for c in obj.cells())
    if not isinstance(hc, HClust) or any(str(l) not in have for l in hc.labels) or "all_observations" not in (ts.get("subclusters") or {}):
        raise ValueError(f"plot_per_group: group {name!r} was sampled, and sample_object leaves no tree and no subclusters of the "
                         f"sampled cells under 'all_observations': plot_cnv(cluster_by_groups = FALSE) stops there "
                         f"(R/inferCNV_heatmap.R:643-656)")


def plot_per_group(infercnv_obj: InfercnvObject, on_references=True, on_observations=True, sample=False, n_cells=1000, every_n=None,
                   above_m=1000, k_obs_groups=1, base_filename="infercnv_per_group", output_format="png", write_expr_matrix=True,
                   save_objects=False, png_res=300, dynamic_resize=0, useRaster=True, out_dir=None, *, seed=0):
    """plot_per_group (R/infercnv_sampling.R:505-661): one plot_cnv per reference group, then per observation group, all on
    the colour scale of the whole matrix: x.center = mean(expr.data) (device.matrix_mean, DESIGN K23), x.range = its 1 % and
    99 % quantiles over the values that differ from the centre, as the pair it is.  The matrix is uploaded once; the centre,
    the range and every group's matrix (device.gather_matrix) come from that copy.  Each group is drawn as R draws it: title
    "inferCNV <name>", obs_title <name>, ref_title "", cluster_by_groups = FALSE, cluster_references = FALSE, contig_cex = 1,
    color_safe_pal = FALSE, files `<base_filename>_REF_<make_filename(name)>` / `_OBS_`.  output_format None is R's NA; "pdf"
    raises from plot_cnv.

    sample: a group of more than above_m cells goes through sample_object(..., on_references = FALSE) first.  As in R, that
    cannot be drawn afterwards: sample_object files the group's tree under the group's name, plot_cnv(cluster_by_groups =
    FALSE) reads "all_observations" (and every_n stops inside sample_object for the same reason).  ValueError at that group,
    with the files of the groups before it written, as R leaves them.

    save_objects = True (nothing is serialised here: NotImplementedError) and out_dir = None (ValueError) are refused before
    anything is written.  seed: sample_object's."""
    import torch
    from . import device
    from .heatmap import _plot_cnv
    if save_objects:
        raise NotImplementedError("save_objects = TRUE: saveRDS has no counterpart here")
    if out_dir is None:
        raise ValueError('argument "out_dir" is missing, with no default')
    obj = infercnv_obj
    x = torch.from_numpy(np.ascontiguousarray(np.asarray(obj.expr_data, dtype=np.float64).T)).cuda()
    plot_center = device.matrix_mean(x)
    q = device.quantiles_excluding(x, plot_center, (0.01, 0.99))["quantiles"]
    plot_range = (float(q[0]), float(q[1]))
    for groups, on, tag in ((obj.reference_grouped_cell_indices, on_references, "REF"),
                            (obj.observation_grouped_cell_indices, on_observations, "OBS")):
        if not on:
            continue
        for name, cells in groups.items():
            cells = np.asarray(cells, dtype=np.int64).ravel()
            new_obj = per_group_object(obj, name, cells)
            x_group = device.gather_matrix(x, cells=cells)
            if sample and above_m is not None and cells.size > above_m:
                new_obj, x_group = sample_object(new_obj, n_cells=n_cells, every_n=every_n, above_m=above_m, on_references=False,
                                                 on_observations=True, seed=seed, x_dev=x_group, return_device=True)
                _check_sampled_tree(new_obj, name)
            _plot_cnv(new_obj, x_group, out_dir, f"inferCNV {name}", name, "", False, False, False, None, k_obs_groups, 1, plot_center,
                      plot_range, "ward.D", None, False, f"{base_filename}_{tag}_{make_filename(name)}", output_format, png_res,
                      dynamic_resize, None, write_expr_matrix, False, useRaster)
