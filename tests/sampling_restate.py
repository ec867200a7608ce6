"""Sequential restatement of K23 and of the sampling / per-group plotting mirrors, written from R/infercnv_sampling.R,
R/inferCNV_tumor_subclusters.R:336-361 and the contracts in include/icnv.h and the docstrings -- not from the library's code.

  exact_sum            the exact real sum of doubles, rounded once (fractions.Fraction and one float())
  prune_tree           the induced subtree on kept leaves, by recursion over the nested tree
  expand_tree          leaves replaced by zero-height caterpillars
  sample_plan          sample_object without the matrix; written with R's 1-based indices and converted at the end
  per_group_objects    the objects plot_per_group draws
  subcluster_object    the object plot_subclusters draws

Trees are plain dicts {"merge": [[a, b], ...], "height": [...], "order": [...], "labels": [...]} with R's 1-based numbers.
"""
import math
from fractions import Fraction

import numpy as np


# ------------------------------------------------------------------ exact sum
def exact_sum(values):
    vals = [float(v) for v in np.asarray(values, dtype=np.float64).ravel()]
    if any(v != v for v in vals):
        return float("nan")
    pos, neg = any(v == math.inf for v in vals), any(v == -math.inf for v in vals)
    if pos and neg:
        return float("nan")
    if pos or neg:
        return math.inf if pos else -math.inf
    units = 0                                 # every double is a whole number of 2^-1074
    for v in vals:
        num, den = v.as_integer_ratio()       # den is a power of two, at most 2^1074
        units += num * ((1 << 1074) // den)
    total = Fraction(units, 1 << 1074)
    if total == 0:
        return 0.0
    try:
        return float(total)                   # correctly rounded, ties to even
    except OverflowError:
        return math.inf if total > 0 else -math.inf


# ------------------------------------------------------------------ trees
def tree_dict(hc):
    """An HClust (or a dict already) as the plain dict used here."""
    if hc is None or isinstance(hc, dict):
        return hc
    return {"merge": [[int(a), int(b)] for a, b in np.asarray(hc.merge)], "height": [float(h) for h in hc.height],
            "order": [int(o) for o in hc.order], "labels": [str(l) for l in hc.labels]}


def _pair(a, b):
    neg = sorted([v for v in (a, b) if v < 0], key=lambda v: -v)
    pos = sorted(v for v in (a, b) if v > 0)
    return neg + pos


def _nested(tree):
    """(root, rows): nodes are ("leaf", i) or ("node", row, left, right)."""
    rows = []
    get = lambda v: ("leaf", -v) if v < 0 else rows[v - 1]
    for r, (a, b) in enumerate(tree["merge"]):
        rows.append(("node", r, get(a), get(b)))
    return rows[-1]


def prune_tree(tree, keep):
    """keep: one bool per leaf (label order)."""
    keep = [bool(k) for k in keep]
    if sum(keep) < 2:
        return None
    number = {}
    for i, k in enumerate(keep):
        if k:
            number[i + 1] = len(number) + 1

    def walk(node):                           # -> pruned node or None
        if node[0] == "leaf":
            return ("leaf", number[node[1]]) if keep[node[1] - 1] else None
        left, right = walk(node[2]), walk(node[3])
        if left is not None and right is not None:
            return ("node", node[1], left, right)
        return left if left is not None else right

    root = walk(_nested(tree))
    kept_rows = []

    def collect(node):
        if node[0] == "node":
            collect(node[2]); collect(node[3]); kept_rows.append(node)
    collect(root)
    kept_rows.sort(key=lambda nd: nd[1])
    new_row = {nd[1]: i + 1 for i, nd in enumerate(kept_rows)}
    ref = lambda nd: -nd[1] if nd[0] == "leaf" else new_row[nd[1]]
    return {"merge": [_pair(ref(nd[2]), ref(nd[3])) for nd in kept_rows], "height": [tree["height"][nd[1]] for nd in kept_rows],
            "order": [number[o] for o in tree["order"] if keep[o - 1]], "labels": [l for l, k in zip(tree["labels"], keep) if k]}


def expand_tree(tree, copies, labels=None, suffix_single=True):
    labels = list(tree["labels"] if labels is None else labels)
    copies = [int(c) for c in copies]
    first, acc = [], 1
    for c in copies:
        first.append(acc)
        acc += c
    merge, stands_for = [], {}
    for k, c in enumerate(copies):
        if c == 1:
            stands_for[k + 1] = -first[k]
            continue
        merge.append([-first[k], -(first[k] + 1)])
        for j in range(3, c + 1):
            merge.append([-(first[k] + j - 1), len(merge)])
        stands_for[k + 1] = len(merge)
    n_zero = len(merge)
    for a, b in tree["merge"]:
        a2 = stands_for[-a] if a < 0 else a + n_zero
        b2 = stands_for[-b] if b < 0 else b + n_zero
        merge.append(_pair(a2, b2))
    order = []
    for o in tree["order"]:
        order += list(range(first[o - 1], first[o - 1] + copies[o - 1]))
    new_labels = []
    for k, c in enumerate(copies):
        if c == 1 and not suffix_single:
            new_labels.append(str(labels[k]))
        else:
            new_labels += [f"{labels[k]}_{j}" for j in range(1, c + 1)]
    return {"merge": merge, "height": [0.0] * n_zero + list(tree["height"]), "order": order, "labels": new_labels}


def cophenetic(tree):
    """{(label a, label b): height of their first common merge}."""
    members, out = [], {}
    for (a, b), h in zip(tree["merge"], tree["height"]):
        la = [tree["labels"][-a - 1]] if a < 0 else members[a - 1]
        lb = [tree["labels"][-b - 1]] if b < 0 else members[b - 1]
        for p in la:
            for q in lb:
                out[(p, q)] = out[(q, p)] = h
        members.append(la + lb)
    return out


# ------------------------------------------------------------------ sample_object
def fnv1a64(text):
    h = 0xCBF29CE484222325
    for b in text.encode("utf-8"):
        h = ((h ^ b) * 0x100000001B3) % (1 << 64)
    return h


def draw(seed, group, v, size):
    gen = np.random.Generator(np.random.Philox(key=[seed, fnv1a64("sample_object/" + group)]))
    perm = gen.permutation(len(v))
    return [v[int(i)] for i in perm[:size]]


def _order_labels(hc, subs, colnames):
    """labels[order] of one tree, or plot_cnv's concatenation over a Leiden list (subs: 1-based indices)."""
    if isinstance(hc, dict):
        return [hc["labels"][o - 1] for o in hc["order"]]
    trees, out = list(hc), []
    for cells in subs.values():
        if len(cells) >= 2:
            t = trees.pop(0)
            out += [t["labels"][o - 1] for o in t["order"]]
        else:
            out += [colnames[c - 1] for c in cells]
    return out


def _each(hc, fn):
    return fn(hc) if isinstance(hc, dict) else [None if t is None else fn(t) for t in hc]


def sample_plan(colnames, ref_groups, obs_groups, hc, subclusters, n_cells=100, every_n=None, above_m=None, on_references=True,
                on_observations=True, seed=0):
    """colnames: the cells' names; ref_groups / obs_groups: {name: 1-based indices}; hc: {name: tree dict or list of them};
    subclusters: {name: {sub: 1-based indices}}.  Returns a dict with 0-based `source`, `names`, `ref`, `obs`, `hc`,
    `subclusters`."""
    do_every_n = every_n is not None and above_m is not None
    if do_every_n:
        n_cells = None
    match = {}
    for i, s in enumerate(colnames):
        match.setdefault(s, i + 1)
    new_hc, new_subs = dict(hc), {}
    columns, futur_colnames, ref, obs = [], [], {}, {}
    i = 1
    for groups, on, is_ref, into in ((ref_groups, on_references, True, ref), (obs_groups, on_observations, False, obs)):
        for sample_name, cells in groups.items():
            cells = [int(c) for c in cells]
            tree, subs = hc.get(sample_name), subclusters.get(sample_name)
            if not on:
                columns += cells
                futur_colnames += [colnames[c - 1] for c in cells]
                into[sample_name] = list(range(i, i + len(cells)))
                if subs is not None:
                    new_subs[sample_name] = {s: [i + cells.index(c) for c in v] for s, v in subs.items()}
                i += len(cells)
                continue
            if (n_cells is not None and len(cells) >= n_cells) or do_every_n:
                if not do_every_n:
                    sampled = draw(seed, sample_name, cells, n_cells)
                elif len(cells) > above_m:
                    upto = sum(len(v) for v in subs.values()) if is_ref else len(cells)
                    ordered = _order_labels(tree, subs, colnames)
                    sampled = [match[ordered[k - 1]] for k in range(1, upto + 1, every_n)]
                    for v in subs.values():
                        if not any(c in sampled for c in v):
                            sampled.append(v[0])
                else:
                    sampled = cells
                new_names = [colnames[c - 1] for c in sampled]
                if tree is not None:
                    kept = set(new_names)
                    pruned = _each(tree, lambda t: prune_tree(t, [l in kept for l in t["labels"]]))
                    if pruned is None:
                        new_hc.pop(sample_name, None)
                    else:
                        new_hc[sample_name] = pruned
                width = len(sampled)
            else:
                n_copies, to_sample = n_cells // len(cells), n_cells % len(cells)
                pre = draw(seed, sample_name, list(range(1, len(cells) + 1)), to_sample)
                times = {colnames[cells[k - 1] - 1]: n_copies + (1 if k in pre else 0) for k in range(1, len(cells) + 1)}
                if tree is not None:
                    if is_ref:
                        positions = sorted(pre + list(range(1, len(cells) + 1)) * n_copies)
                        sampled = [cells[p - 1] for p in positions]
                        new_names = [f"{colnames[c - 1]}_{j}" for j, c in enumerate(sampled, start=1)]
                        new_hc[sample_name] = _each(tree, lambda t: expand_tree(t, [times[l] for l in t["labels"]], suffix_single=False))
                    else:
                        ordered = _order_labels(tree, subs, colnames)
                        sampled, new_names = [], []
                        for l in ordered:
                            sampled += [match[l]] * times[l]
                            new_names += [f"{l}_{j}" for j in range(1, times[l] + 1)]
                        new_hc[sample_name] = _each(tree, lambda t: expand_tree(t, [times[l] for l in t["labels"]]))
                else:
                    label = colnames[cells[0] - 1]
                    sampled = [cells[0]] * n_cells
                    new_names = [f"{label}_{j}" for j in range(1, n_cells + 1)]
                    new_hc[sample_name] = {"merge": [[-1, -2]] + [[k, -(k + 2)] for k in range(1, n_copies - 1)],
                                           "height": [1.0] * (n_copies - 1), "order": list(range(1, n_copies + 1)),
                                           "labels": [f"{label}_{j}" for j in range(1, n_copies + 1)]}
                width = n_cells
            columns += sampled
            futur_colnames += new_names
            new_subs[sample_name] = {sample_name + "_s1": list(range(i, i + width))}
            into[sample_name] = list(range(i, i + width))
            i += width
    zero = lambda v: [c - 1 for c in v]
    return {"source": zero(columns), "names": futur_colnames, "ref": {k: zero(v) for k, v in ref.items()},
            "obs": {k: zero(v) for k, v in obs.items()}, "hc": new_hc,
            "subclusters": {g: {s: zero(v) for s, v in d.items()} for g, d in new_subs.items()}}


# ------------------------------------------------------------------ plot_per_group / plot_subclusters
def per_group_objects(ref_groups, obs_groups, hc, subclusters, on_references=True, on_observations=True):
    """[(tag, name, cells, tumor_subclusters or None)] in plotting order; indices 0-based; hc / subclusters None: no
    tumor_subclusters."""
    out = []
    for groups, on, tag in ((ref_groups, on_references, "REF"), (obs_groups, on_observations, "OBS")):
        if not on:
            continue
        for name, cells in groups.items():
            cells = [int(c) for c in cells]
            ts = None
            if hc is not None:
                ts = {"hc": {}, "subclusters": {}}
                if hc.get(name) is not None:
                    ts["hc"]["all_observations"] = hc[name]
                for sub, v in (subclusters.get(name) or {}).items():
                    ts["subclusters"].setdefault("all_observations", {})[sub] = [cells.index(int(c)) for c in v]
            out.append((tag, name, cells, ts))
    return out


def subcluster_object(ref_groups, obs_groups, subclusters):
    """(reference groups, observation groups) of plot_subclusters' object."""
    ref, obs = {}, {}
    for grp in ref_groups:
        for grp2, v in (subclusters.get(grp) or {}).items():
            ref[grp2] = [int(c) for c in v]
    for grp in list(obs_groups) + ["all_observations"]:
        for grp2, v in (subclusters.get(grp) or {}).items():
            obs[grp2] = [int(c) for c in v]
    return ref, obs


def make_filename(text):
    out = ""
    for ch in text:
        out += "_" if ch in '/\\:*?"<>|' else ch
    return out
