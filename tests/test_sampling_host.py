"""sample_object / plot_per_group / plot_subclusters on the host (infercnv_amd.sampling, the tree helpers of
infercnv_amd.tumor_subclusters) against the sequential restatement of tests/sampling_restate.py.  No GPU."""
import os

import numpy as np
import pytest
from scipy.cluster.hierarchy import cophenet
from scipy.spatial.distance import squareform

import sampling_restate as sr

from infercnv_amd import GeneOrder, InfercnvObject, sampling            # noqa: E402
from infercnv_amd import tumor_subclusters as ts                         # noqa: E402
from infercnv_amd.tumor_subclusters import HClust, expand_hclust, prune_hclust   # noqa: E402


# ---------------------------------------------------------------- hand-made trees
def make_tree(labels, seed, tie=2):
    """A valid R hclust over `labels`: random merges in R's row conventions, heights that rise every `tie` rows (equal heights
    in between), order from the left-to-right walk of the last merge."""
    n = len(labels)
    rng = np.random.default_rng(seed)
    alive = [(-(i + 1), [i + 1]) for i in range(n)]           # (reference, leaves left to right)
    merge, height = [], []
    for step in range(n - 1):
        i, j = sorted(rng.choice(len(alive), size=2, replace=False).tolist())
        a, b = alive[i], alive[j]
        pair = sorted((a, b), key=lambda t: (t[0] > 0, abs(t[0])))
        merge.append([pair[0][0], pair[1][0]])
        height.append(float(step // tie) * 0.5)
        alive = [t for k, t in enumerate(alive) if k not in (i, j)] + [(step + 1, pair[0][1] + pair[1][1])]
    return HClust(np.asarray(merge, dtype=np.int32).reshape(n - 1, 2), np.asarray(height), np.asarray(alive[0][1], dtype=np.int32),
                  np.asarray(labels), "hand-made")


def linkage_of(tree):
    """scipy's linkage matrix of an hclust (leaf i -> i - 1, row r -> n + r - 1)."""
    n = len(tree.labels)
    size, Z = {}, []
    node = lambda v: (-v - 1) if v < 0 else n + v - 1
    for r, ((a, b), h) in enumerate(zip(np.asarray(tree.merge).tolist(), tree.height)):
        cnt = size.get(node(a), 1) + size.get(node(b), 1)
        size[n + r] = cnt
        Z.append([node(a), node(b), h, cnt])
    return np.asarray(Z, dtype=np.float64)


def coph(tree):
    n = len(tree.labels)
    return squareform(cophenet(linkage_of(tree))) if n > 2 else np.array([[0.0, tree.height[0]], [tree.height[0], 0.0]])


def check_conventions(tree):
    merge = np.asarray(tree.merge)
    n = merge.shape[0] + 1
    assert len(tree.labels) == n and sorted(np.asarray(tree.order).tolist()) == list(range(1, n + 1))
    assert (np.diff(tree.height) >= 0).all()
    used = []
    for r, (a, b) in enumerate(merge.tolist()):
        assert a != 0 and b != 0 and a < r + 1 and b < r + 1 and -n <= a and -n <= b
        if a < 0 and b < 0:
            assert -a < -b
        elif a > 0 and b > 0:
            assert a < b
        else:
            assert a < 0 < b
        used += [a, b]
    assert len(set(used)) == len(used)                        # every node merged once


def equal_trees(got, want):
    want = sr.tree_dict(want)
    assert np.asarray(got.merge).tolist() == want["merge"]
    assert np.asarray(got.height).tolist() == want["height"]
    assert np.asarray(got.order).tolist() == want["order"]
    assert [str(l) for l in got.labels] == want["labels"]


SIZES = [2, 3, 7, 33]


@pytest.mark.parametrize("n", SIZES)
def test_prune_hclust(n):
    labels = [f"c{i}" for i in range(n)]
    for seed in range(3):
        tree = make_tree(labels, seed)
        check_conventions(tree)
        full = coph(tree)
        rng = np.random.default_rng(100 + seed)
        masks = [np.ones(n, dtype=bool), rng.random(n) < 0.5, rng.random(n) < 0.2]
        masks.append(np.arange(n) < 2)
        masks.append(np.arange(n) >= n - 2)
        for mask in masks:
            got = prune_hclust(tree, mask)
            want = sr.prune_tree(sr.tree_dict(tree), mask)
            if mask.sum() < 2:
                assert got is None and want is None
                continue
            equal_trees(got, want)
            check_conventions(got)
            kept = np.flatnonzero(mask)
            assert np.array_equal(coph(got), full[np.ix_(kept, kept)])
            by_index = prune_hclust(tree, kept[::-1])
            equal_trees(by_index, want)
        equal_trees(prune_hclust(tree, np.ones(n, dtype=bool)), tree)
        one = np.zeros(n, dtype=bool)
        one[n // 2] = True
        assert prune_hclust(tree, one) is None and prune_hclust(tree, np.zeros(n, dtype=bool)) is None


@pytest.mark.parametrize("n", SIZES)
def test_expand_hclust(n):
    labels = [f"c{i}" for i in range(n)]
    for seed in range(3):
        tree = make_tree(labels, seed)
        full = coph(tree)
        rng = np.random.default_rng(200 + seed)
        for copies in (np.ones(n, dtype=int), rng.integers(1, 4, n), np.where(np.arange(n) == n - 1, 5, 1)):
            got = expand_hclust(tree, copies, tree.labels)
            equal_trees(got, sr.expand_tree(sr.tree_dict(tree), copies))
            check_conventions(got)
            origin = np.repeat(np.arange(n), copies)
            d = coph(got)
            want = full[np.ix_(origin, origin)]                # 0 between copies of one leaf (the diagonal), else as before
            assert np.array_equal(d, want)
            assert [str(l) for l in got.labels] == [f"c{k}_{j}" for k in range(n) for j in range(1, copies[k] + 1)]
            assert int((np.asarray(got.height) == 0).sum()) >= int((copies - 1).sum())
    with pytest.raises(ValueError):
        expand_hclust(tree, np.zeros(n, dtype=int))


# ---------------------------------------------------------------- the object
def build_object(leiden=False, with_ts=True):
    sizes = {"refA": 8, "refB": 1, "o1": 1, "o6": 6, "o40": 40}
    rng = np.random.default_rng(5)
    C = sum(sizes.values())
    perm = rng.permutation(C)                                   # groups are scattered over the columns
    groups, at = {}, 0
    for name, n in sizes.items():
        groups[name] = np.sort(perm[at:at + n]).astype(np.int64)
        at += n
    names = np.array([f"cell{i:02d}" for i in range(C)])
    G = 12
    expr = rng.normal(1.0, 0.1, size=(G, C))
    subs = {"refA": {"refA_s1": groups["refA"][:5], "refA_s2": groups["refA"][5:]}, "refB": {"refB_s1": groups["refB"]},
            "o1": {"o1_s1": groups["o1"]}, "o6": {"o6_s1": groups["o6"]},
            "o40": {"o40_s1": groups["o40"][0:25], "o40_s2": groups["o40"][25:26], "o40_s3": groups["o40"][26:]}}
    hc = {"refA": make_tree(names[groups["refA"]], 1), "o6": make_tree(names[groups["o6"]], 2, tie=1),
          "o40": make_tree(names[groups["o40"]], 3, tie=3)}
    if leiden:                                                  # one tree per partition of two or more cells
        hc["o40"] = [make_tree(names[subs["o40"]["o40_s1"]], 4), make_tree(names[subs["o40"]["o40_s3"]], 5)]
    obj = InfercnvObject(expr_data=expr, gene_order=GeneOrder(chr=np.repeat(["chr1", "chr2", "chr3"], 4)),
                         reference_grouped_cell_indices={k: groups[k] for k in ("refA", "refB")},
                         observation_grouped_cell_indices={k: groups[k] for k in ("o1", "o6", "o40")},
                         tumor_subclusters={"hc": hc, "subclusters": subs} if with_ts else None,
                         gene_names=np.array([f"g{i}" for i in range(G)]), cell_names=names)
    return obj


def restate_plan(obj, **kw):
    t = obj.tumor_subclusters or {}
    one = lambda d: {k: [int(c) + 1 for c in v] for k, v in d.items()}
    hc = {k: ([sr.tree_dict(x) for x in v] if isinstance(v, list) else sr.tree_dict(v)) for k, v in (t.get("hc") or {}).items()}
    return sr.sample_plan([str(c) for c in obj.cells()], one(obj.reference_grouped_cell_indices), one(obj.observation_grouped_cell_indices),
                          hc, {g: one(d) for g, d in (t.get("subclusters") or {}).items()}, **kw)


def check_plan(plan, want):
    assert plan.source.tolist() == want["source"]
    assert [str(s) for s in plan.cell_names] == want["names"]
    for got_groups, want_groups in ((plan.reference_grouped_cell_indices, want["ref"]), (plan.observation_grouped_cell_indices, want["obs"])):
        assert list(got_groups) == list(want_groups)
        for k in want_groups:
            assert np.asarray(got_groups[k]).tolist() == want_groups[k]
    got_subs = plan.tumor_subclusters["subclusters"]
    assert list(got_subs) == list(want["subclusters"])
    for g, d in want["subclusters"].items():
        assert list(got_subs[g]) == list(d)
        for s, v in d.items():
            assert np.asarray(got_subs[g][s]).tolist() == v
    got_hc = plan.tumor_subclusters["hc"]
    assert sorted(got_hc) == sorted(want["hc"])
    for g, t in want["hc"].items():
        if isinstance(t, list):
            assert isinstance(got_hc[g], list) and len(got_hc[g]) == len(t)
            for a, b in zip(got_hc[g], t):
                assert (a is None) == (b is None)
                if b is not None:
                    equal_trees(a, b)
        else:
            equal_trees(got_hc[g], t)
            check_conventions(got_hc[g]) if g != "o1" and g != "refB" else None


CASES = [dict(n_cells=n) for n in (1, 6, 7, 40, 100)] + \
        [dict(every_n=e, above_m=m) for e in (2, 7) for m in (5, 50)]
SWITCHES = [(True, True), (True, False), (False, True), (False, False)]


@pytest.mark.parametrize("leiden", [False, True])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_sample_plan(case, leiden):
    obj = build_object(leiden)
    for on_ref, on_obs in SWITCHES:
        kw = dict(case, on_references=on_ref, on_observations=on_obs, seed=3)
        plan = sampling.sample_plan(obj, **kw)
        check_plan(plan, restate_plan(obj, **kw))
        if "n_cells" in case:
            n = case["n_cells"]
            for groups, on in ((plan.reference_grouped_cell_indices, on_ref), (plan.observation_grouped_cell_indices, on_obs)):
                if on:
                    assert all(len(v) == n for v in groups.values())
        new = sampling.sample_object(obj, **kw)
        assert np.array_equal(new.expr_data, obj.expr_data[:, plan.source]) and new.count_data is None
        assert new.gene_order is obj.gene_order and new.hspike is obj.hspike and list(new.cells()) == list(plan.cell_names)
        assert new.validate()


def test_sample_plan_without_subclusters():
    obj = build_object(with_ts=False)
    kw = dict(n_cells=1, seed=1)
    check_plan(sampling.sample_plan(obj, **kw), restate_plan(obj, **kw))
    one_cell = InfercnvObject(expr_data=obj.expr_data, gene_order=obj.gene_order, observation_grouped_cell_indices={"o1": obj.observation_grouped_cell_indices["o1"]},
                              cell_names=obj.cell_names, gene_names=obj.gene_names)
    plan = sampling.sample_plan(one_cell, n_cells=4)
    assert np.asarray(plan.tumor_subclusters["hc"]["o1"].merge).tolist() == [[-1, -2], [1, -3], [2, -4]]
    assert plan.tumor_subclusters["hc"]["o1"].height.tolist() == [1.0, 1.0, 1.0]
    check_plan(plan, restate_plan(one_cell, n_cells=4))


def test_draws_are_keyed_by_seed_and_group_name():
    obj = build_object()
    a = sampling.sample_plan(obj, n_cells=7, seed=1)
    b = sampling.sample_plan(obj, n_cells=7, seed=2)
    again = sampling.sample_plan(obj, n_cells=7, seed=1)
    assert a.source.tolist() == again.source.tolist() and list(a.cell_names) == list(again.cell_names)
    o40 = lambda p: p.source[p.observation_grouped_cell_indices["o40"]].tolist()
    assert o40(a) != o40(b)
    renamed = obj.copy()
    renamed.observation_grouped_cell_indices = {("tumor" if k == "o40" else k): v for k, v in obj.observation_grouped_cell_indices.items()}
    t = obj.tumor_subclusters
    renamed.tumor_subclusters = {"hc": {("tumor" if k == "o40" else k): v for k, v in t["hc"].items()},
                                 "subclusters": {("tumor" if k == "o40" else k): v for k, v in t["subclusters"].items()}}
    c = sampling.sample_plan(renamed, n_cells=7, seed=1)
    assert c.source[c.observation_grouped_cell_indices["tumor"]].tolist() != o40(a)
    assert sorted(o40(a)) != sorted(c.source[c.observation_grouped_cell_indices["tumor"]].tolist())
    o6 = lambda p: p.source[p.observation_grouped_cell_indices["o6"]].tolist()
    assert o6(a) == o6(c)                                      # another group's name does not move this group's draw


# ---------------------------------------------------------------- errors and names
def test_argument_errors():
    obj = build_object()
    for kw, text in ((dict(every_n=1, above_m=5), "every_n < 2"), (dict(every_n=2.5, above_m=5), "every_n not an integer"),
                     (dict(every_n=2, above_m="5"), "above_m not numeric"), (dict(n_cells=0), "invalid n_cells"),
                     (dict(n_cells=None), "invalid n_cells"), (dict(n_cells=None, every_n=3), "invalid n_cells"),
                     (dict(n_cells=0, above_m=3), "invalid n_cells"), (dict(n_cells=2.5), "invalid n_cells")):
        with pytest.raises(ValueError, match=text):
            sampling.sample_plan(obj, **kw)
    only_one = sampling.sample_plan(obj, n_cells=6, every_n=3, seed=3)             # falls through to n_cells
    assert only_one.source.tolist() == sampling.sample_plan(obj, n_cells=6, seed=3).source.tolist()


def test_broken_r_paths_raise():
    obj = build_object()
    t = obj.tumor_subclusters

    def variant(hc=None, subs=None, **fields):
        o = obj.copy()
        o.tumor_subclusters = {"hc": dict(t["hc"], **(hc or {})), "subclusters": dict(t["subclusters"], **(subs or {}))}
        for k, v in fields.items():
            setattr(o, k, v)
        return o

    rekeyed = variant()
    rekeyed.tumor_subclusters["hc"]["all_observations"] = rekeyed.tumor_subclusters["hc"].pop("o40")
    with pytest.raises(ValueError, match=r"infercnv_sampling\.R:274"):
        sampling.sample_plan(rekeyed, every_n=2, above_m=5)
    no_ref_tree = variant()
    del no_ref_tree.tumor_subclusters["hc"]["refA"]
    with pytest.raises(ValueError, match=r"infercnv_sampling\.R:155"):
        sampling.sample_plan(no_ref_tree, every_n=2, above_m=5)
    no_ref_subs = variant()
    del no_ref_subs.tumor_subclusters["subclusters"]["refA"]
    with pytest.raises(ValueError, match=r"infercnv_sampling\.R:153"):
        sampling.sample_plan(no_ref_subs, every_n=2, above_m=5)
    short_tree = variant(hc={"o40": make_tree(obj.cell_names[obj.observation_grouped_cell_indices["o40"]][:30], 1)})
    with pytest.raises(ValueError, match=r"30 leaves for 40 cells.*:274"):
        sampling.sample_plan(short_tree, every_n=2, above_m=5)
    with pytest.raises(ValueError, match=r"infercnv_sampling\.R:370"):
        sampling.sample_plan(short_tree, n_cells=100)
    stranger = variant(hc={"o6": make_tree(["nobody"] + list(obj.cell_names[obj.observation_grouped_cell_indices["o6"]][1:]), 1)})
    with pytest.raises(ValueError, match=r"'nobody'.*:274"):
        sampling.sample_plan(stranger, every_n=2, above_m=5)
    with pytest.raises(ValueError, match=r"'nobody'.*:316"):
        sampling.sample_plan(stranger, n_cells=100)
    ref_stranger = variant(hc={"refA": make_tree(["nobody"] + list(obj.cell_names[obj.reference_grouped_cell_indices["refA"]][1:]), 1)})
    with pytest.raises(ValueError, match=r"'nobody'.*:182"):
        sampling.sample_plan(ref_stranger, n_cells=100)
    leiden = build_object(leiden=True)
    leiden.tumor_subclusters["hc"]["o40"] = leiden.tumor_subclusters["hc"]["o40"][:1]
    with pytest.raises(ValueError, match="without a tree"):
        sampling.sample_plan(leiden, every_n=2, above_m=5)
    two_subs = variant()
    del two_subs.tumor_subclusters["hc"]["refA"]
    with pytest.raises(ValueError, match="Missing clustering information"):
        sampling.sample_plan(two_subs, n_cells=100)
    no_tree = variant()
    del no_tree.tumor_subclusters["hc"]["o6"]
    with pytest.raises(ValueError, match=r"6 cells and no tree.*:395"):
        sampling.sample_plan(no_tree, n_cells=100)
    no_ref_tree_one_sub = variant(subs={"refA": {"refA_s1": obj.reference_grouped_cell_indices["refA"]}})
    del no_ref_tree_one_sub.tumor_subclusters["hc"]["refA"]
    with pytest.raises(ValueError, match=r"8 cells and no tree.*:225"):
        sampling.sample_plan(no_ref_tree_one_sub, n_cells=100)
    empty = variant(observation_grouped_cell_indices=dict(obj.observation_grouped_cell_indices, none=np.zeros(0, dtype=np.int64)))
    with pytest.raises(ValueError, match=r"is empty.*:150"):
        sampling.sample_plan(empty, n_cells=5)


def test_refusals_come_before_any_file(tmp_path):
    obj = build_object()
    target = tmp_path / "never"
    with pytest.raises(NotImplementedError):
        sampling.plot_per_group(obj, save_objects=True, out_dir=str(target))
    with pytest.raises(ValueError, match="out_dir"):
        sampling.plot_per_group(obj)
    assert not target.exists() and os.listdir(tmp_path) == []
    bare = build_object(with_ts=False)
    with pytest.raises(ValueError, match="no tumor_subclusters"):
        ts.plot_subclusters(bare, str(target))
    assert not target.exists()


def test_make_filename():
    for ch in '/\\:*?"<>|':
        assert sampling.make_filename(f"a{ch}b") == "a_b" == sr.make_filename(f"a{ch}b")
    assert sampling.make_filename('/\\:*?"<>|') == "_" * 9
    assert sampling.make_filename("T cells (CD8+) #1.x-y_z") == "T cells (CD8+) #1.x-y_z"


# ---------------------------------------------------------------- per-group objects, the subcluster object
@pytest.mark.parametrize("with_ts", [True, False])
def test_per_group_objects(with_ts):
    obj = build_object(with_ts=with_ts)
    t = obj.tumor_subclusters
    want = sr.per_group_objects(obj.reference_grouped_cell_indices, obj.observation_grouped_cell_indices, t["hc"] if t else None,
                                t["subclusters"] if t else None)
    assert [(tag, name) for tag, name, _, _ in want] == [("REF", "refA"), ("REF", "refB"), ("OBS", "o1"), ("OBS", "o6"), ("OBS", "o40")]
    for tag, name, cells, want_ts in want:
        groups = obj.reference_grouped_cell_indices if tag == "REF" else obj.observation_grouped_cell_indices
        got = sampling.per_group_object(obj, name, groups[name], obj.expr_data[:, groups[name]])
        assert got.reference_grouped_cell_indices == {} and list(got.observation_grouped_cell_indices) == [name]
        assert got.observation_grouped_cell_indices[name].tolist() == list(range(len(cells)))
        assert list(got.cells()) == list(obj.cell_names[cells]) and got.validate()
        if want_ts is None:
            assert got.tumor_subclusters is None
            continue
        assert list(got.tumor_subclusters["hc"]) == list(want_ts["hc"])
        if want_ts["hc"]:
            assert got.tumor_subclusters["hc"]["all_observations"] is want_ts["hc"]["all_observations"]
        subs = got.tumor_subclusters["subclusters"]["all_observations"]
        assert list(subs) == list(want_ts["subclusters"]["all_observations"])
        for s, v in want_ts["subclusters"]["all_observations"].items():
            assert subs[s].tolist() == v
