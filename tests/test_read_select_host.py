"""ShardedCreate's host logic without a GPU (DESIGN K26): the deal and the J arithmetic, the error cases, and run() over gloo.
The two device readers are replaced by tests/read_select_restate.host_reader, so every number comes from the restatements."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import create_object_restate as cor
import read_select_restate as rsr
import sparse_counts_restate as scr

pytest.importorskip("scipy")

from infercnv_amd import device, sharded                # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, C = 12, 13
LOW = (1,)                                               # cells whose counts fall below the default 100
GENE_ORDER = [[f"g{i}", "chr1" if i % 3 else "chr2", 100 * (G - i), 100 * (G - i) + 50] for i in range(G)] + [["gX", "chrX", 1, 2]]
ANNOT = [[f"cell{j}", ("normal", "tumorA", "tumorB")[j % 3]] for j in range(C)]


def counts_table():
    rng = np.random.default_rng(26)
    m = rng.integers(20, 60, size=(G, C))
    m[:, list(LOW)] = rng.integers(0, 5, size=(G, len(LOW)))
    return m


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("read_select_host")
    m = counts_table()
    table = str(d / "counts.tsv")
    with open(table, "w") as fh:
        fh.write("\t".join(f"cell{j}" for j in range(C)) + "\n")
        fh.write("".join(f"g{i}\t" + "\t".join(str(v) for v in m[i]) + "\n" for i in range(G)))
    mtx = str(d / "counts.mtx")
    scr.write_mtx(mtx, m)
    order, annot = str(d / "order.txt"), str(d / "annot.txt")
    with open(order, "w") as fh:
        fh.write("".join("\t".join(str(v) for v in r) + "\n" for r in GENE_ORDER))
    with open(annot, "w") as fh:
        fh.write("".join("\t".join(r) + "\n" for r in ANNOT))
    return {"table": table, "mtx": mtx, "order": order, "annot": annot, "genes": [f"g{i}" for i in range(G)],
            "cells": [f"cell{j}" for j in range(C)], "m": m}


def make(files, route, rank, world, how, **kw):
    names = dict(gene_names=files["genes"], cell_names=files["cells"]) if route == "mtx" else {}
    return sharded.ShardedCreate(files[route], files["order"], files["annot"], kw.pop("refs", ["normal"]), rank=rank, world=world, deal=how,
                                 reader=rsr.host_reader, **names, **kw)


def two_phase(files, route, world, how, **kw):
    ranks = [make(files, route, r, world, how, **kw) for r in range(world)]
    parts = [sc.read() for sc in ranks]
    for r, p in enumerate(parts):
        assert len(p) == len(rsr.deal(C, world, r, how))
    sums = ranks[0].place(parts)
    return sums, [sc.finish(sums) for sc in ranks]


@pytest.mark.parametrize("route", ["table", "mtx"])
@pytest.mark.parametrize("kw,worlds", [(dict(), range(1, 9)), (dict(max_cells_per_group=3, seed=5), (1, 2, 3))])
def test_deal_and_J_for_every_world_up_to_eight(files, route, kw, worlds):
    single, _, shard1 = make(files, route, 0, 1, "cyclic", **kw).run()
    table = cor.read_table(files["table"])
    want = cor.create_object(*table, files["order"], files["annot"], ["normal"], **kw)
    (scr.compare(cor, single, want) if route == "mtx" else cor.compare(single, want))
    assert shard1["global_index"].tolist() == list(range(len(want["cell_names"]))) and not set(LOW) & set(shard1["file_columns"].tolist())
    sizes = set()
    for world in worlds:
        for how in ("cyclic", "block"):
            sums, shards = two_phase(files, route, world, how, **kw)
            assert sums.tolist() == files["m"].sum(axis=0).tolist()
            rsr.check_shards(single, shards, C, world, how)
            sizes.add(tuple(len(s[2]["global_index"]) for s in shards))
    assert any(len(set(s)) > 1 for s in sizes)          # ranks with unequal counts


def test_errors_of_the_sharded_route(files):
    with pytest.raises(ValueError, match="world is 14, but the file has only 13 columns"):
        make(files, "table", 0, 14, "cyclic").read()
    with pytest.raises(ValueError, match="world is 14, but the file has only 13 columns"):
        make(files, "mtx", 13, 14, "block").read()
    # one column per rank: rank 1 holds file column 1, which is below the counts filter
    ranks = [make(files, "table", r, 13, "block") for r in range(13)]
    sums = ranks[0].place([sc.read() for sc in ranks])
    with pytest.raises(ValueError, match="no cell is left on rank 1 of 13"):
        ranks[1].finish(sums)
    assert ranks[0].finish(sums)[2]["C_total"] == C - len(LOW)
    # nothing left anywhere: the single-rank error, on every rank
    for r in range(2):
        sc = make(files, "table", r, 2, "block", refs=[], min_max_counts_per_cell=(10 ** 9, float("inf")))
        sc.read()
        with pytest.raises(ValueError, match="^no cell is left after the counts-per-cell filter and the annotations$"):
            sc.finish(sums)
    with pytest.raises(ValueError, match="col_sums_all has 3 entries"):
        ranks[0].finish(sums[:3])
    with pytest.raises(RuntimeError, match="finish\\(\\) comes after read\\(\\)"):
        make(files, "table", 0, 2, "block").finish(sums)
    with pytest.raises(RuntimeError, match="no process group"):
        make(files, "table", 0, 2, "block").run()
    with pytest.raises(ValueError, match="deal must be"):
        make(files, "table", 0, 2, "striped")
    with pytest.raises(ValueError, match="reads the matrix from a file"):
        sharded.ShardedCreate(files["m"], files["order"], files["annot"], ["normal"], rank=0, world=1).read()


def test_cells_argument_is_checked_before_the_file_is_opened():
    for read in (device.read_table, device.read_mtx):
        for cells, text in (([], "non-empty"), ([2, 0, 2], "column 2 more than once"), ([1, -3], "entry -3 is negative")):
            with pytest.raises(ValueError, match=text):
                read("/no/such/file.mtx", cells=cells)


WORKER = r'''
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np, torch.distributed as dist
import read_select_restate as rsr
from infercnv_amd import sharded
port, rank, table, order, annot = sys.argv[2], int(sys.argv[3]), sys.argv[4], sys.argv[5], sys.argv[6]
kw = dict(deal="cyclic", reader=rsr.host_reader, max_cells_per_group=3, seed=2)
ranks = [sharded.ShardedCreate(table, order, annot, ["normal"], rank=r, world=2, **kw) for r in range(2)]
sums = ranks[0].place([sc.read() for sc in ranks])
want, want_x, want_shard = ranks[rank].finish(sums)                 # the in-process two-phase result of this rank
dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=2)
obj, x, shard = sharded.ShardedCreate(table, order, annot, ["normal"], rank=rank, world=2, **kw).run()
rsr.same_object(obj, want)
assert np.array_equal(x, want_x) and x.shape[0] == len(shard["global_index"])
assert all(np.array_equal(shard[k], want_shard[k]) for k in ("global_index", "file_columns")) and shard["C_total"] == want_shard["C_total"]
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "ok", len(shard["global_index"]))
'''


def test_run_over_gloo_with_two_ranks(files, tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = [subprocess.Popen([sys.executable, str(script), ROOT, str(port), str(r), files["table"], files["order"], files["annot"]],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=240)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} failed:\n{o[-3000:]}"
        assert f"rank {r} ok" in o
