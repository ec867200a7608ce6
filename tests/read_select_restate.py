"""Expectations of the column-selected readers and of ShardedCreate (DESIGN K26), in plain Python on top of the two restatements
the full readers are held to: create_object_restate (text tables, CreateInfercnvObject) and sparse_counts_restate (MatrixMarket).
A selected read is a slice of the full read; only `read_table_cols` reads a file itself, because the selected read must not look
at the fields it skips.  Shares no code with infercnv_amd."""
import numpy as np

import create_object_restate as cor
import sparse_counts_restate as scr


def table_slice(table, sel):
    """(len(sel), rows) int64 bits of the columns `sel` of cor.read_table's (names, cols, bits)."""
    return np.ascontiguousarray(np.asarray(table[2], dtype=np.int64)[:, list(sel)].T)


def read_table_cols(path, sel, sep="\t"):
    """cor.read_table for the numeric columns `sel` only: float() is applied to the selected fields and to no other."""
    with open(path, "rb") as fh:
        text = fh.read().decode("utf-8")
    lines = [ln[:-1] if ln.endswith("\r") else ln for ln in text.split("\n")]
    header = [cor.strip_quotes(t) for t in lines[0].split(sep)]
    rows = [ln.split(sep) for ln in lines[1:] if ln != ""]
    width = len(rows[0])
    assert all(len(r) == width for r in rows)
    cols = header if len(header) == width - 1 else header[1:]
    vals = np.array([[cor.signed(cor.bits(r[1 + c])) for r in rows] for c in sel], dtype=np.int64).reshape(len(sel), len(rows))
    return [cor.strip_quotes(r[0]) for r in rows], cols, vals


def mtx_entries(path):
    """(G, C, nnz of the size line, the entries [(row, col, val)] in file order)."""
    data = scr.read_bytes(path)
    field, G, C, nnz, n_lines, n_bytes = scr.header(data)
    return G, C, nnz, scr.parse_body(data[n_bytes:], field, G, C, line0=n_lines + 1)


def mtx_slice(path, sel):
    """(colptr, rowidx, vals, sorted_already, kept) of the G x len(sel) matrix whose column k is file column sel[k]: the kept
    entries in file order with their new column, then what the full reader does with triplets."""
    G, C, nnz, entries = mtx_entries(path)
    assert len(entries) == nnz
    new_col = {int(c): k for k, c in enumerate(sel)}
    kept = [(r, new_col[c], v) for r, c, v in entries if c in new_col]
    return scr.csc_from_triplets(kept, G, len(sel)) + (len(kept),)


def deal(C_file, world, rank, how):
    """The file columns of a rank: rank, rank + world, ... or the rank-th of `world` contiguous blocks, the first C_file %
    world of them one longer."""
    if how == "cyclic":
        return list(range(rank, C_file, world))
    base, rem = divmod(C_file, world)
    c0 = rank * base + min(rank, rem)
    return list(range(c0, c0 + base + (1 if rank < rem else 0)))


def host_reader(path, cells):
    """The `reader` of ShardedCreate on the host: (genes, all cell names, the selected columns)."""
    from scipy.sparse import csc_matrix
    path = str(path)
    if path.endswith(".mtx") or path.endswith(".mtx.gz"):
        colptr, rowidx, vals, _, _ = mtx_slice(path, [int(c) for c in cells])
        G = mtx_entries(path)[0]
        return None, None, csc_matrix((vals.astype(np.float64), rowidx, colptr), shape=(G, len(cells)))
    table = cor.read_table(path)
    return table[0], table[1], cor.as_double(table_slice(table, [int(c) for c in cells]))


def expr_bits(obj):
    x = obj.expr_data.toarray() if hasattr(obj.expr_data, "toarray") else obj.expr_data
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.int64)


def check_shards(single, shards, C_file, world, how):
    """single: the single-rank InfercnvObject; shards[r] = (obj_r, x_r, shard_r).  The asserts of the issue's ShardedCreate list
    that need no device: J disjoint and covering, expr_data columns, groups mapped back in order, the other slots equal."""
    full = expr_bits(single)
    C = full.shape[1]
    seen = np.zeros(C, dtype=np.int64)
    for r, (obj, _, shard) in enumerate(shards):
        J = np.asarray(shard["global_index"])
        assert (shard["rank"], shard["world"], shard["deal"], shard["C_total"]) == (r, world, how, C)
        assert J.size >= 1 and np.all(np.diff(J) > 0)
        seen[J] += 1
        assert set(np.asarray(shard["file_columns"]).tolist()) <= set(deal(C_file, world, r, how))
        assert np.array_equal(expr_bits(obj), full[:, J])
        assert obj.count_data is obj.expr_data
        assert list(obj.cell_names) == [single.cell_names[j] for j in J] and list(obj.gene_names) == list(single.gene_names)
        for slot in ("chr", "start", "stop"):
            assert list(getattr(obj.gene_order, slot)) == list(getattr(single.gene_order, slot))
        assert obj.options == single.options and obj.validate()
        for mine, theirs in ((obj.reference_grouped_cell_indices, single.reference_grouped_cell_indices),
                             (obj.observation_grouped_cell_indices, single.observation_grouped_cell_indices)):
            assert list(mine) == list(theirs)
            for name in theirs:
                assert mine[name].dtype == np.int32
                assert J[mine[name]].tolist() == [j for j in np.asarray(theirs[name]).tolist() if j in set(J.tolist())]
    assert np.all(seen == 1)


def same_object(a, b):
    """Two InfercnvObjects slot for slot."""
    assert np.array_equal(expr_bits(a), expr_bits(b)) and hasattr(a.expr_data, "tocsc") == hasattr(b.expr_data, "tocsc")
    assert list(a.gene_names) == list(b.gene_names) and list(a.cell_names) == list(b.cell_names)
    for slot in ("chr", "start", "stop"):
        assert list(getattr(a.gene_order, slot)) == list(getattr(b.gene_order, slot))
    for da, db in ((a.reference_grouped_cell_indices, b.reference_grouped_cell_indices),
                   (a.observation_grouped_cell_indices, b.observation_grouped_cell_indices)):
        assert list(da) == list(db) and all(np.array_equal(da[k], db[k]) and da[k].dtype == db[k].dtype for k in da)
    assert a.options == b.options
