"""Cell-sharded multi-GPU execution: one process per GPU, torch.distributed
(backend "nccl" == RCCL over xGMI on ROCm; "gloo" in the CPU tests).

Cells are independent in every stage of the hot path, so each
rank owns its share of the cells -- a contiguous block, a round-robin deal
(`cyclic_cells`) or whole groups -- and there is NO data-path collective.
The only exchange is the reference-normal statistics of the smoothing chain:
one small all-reduce(sum) per reference round (steps 8, 12 and 22 each need
the statistics of the *previous* stages' output on the reference cells, so the
rounds are dependent):

    subtract rounds: [G * n_ref_groups gene sums | n_ref_groups counts]  (160 KB at G=10k, 2 groups)
    denoise round:   [sum x, sum_c sd_c, n_ref_cells, n_ref_values]       (32 B)

The per-rank engine is `device.ChainPlan` (libicnv_hip.so); anything with the
same four methods can be plugged in (the gloo tests use an oracle-backed one).
"""
from __future__ import annotations

import numpy as np


def shard_bounds(C_total: int, world: int, rank: int):
    """Contiguous block [c0, c1) of rank `rank`; the first C_total % world ranks get one more cell."""
    base, rem = divmod(int(C_total), int(world))
    c0 = rank * base + min(rank, rem)
    return c0, c0 + base + (1 if rank < rem else 0)


def localize_groups(groups, c0: int, c1: int):
    """Keep each group's members that live in [c0, c1), as LOCAL indices, order preserved."""
    out = []
    for g in groups:
        g = np.asarray(g, dtype=np.int64)
        m = g[(g >= c0) & (g < c1)] - c0
        out.append(m.astype(np.int32))
    return out


def cyclic_cells(C_total: int, world: int, rank: int):
    """Global indices of the cells rank `rank` holds when cells are dealt round-robin: rank, rank + world, ...
    Every annotation group -- the reference groups in particular -- is then spread evenly over the ranks, so the
    reference rounds cost every rank the same (a contiguous block partition of a matrix whose reference cells
    come first would leave them all on rank 0)."""
    return np.arange(rank, C_total, world, dtype=np.int64)


def localize_groups_cyclic(groups, rank: int, world: int):
    """Members of each group held by `rank` under the round-robin deal, as LOCAL indices, order preserved."""
    out = []
    for g in groups:
        g = np.asarray(g, dtype=np.int64)
        m = g[(g % world) == rank]
        out.append(((m - rank) // world).astype(np.int32))
    return out


def align_to_groups(C_total: int, world: int, group_boundaries):
    """Shard boundaries moved to the nearest group boundary so that every group
    (HMM subcluster / median-filter tile) lives on one GPU.
    `group_boundaries`: sorted cell offsets at which a cut is allowed."""
    gb = np.asarray(sorted(set(int(b) for b in group_boundaries) | {0, int(C_total)}), dtype=np.int64)
    cuts = [0]
    for r in range(1, world):
        ideal = shard_bounds(C_total, world, r)[0]
        cand = gb[np.argmin(np.abs(gb - ideal))]
        cuts.append(int(max(cand, cuts[-1])))
    cuts.append(int(C_total))
    return [(cuts[i], cuts[i + 1]) for i in range(world)]


class ShardedChain:
    """Drives one rank's engine through the reference rounds with an all-reduce
    between `round_partial` and `round_finish`, then the fused apply pass."""

    def __init__(self, engine, process_group=None, world_size=None, always_reduce=False):
        self.engine = engine
        self.pg = process_group
        self.world = world_size
        self.always_reduce = always_reduce      # issue the collective on a communicator of one rank too (bench.py's RCCL smoke)

    def _all_reduce(self, buf):
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and (dist.get_world_size(self.pg) > 1 or self.always_reduce):
            dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.pg)

    def run(self, x_local, out=None, want_pre_denoise=False, pre=None):
        for r in range(self.engine.num_rounds):
            buf = self.engine.round_partial(r, x_local)
            self._all_reduce(buf)
            self.engine.round_finish(r)
        if pre is not None:                      # a preallocated HMM-input matrix (engines without the keyword allocate their own)
            return self.engine.apply(x_local, out=out, want_pre_denoise=True, pre=pre)
        return self.engine.apply(x_local, out=out, want_pre_denoise=want_pre_denoise)


# ---------------------------------------------------------------------------------------------------------------------
# Group-level HMM (BASELINE config 4: i3 at subcluster level) and the 2-D median filter (config 5) on cell shards.
#
# Groups are independent in the group HMM (R/inferCNV_HMM.R:371, 529-533; R/inferCNV_i3HMM.R:249-308) and tiles in the
# median filter (R/noise_reduction.R:57-86), so the partition puts every group / tile WHOLE on one rank: no halo, no
# cross-rank mean.  RCCL call sequence per step (all latency-bound, f64, sum):
#   group HMM, i3:  all-reduce of 2 doubles {sum x, n} over the reference values     -> mu
#                   all-reduce of 2 doubles {sum (x - mu)^2, n}                      -> sigma, delta = |qnorm(p, 0, sigma)|
#                   then group means -> Viterbi -> broadcast, rank-local
#   group HMM, i6:  none (the per-group sd comes from the hspike fit, a host-side input)
#   median filter:  none
def assign_groups(group_sizes, world: int):
    """Whole groups to ranks: longest group first onto the least loaded rank (ties: lowest rank) -- deterministic.
    Returns one ascending list of group ids per rank."""
    sizes = [int(s) for s in group_sizes]
    load = [0] * world
    out = [[] for _ in range(world)]
    for gid in sorted(range(len(sizes)), key=lambda i: (-sizes[i], i)):
        r = min(range(world), key=lambda k: (load[k], k))
        out[r].append(gid)
        load[r] += sizes[gid]
    return [sorted(v) for v in out]


def gather_groups(groups, group_ids):
    """The cells a rank holds when it owns `group_ids`: (global cell ids in storage order, the groups as LOCAL index lists).
    A cell that sits in several owned groups is stored once."""
    cells, pos = [], {}
    local = []
    for gid in group_ids:
        idx = []
        for c in np.asarray(groups[gid], dtype=np.int64):
            c = int(c)
            if c not in pos:
                pos[c] = len(cells)
                cells.append(c)
            idx.append(pos[c])
        local.append(np.asarray(idx, dtype=np.int32))
    return np.asarray(cells, dtype=np.int64), local


def _all_reduce_pair(a, b, pg=None, device=None):
    """all-reduce(sum) of two doubles; a no-op without an initialised process group."""
    import torch
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size(pg) > 1):
        return float(a), float(b)
    buf = torch.tensor([a, b], dtype=torch.float64, device=device if device is not None else "cpu")
    dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=pg)
    v = buf.cpu().tolist()
    return v[0], v[1]


def sharded_mean_sd(moments_partial, pg=None, device=None):
    """mean and sd over ALL reference values of a cell-sharded matrix (R/inferCNV_i3HMM.R:38-52: mean(ref), sd(ref)):
    `moments_partial(phase, mean)` returns this rank's {sum, n} (phase 0) or {sum (x - mean)^2, n} (phase 1) --
    icnv_cells_moments_partial_dev; two all-reduces of two doubles."""
    s, n = _all_reduce_pair(*moments_partial(0, 0.0), pg=pg, device=device)
    if not n > 1:
        raise ValueError("fewer than two reference values")
    mean = s / n
    ss, n2 = _all_reduce_pair(*moments_partial(1, mean), pg=pg, device=device)
    return mean, float(np.sqrt(ss / (n2 - 1.0)))


class DeviceGroupEngine:
    """The rank-local pieces of the group HMM / median filter on libicnv_hip.so (device-resident tensors)."""

    def moments_partial(self, x_local, ref_local, phase, mean):
        from . import device
        return device.cells_moments_partial(x_local, ref_local, phase, mean)

    def viterbi_groups(self, x_local, chr_start, groups_local, means, sds, logPi, logDelta):
        from . import device
        return device.viterbi_groups(x_local, chr_start, groups_local, means, sds, logPi, logDelta)[0]

    def median_filter(self, x_local, chr_start, tiles_local, window_size, na_aware=False):
        from . import device
        return device.median_filter(x_local, chr_start, tiles_local, window_size, na_aware=na_aware)


class ShardedGroupHMM:
    """predict_CNV_via_HMM_on_tumor_subclusters / _whole_tumor_samples and their i3 forms on a cell-sharded matrix whose
    groups are whole on their ranks (assign_groups + gather_groups, or contiguous blocks cut by align_to_groups)."""

    def __init__(self, engine=None, process_group=None, device=None):
        self.engine = engine or DeviceGroupEngine()
        self.pg = process_group
        self.device = device

    def i3_params(self, x_local, ref_local, i3_p_val=0.05):
        """(mu, sigma, delta) of .i3HMM_get_sd_trend_by_num_cells_fit (R/inferCNV_i3HMM.R:17-80, 435-445)."""
        import statistics
        mu, sigma = sharded_mean_sd(lambda ph, m: self.engine.moments_partial(x_local, ref_local, ph, m), self.pg, self.device)
        return mu, sigma, abs(statistics.NormalDist(0.0, sigma).inv_cdf(i3_p_val))

    def _plan_for(self, x_local, chr_start, groups_local, ref_local):
        """The device plan of this (matrix shape, layout, groups, reference cells), built on first use and kept: the group
        structure is uploaded once, not per step.  None when the engine is not the device engine or the plan does not take
        the groups (a cell in two groups, more than 8192 sequences): run_i3 then takes the call-by-call path."""
        if not isinstance(self.engine, DeviceGroupEngine):
            return None
        key = (tuple(x_local.shape), np.asarray(chr_start).tobytes(), tuple(np.asarray(g).tobytes() for g in groups_local),
               np.asarray(ref_local).tobytes())
        if getattr(self, "_plan_key", None) != key:
            from . import device
            self._plan, self._plan_key = None, key
            try:
                self._plan = device.GroupHMMPlan(x_local.shape[1], x_local.shape[0], chr_start, groups_local, ref_local)
            except RuntimeError as e:                # ICNV_ERR_UNSUPPORTED (3): the call-by-call path serves these groups
                if getattr(e, "code", None) != 3:
                    raise
                self._plan = None
        return self._plan

    def run_i3(self, x_local, chr_start, groups_local, ref_local, t=1e-6, i3_p_val=0.05, ks_delta=None):
        """i3HMM_predict_CNV_via_HMM_on_tumor_subclusters (R/inferCNV_i3HMM.R:249-308): states of this rank's cells.
        The state means sit at mu +- delta: the Z-based delta of use_KS = FALSE, or `ks_delta` -- the KS-based one of the
        reference's default use_KS = TRUE, a function of (sigma, p, number of reference cells, RNG state) alone
        (hmm.get_HoneyBADGER_setGexpDev), so every rank computes the same value from the all-reduced sigma."""
        Pi = np.full((3, 3), t)
        np.fill_diagonal(Pi, 1.0 - 5.0 * t)               # the reference's 1 - 5t diagonal with three states (:108-112)
        d0 = np.array([t, 1.0 - 5.0 * t, t])
        plan = None if callable(ks_delta) else self._plan_for(x_local, chr_start, groups_local, ref_local)
        if plan is not None:
            # device-resident parameters (round 6): one pass for the group means AND the reference moments, the all-reduce of three
            # doubles on the library's own buffer, mu / sigma / delta derived on the device -- no host round trip in the step
            import statistics
            import torch.distributed as dist
            m3 = plan.i3_partial(x_local)
            if dist.is_available() and dist.is_initialized() and dist.get_world_size(self.pg) > 1:
                dist.all_reduce(m3, op=dist.ReduceOp.SUM, group=self.pg)
            z = abs(statistics.NormalDist().inv_cdf(i3_p_val))
            return plan.i3_finish(np.log(Pi), np.log(d0), z, None if ks_delta is None else float(ks_delta), device=x_local.device)
        mu, sigma, delta = self.i3_params(x_local, ref_local, i3_p_val)
        if ks_delta is not None:
            delta = float(ks_delta(sigma)) if callable(ks_delta) else float(ks_delta)
        means = np.array([mu - delta, mu, mu + delta])
        return self.engine.viterbi_groups(x_local, chr_start, groups_local, means, [sigma] * len(groups_local),
                                          np.log(Pi), np.log(d0))

    def run_i6(self, x_local, chr_start, groups_local, means, sd_per_group, logPi, logDelta):
        """predict_CNV_via_HMM_on_tumor_subclusters (R/inferCNV_HMM.R:345-408): no exchange at all."""
        return self.engine.viterbi_groups(x_local, chr_start, groups_local, means, sd_per_group, logPi, logDelta)


class ShardedMedianFilter:
    """apply_median_filtering (R/noise_reduction.R:43-113) on a cell-sharded matrix whose tiles are whole on their ranks:
    rank-local, no collective.  na_aware=True gives R's NA result (device.median_filter): a rank whose shard holds no NaN
    takes the plain launches, one that holds some takes the cleaned copy -- the filter has no collective and a window never
    leaves its tile, so every rank may decide for itself."""

    def __init__(self, engine=None):
        self.engine = engine or DeviceGroupEngine()

    def run(self, x_local, chr_start, tiles_local, window_size=7, na_aware=False):
        if na_aware:      # (an engine without the keyword refuses: no silent fall-back to the plain filter)
            return self.engine.median_filter(x_local, chr_start, tiles_local, window_size, na_aware=True)
        return self.engine.median_filter(x_local, chr_start, tiles_local, window_size)


class ShardedIngest:
    """Steps 2-4 of run() from integer counts on cell shards.  Exchange steps:
        all-reduce(sum) of [G gene sums | G numbers of expressing cells]   -> the filter decision, identical on every rank
        all-gather of the ranks' column sums over the kept genes          -> median(colSums) = the normalisation factor
    `engine` has gene_stats(counts) -> 2G vector, col_sums(counts, keep) -> C_local vector and apply(counts, keep, col_sums,
    factor) -> matrix; the default one runs on libicnv_hip.so (device.ingest_*)."""

    def __init__(self, engine=None, process_group=None):
        self.engine = engine
        self.pg = process_group

    def run(self, counts_local, C_total, min_mean_expr_cutoff=None, min_cells_per_gene=0, normalize_factor=None):
        import torch
        import torch.distributed as dist
        multi = dist.is_available() and dist.is_initialized() and dist.get_world_size(self.pg) > 1
        eng = self.engine
        if eng is None:
            from . import device as eng_mod
            class _Dev:
                gene_stats = staticmethod(eng_mod.ingest_gene_stats)
                col_sums = staticmethod(eng_mod.ingest_col_sums)
                apply = staticmethod(eng_mod.ingest_apply)
                select = staticmethod(eng_mod.ingest_select)
            eng = _Dev
        stats = eng.gene_stats(counts_local)
        if multi:
            dist.all_reduce(stats, op=dist.ReduceOp.SUM, group=self.pg)
        stats_h = stats.cpu().numpy() if hasattr(stats, "cpu") else np.asarray(stats)
        G = stats_h.size // 2
        keep = eng.select(stats_h, G, C_total, min_mean_expr_cutoff, min_cells_per_gene)
        cs = eng.col_sums(counts_local, keep)
        factor = normalize_factor
        if factor is None:
            if multi:
                world = dist.get_world_size(self.pg)
                n_local = torch.tensor([cs.numel()], dtype=torch.int64, device=cs.device)
                sizes = [torch.zeros_like(n_local) for _ in range(world)]
                dist.all_gather(sizes, n_local, group=self.pg)
                nmax = int(max(int(v.item()) for v in sizes))
                pad = torch.zeros(nmax, dtype=cs.dtype, device=cs.device)
                pad[: cs.numel()] = cs
                parts = [torch.zeros_like(pad) for _ in range(world)]
                dist.all_gather(parts, pad, group=self.pg)
                allcs = np.concatenate([p[: int(n.item())].cpu().numpy() for p, n in zip(parts, sizes)])
            else:
                allcs = cs.cpu().numpy() if hasattr(cs, "cpu") else np.asarray(cs)
            factor = float(np.median(allcs))              # stats::median: mean of the two middle values for an even count
        return eng.apply(counts_local, keep, cs, factor), keep, factor


# ---------------------------------------------------------------------------------------------------------------------
# From files to a rank's cells (DESIGN K26): CreateInfercnvObject for one rank.  Every rank reads the whole file's bytes and
# converts its own columns only (device.read_table / read_mtx with cells=); the one exchange is the all-gather of the column
# sums, from which every rank takes the same cell filter and the same down-sampling.
def _table_columns(path, sep):
    """The column names of a text table as device.read_table takes them: the header line has one name per numeric column, or
    one more with a corner label in front; the first data line decides which."""
    import os
    from . import device
    path = os.fspath(path)
    if path.endswith(".rds"):
        raise NotImplementedError("read_table: .rds input is not read; pass the matrix as an array")
    sep_b = sep if isinstance(sep, bytes) else str(sep).encode("utf-8")
    with device._open_text(path) as f:
        header = f.readline().rstrip(b"\n")
        first = next((raw for raw in (line.rstrip(b"\n") for line in f) if raw not in (b"", b"\r")), None)
    return [c.decode("utf-8", "surrogateescape") for c in device._table_columns(header, first, sep_b)]


class ShardedCreate:
    """CreateInfercnvObject (create_object.py) for rank `rank` of `world`: the formals of CreateInfercnvObject without
    return_device, and keyword-only after ref_group_names
        rank, world     this rank and the number of ranks
        deal            "cyclic" (cyclic_cells) or "block" (shard_bounds) of the FILE's columns
        process_group   the torch.distributed group of run()'s all-gather
        reader          (path, cells) -> (gene names, ALL cell names, the (len(cells), G) array of file columns `cells`, or
                        for a .mtx / 10x source the G x len(cells) scipy CSC); replaces device.read_table / read_mtx, and the
                        matrix work then runs in NumPy / SciPy -- the host logic without a GPU.
    The matrix is a file: a text table, a .mtx, a 10x directory, or an R file (.rds, .rda / .RData: DESIGN K34 -- the column count
    comes from rds.locate_counts, the rank's columns from device.read_rds_counts(cells=)).  Two phases around one exchange:
        read()              header or size line, gene order, annotations -- CreateInfercnvObject's checks in its order --, the
                            deal (world > the file's columns: ValueError before the body is read), this rank's columns parsed,
                            .order_reduce; returns the column sums of its columns over the kept genes, in the order of the deal
        finish(sums_all)    the sums of ALL file columns in file order -> select_cells with the same seed, so the same global
                            `columns` on every rank; the rank keeps J = [j : columns[j] is its own], ascending, and returns
                            (obj_local, x_local, shard): the InfercnvObject over those cells (group dicts of LOCAL indices,
                            order within a group preserved, every other slot the single-rank object's), what
                            CreateInfercnvObject(return_device=True) hands back for these cells, and
                            {"global_index": J, "file_columns": columns[J], "C_total", "rank", "world", "deal"}
        run()               read(), the all-gather of the padded sums placed into file order by the deal, finish(); without an
                            initialised process group the one-rank case, equal to CreateInfercnvObject slot for slot."""

    def __init__(self, raw_counts_matrix, gene_order_file, annotations_file, ref_group_names, *, rank, world, deal="cyclic",
                 process_group=None, reader=None, delim="\t", max_cells_per_group=None, min_max_counts_per_cell=(100, float("inf")),
                 chr_exclude=("chrX", "chrY", "chrM"), seed=0, gene_names=None, cell_names=None, chunk_bytes=None, sparse=None,
                 gene_column=2):
        if deal not in ("cyclic", "block"):
            raise ValueError("deal must be 'cyclic' or 'block'")
        rank, world = int(rank), int(world)
        if world < 1 or not 0 <= rank < world:
            raise ValueError("rank must be 0 .. world - 1")
        self.args = dict(raw_counts_matrix=raw_counts_matrix, gene_order_file=gene_order_file, annotations_file=annotations_file,
                         ref_group_names=ref_group_names, delim=delim, max_cells_per_group=max_cells_per_group,
                         min_max_counts_per_cell=min_max_counts_per_cell, chr_exclude=chr_exclude,
                         seed=seed, gene_names=gene_names, cell_names=cell_names, chunk_bytes=chunk_bytes, sparse=sparse,
                         gene_column=gene_column)
        self.rank, self.world, self.deal, self.pg, self.reader = rank, world, deal, process_group, reader
        self._read = None

    def dealt(self, C_file, rank=None):
        """The file columns of `rank` (default: this rank), in the order of the deal."""
        rank = self.rank if rank is None else rank
        if self.deal == "cyclic":
            return cyclic_cells(C_file, self.world, rank)
        c0, c1 = shard_bounds(C_file, self.world, rank)
        return np.arange(c0, c1, dtype=np.int64)

    def read(self):
        import os
        from . import create_object as co
        a = self.args
        positions = co.read_gene_order(a["gene_order_file"], a["chr_exclude"])
        annotations = co.read_annotations(a["annotations_file"], a["delim"])
        raw = a["raw_counts_matrix"]
        if not isinstance(raw, (str, os.PathLike)):
            raise ValueError("ShardedCreate reads the matrix from a file: a text table, a .mtx file, a 10x directory or an .rds / .rda file")
        rds_path = co._rds_source(raw)
        mtx = None if rds_path is not None else co._mtx_source(raw, a["gene_names"], a["cell_names"], a["gene_column"])
        if rds_path is not None:                                         # K34: the shape is in the stream's attributes
            from . import rds
            names = co._rds_names(a["gene_names"], a["cell_names"], a["gene_column"])
            opened = rds.open_counts(rds_path, device=self.reader is None)
            located = rds.locate_counts(opened[0], **names)
            if a["sparse"] and located.kind != "dgCMatrix":
                raise ValueError("sparse=True wants a .mtx file, a 10x directory or a scipy sparse matrix")
            C_file = located.C
        elif mtx is None and a["sparse"]:
            raise ValueError("sparse=True wants a .mtx file, a 10x directory or a scipy sparse matrix")
        elif mtx is not None:                                            # the size line
            from .device import _mtx_header, _open_text
            with _open_text(mtx[0]) as f:
                _, G_file, C_file, _, _, _ = _mtx_header(f)
        else:                                                            # the header line
            C_file = len(_table_columns(raw, a["delim"]))
        if self.world > C_file:
            raise ValueError(f"world is {self.world}, but the file has only {C_file} columns")
        mine = self.dealt(C_file)
        counts = x = None
        if rds_path is not None:
            if self.reader is not None:
                genes, cells, got = self.reader(rds_path, mine)
                sparse_kind = hasattr(got, "tocsc")
            else:
                from . import device
                genes, cells, got, _ = device.read_rds_counts(rds_path, cells=mine, chunk_bytes=a["chunk_bytes"], opened=opened, **names)
                sparse_kind = isinstance(got, device.DeviceCounts)
            rds.close_counts(opened[0])
            del opened
            if sparse_kind and a["sparse"] is False:
                x = np.ascontiguousarray(got.toarray().T) if self.reader is not None else got.to_dense()
            elif sparse_kind:
                counts = got
            else:
                x = got
        elif mtx is not None:
            genes, cells = mtx[1], mtx[2]
            if self.reader is not None:
                _, _, counts = self.reader(mtx[0], mine)
            else:
                from . import device
                counts, _ = device.read_mtx(mtx[0], chunk_bytes=a["chunk_bytes"], cells=mine)
            if (G_file, C_file) != (len(genes), len(cells)):
                raise ValueError(f"the matrix is {G_file} x {C_file}, but there are {len(genes)} gene names and {len(cells)} cell names")
            if a["sparse"] is False:
                counts, x = None, (np.ascontiguousarray(counts.toarray().T) if self.reader is not None else counts.to_dense())
        elif self.reader is not None:
            genes, cells, x = self.reader(raw, mine)
        else:
            from . import device
            genes, cells, x, _ = device.read_table(raw, sep=a["delim"], chunk_bytes=a["chunk_bytes"], cells=mine)
        genes, cells = [str(g) for g in genes], [str(c) for c in cells]
        if co._first_duplicate(genes) is not None:
            raise ValueError(f"{co.ERR_DUP_ROW_NAMES} ({co._first_duplicate(genes)!r})")
        co.check_annotated_cells(cells, annotations)
        rows, chrs, start, stop = co.order_reduce(genes, positions)
        if rows is None:
            raise ValueError(co.ERR_NO_GENES)
        if self.reader is not None:
            if counts is not None:
                sums = np.asarray(counts.tocsr()[rows].sum(axis=0), dtype=np.float64).ravel()
            else:
                x = np.ascontiguousarray(np.asarray(x, dtype=np.float64)[:, rows])
                sums = x.sum(axis=1)
        else:
            from . import device
            if counts is not None:
                sums = device.ingest_col_sums(counts, rows).cpu().numpy()
            else:
                x = device.gather_matrix(x, genes=rows)
                sums = device.col_sums(x).cpu().numpy()
        self._read = dict(annotations=annotations, genes=genes, cells=cells, rows=rows, chrs=chrs, start=start, stop=stop, mine=mine,
                          C_file=C_file, counts=counts, x=x)
        return sums

    def finish(self, col_sums_all):
        from . import create_object as co
        from .infercnv_object import GeneOrder, InfercnvObject
        if self._read is None:
            raise RuntimeError("finish() comes after read()")
        r, a = self._read, self.args
        cs = np.asarray(col_sums_all, dtype=np.float64).ravel()
        if cs.size != r["C_file"]:
            raise ValueError(f"col_sums_all has {cs.size} entries, the file has {r['C_file']} columns")
        columns, _, ref, obs = co.select_cells(r["cells"], cs, r["annotations"], a["ref_group_names"], a["min_max_counts_per_cell"],
                                               a["max_cells_per_group"], a["seed"])
        if columns.size == 0:
            raise ValueError("no cell is left after the counts-per-cell filter and the annotations")
        local_of = np.full(r["C_file"], -1, dtype=np.int64)
        local_of[r["mine"]] = np.arange(r["mine"].size)
        J = np.flatnonzero(local_of[columns] >= 0)
        if J.size == 0:
            raise ValueError(f"no cell is left on rank {self.rank} of {self.world} after the counts-per-cell filter and the annotations")
        keep = local_of[columns[J]]                                      # this rank's columns that stay, in the global order
        counts, x, rows = r["counts"], r["x"], r["rows"]
        if counts is not None:
            if self.reader is not None:
                x_local = counts.tocsr()[rows].tocsc()[:, keep]
                expr = x_local
            else:
                from . import device
                x_local = device.csc_select(counts, rows, keep)
                expr = x_local.to_scipy()
        elif self.reader is not None:
            x_local = np.ascontiguousarray(x[keep])
            expr = x_local.T
        else:
            from . import device
            x_local = x if (keep.size == x.shape[0] and np.array_equal(keep, np.arange(keep.size))) else device.gather_matrix(x, cells=keep)
            expr = x_local.cpu().numpy().T
        localize = lambda groups: {name: np.searchsorted(J, idx[np.isin(idx, J)]).astype(np.int32) for name, idx in groups.items()}
        obj = InfercnvObject(expr_data=expr, count_data=expr,
                             gene_order=GeneOrder(chr=np.array(r["chrs"]), start=np.array(r["start"]), stop=np.array(r["stop"])),
                             reference_grouped_cell_indices=localize(ref), observation_grouped_cell_indices=localize(obs),
                             options={"chr_exclude": list(a["chr_exclude"]) if a["chr_exclude"] is not None else None,
                                      "max_cells_per_group": a["max_cells_per_group"],
                                      "min_max_counts_per_cell": list(a["min_max_counts_per_cell"]) if a["min_max_counts_per_cell"] is not None
                                      else None,
                                      "counts_md5": None},
                             gene_names=np.array([r["genes"][g] for g in rows]), cell_names=np.array([r["cells"][j] for j in columns[J]]))
        obj.validate()
        shard = {"global_index": J, "file_columns": columns[J], "C_total": int(columns.size), "rank": self.rank, "world": self.world,
                 "deal": self.deal}
        return obj, x_local, shard

    def place(self, parts):
        """The ranks' sums (parts[r] in the order of rank r's deal) as one vector in file order."""
        C_file = int(sum(len(p) for p in parts))
        out = np.empty(C_file, dtype=np.float64)
        for rank, p in enumerate(parts):
            out[self.dealt(C_file, rank)] = np.asarray(p, dtype=np.float64)
        return out

    def run(self):
        import torch
        import torch.distributed as dist
        sums = self.read()
        if not (dist.is_available() and dist.is_initialized() and dist.get_world_size(self.pg) > 1):
            if self.world != 1:
                raise RuntimeError(f"world is {self.world} but no process group is initialised: exchange the sums yourself and call finish()")
            return self.finish(sums)
        world = dist.get_world_size(self.pg)
        if world != self.world:
            raise ValueError(f"world is {self.world}, the process group has {world} ranks")
        dev = "cuda" if dist.get_backend(self.pg) == "nccl" else "cpu"
        cs = torch.from_numpy(np.ascontiguousarray(sums, dtype=np.float64)).to(dev)
        n_local = torch.tensor([cs.numel()], dtype=torch.int64, device=cs.device)         # the size exchange of ShardedIngest.run
        sizes = [torch.zeros_like(n_local) for _ in range(world)]
        dist.all_gather(sizes, n_local, group=self.pg)
        nmax = int(max(int(v.item()) for v in sizes))
        pad = torch.zeros(nmax, dtype=cs.dtype, device=cs.device)
        pad[: cs.numel()] = cs
        parts = [torch.zeros_like(pad) for _ in range(world)]
        dist.all_gather(parts, pad, group=self.pg)
        return self.finish(self.place([p[: int(n.item())].cpu().numpy() for p, n in zip(parts, sizes)]))
