/*
 * icnv.h -- C ABI of libicnv_hip.so: inferCNV's expression-smoothing chain,
 * i6/i3 HMM Viterbi and 2-D median denoise as hand-written HIP kernels for
 * AMD MI355X (gfx950).
 *
 * The reference (broadinstitute/infercnv, pure R, NeedsCompilation: no) has no
 * FFI layer; the boundary this library sits behind is the step-function
 * contract of infercnv::run()  f(infercnv_obj, scalars) -> infercnv_obj  on
 * infercnv_obj@expr.data (R/inferCNV_ops.R:771,817,865,911,952,1031,
 * 1255-1304,1469-1471,1573-1588; scripts/inferCNV.R:1116).  Each entry point
 * below names the reference function(s) it replaces.  INTEGRATION.md shows
 * the R-side .Call shim and the Python ctypes binding.
 *
 * Conventions
 *   - Matrices are column-major genes x cells, element (g, c) at x[g + G*c]:
 *     exactly R's layout of expr.data (R/inferCNV.R:18) and at the same time
 *     the "cell-major" HBM layout (one cell's genes are contiguous).
 *   - All indices are 0-based int32.  Genes of one chromosome are contiguous
 *     (.order_reduce, R/inferCNV.R:407): chr_start[] holds n_chr+1 offsets,
 *     chr_start[0] = 0, chr_start[n_chr] = G.
 *   - Group lists are "packed": idx[] concatenates the member cell indices of
 *     all groups, off[] holds n_grp+1 offsets into idx[].
 *   - Every function returns ICNV_OK (0) or an error code; the message is
 *     available from icnv_last_error() (thread-local).  The library never
 *     longjmps/aborts: an R shim turns codes into stop() after cleanup.
 *   - *_dev entry points take DEVICE pointers for matrices/outputs and enqueue
 *     all work on `stream` (a hipStream_t passed as void*, NULL = default
 *     stream) without synchronising the host.  Small descriptor arrays
 *     (chr_start, group lists, HMM parameters) are HOST pointers in both
 *     flavours and are copied to the device by the library.
 *   - The host-buffer flavours upload, run the *_dev path and download.
 *   - Caller owns every buffer it passes; inputs are never modified.
 *   - Threading: every call acts on the calling thread's current HIP device (icnv_init selects it).  Library state
 *     (workspace pool, emission-table cache, Viterbi statistics) is kept per device and guarded by mutexes, so
 *     threads driving DIFFERENT devices may call concurrently.  On one device use ONE stream at a time: scratch
 *     buffers return to the device's pool when a *_dev call returns while its kernels may still be queued, and the
 *     next call's work must be ordered behind them (same stream, or a stream the caller has made wait).
 */
#ifndef ICNV_H
#define ICNV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ICNV_OK 0
#define ICNV_ERR_ARG 1        /* invalid argument                                   */
#define ICNV_ERR_HIP 2        /* HIP runtime error (message has the hipError string) */
#define ICNV_ERR_UNSUPPORTED 3 /* size/config outside what the kernels support        */
#define ICNV_ERR_UNDERFLOW 4  /* "Problems With Underflow" (R/inferCNV_HMM.R:1165)   */
#define ICNV_ERR_NOMEM 5

/* Stages of the smoothing chain, named by run()'s step numbers
 * (R/inferCNV_ops.R:771-1589).  Stages always execute in this order. */
#define ICNV_ST_SUBTRACT_REF_1 0x01u /* step  8 subtract_ref_expr_from_obs       :1678-1786 */
#define ICNV_ST_MAX_THRESH     0x02u /* step  9 apply_max_threshold_bounds       :2970-2983 */
#define ICNV_ST_SMOOTH         0x04u /* step 10 smooth_by_chromosome             :2406-2532 */
#define ICNV_ST_CENTER         0x08u /* step 11 center_cell_expr_across_chromosome (median) :2074-2109 */
#define ICNV_ST_SUBTRACT_REF_2 0x10u /* step 12 subtract_ref_expr_from_obs (again)         */
#define ICNV_ST_INVERT_LOG2    0x20u /* step 14 invert_log2                      :2814-2826 */
#define ICNV_ST_DENOISE        0x40u /* step 22 clear_noise_via_ref_mean_sd / clear_noise :2232-2346 */
#define ICNV_ST_ALL            0x7Fu
#define ICNV_ST_CENTER_MEAN    0x80u /* modifier: step 11 subtracts the mean instead of the median */
#define ICNV_ST_NA_AWARE       0x100u /* modifier: the matrix may hold NA / NaN.  The cells that do are recomputed with the reference's
                                         NA semantics (csrc/chain_na.hip: step 8 / 12 with bounds turn an NA into 0, the smoothing strips
                                         and re-inserts NAs per chromosome, the centre is taken over the values present,
                                         R/inferCNV_ops.R:1757-1768, 2098, 2487-2489, 2529); costs one extra pass over the input.  Without
                                         it a NaN is not looked for (run()'s chain input, log2(x + 1) of counts, has none).  Any gene count
                                         (fused, two-pass and three-pass chain); a call that runs in place keeps the flagged cells'
                                         input columns aside first (fused chain; ICNV_ERR_UNSUPPORTED in place beyond the LDS-resident
                                         limit); ICNV_ERR_UNSUPPORTED together with inv_log or noise_logistic (no silent default) */

/* ---- library state ------------------------------------------------------ */
int icnv_version(void);
const char *icnv_last_error(void);
/* Selects the HIP device for the calling thread's subsequent calls (-1 = keep
 * current).  Fails with ICNV_ERR_HIP when no gfx950-class GPU is usable. */
int icnv_init(int device);
/* Frees cached device workspaces. */
void icnv_shutdown(void);

/* Devices of the HOST-BUFFER entry points (the ones an R process reaches through the .Call shim).  n_devices = 0: every
 * visible device, n: devices 0 .. n-1, 1 (the default): the calling thread's current device.  With more than one device
 * icnv_smooth_chain and icnv_viterbi_cells split the cells into one contiguous block per device (one host thread, one
 * stream per device); the chain's reference statistics (per-gene sums of the reference groups) are added
 * on the host in device order.  icnv_viterbi_groups and icnv_median_filter deal WHOLE groups / tiles to the devices
 * (longest first onto the least loaded one; every worker packs the columns of its groups' cells, no exchange between
 * devices).  The remaining host-buffer entry points run on the current device.  This is what lets a
 * single R process (infercnv::run() is single-threaded) use the 8 GPUs of a node, each over its own PCIe link.
 * The *_dev entry points are not affected: a device-resident caller (one process per GPU, infercnv_amd/sharded.py)
 * shards by itself. */
int icnv_set_devices(int n_devices);
int icnv_get_devices(void);

/* Residency of the host-buffer entry points.  run() hands every step the matrix the previous step returned
 * (R/inferCNV_ops.R:771-1031, 1237-1309).  With icnv_residency(1) the library keeps the matrices it uploaded or
 * produced on the device(s) -- up to 6 per device, ICNV_RESIDENT_MAX_GB (default 64), given back under memory
 * pressure -- and recognises a host matrix BY CONTENT: its length, a strided sample of ~16 000 values as the quick
 * reject, then a 64-bit hash of every value (the host's cores hash the incoming matrix at memory speed, several times
 * faster than the upload it saves; a device reduction hashes what the library produced).  A recognised matrix is not
 * uploaded again.  Addresses play no part: the caller may free, reuse or edit host memory at any time -- one changed
 * element changes the hash and the matrix is uploaded (the hash is linear inside a 64-byte block: an edit of ONE word is
 * always seen; edits of several words of one block cancel only if sum_j delta_j K_j = 0 mod 2^64, odds 2^-64 for unrelated
 * data).  Whether it pays depends on the host: the hash is one pass over the matrix by the cores the process may use, the
 * upload it saves is one pass by the DMA engines at PCIe speed -- on a 16-core quota the two are about even (the bench
 * line's `host_path` shows both, with the phase times of icnv_host_path_stats).  Off by default, also in the R glue.
 *   icnv_residency_stats  out4 = {matrices recognised, matrices uploaded, resident bytes, resident matrices} */
int icnv_residency(int on);
void icnv_residency_drop(void);
int icnv_residency_stats(int64_t *out4);

/* Where a host-buffer call spends its time (wall-clock milliseconds accumulated since the last reset, per process):
 *   out[0] calls            host-buffer entry points that moved a matrix
 *   out[1] fingerprint_ms   residency: strided samples of incoming matrices
 *   out[2] hash_ms          residency: full content hashes on the host's cores        out[3] hash_threads (of the last hash)
 *   out[4] h2d_ms           time the uploading thread was busy                         out[5] h2d_bytes
 *   out[6] d2h_ms           time the downloading thread was busy                       out[7] d2h_bytes
 *   out[8] device_ms        waiting for the kernels alone (not overlapped with a copy)
 *   out[9] pipelined_calls  calls that ran the three-thread pipeline (upload | kernels | download of column blocks)
 *   out[10] wall_ms         whole calls, entry to return
 *   out[11] alloc_ms        hipMalloc inside the calls (the workspace pool is grow-only: zero in the steady state; with
 *                           residency on, the first calls after a change of shape allocate what the residents hold)
 * n = number of doubles the caller's buffer holds (<= 12 are written).  icnv_host_path_stats_reset() zeroes them.
 * The smoothing chain and the per-cell Viterbi on ONE device pipeline their transfers over column blocks when
 * residency is off (the reference cells' blocks first: the chain's statistics need them before any block can be
 * finished): uploads, kernels and downloads overlap on three streams driven by three host threads, because a copy from
 * or to pageable memory -- what R hands over -- occupies the thread that issues it.  ICNV_HOST_PIPELINE=0 switches it off. */
int icnv_host_path_stats(double *out, int32_t n);
void icnv_host_path_stats_reset(void);

/* ---- smoothing chain ---------------------------------------------------- */
typedef struct icnv_chain_cfg {
    int64_t G;               /* genes                                              */
    int64_t C;               /* cells in this (local) matrix                       */
    const int32_t *chr_start; /* HOST, n_chr+1 offsets                              */
    int32_t n_chr;
    int32_t window_length;   /* odd; < 2 = no smoothing (R/inferCNV_ops.R:2444)    */
    double max_thresh;       /* step 9 threshold; NaN = skip                       */
    int32_t use_bounds;      /* steps 8/12: 1 = min/max-of-group-means bounds      */
    int32_t inv_log;         /* subtract_ref_expr_from_obs(inv_log = TRUE): group means as log2(mean(2^x - 1) + 1)
                                (R/inferCNV_ops.R:1714-1717).  run() never sets it (:771, :952), so it is the
                                stand-alone step only: stage_mask must be ICNV_ST_SUBTRACT_REF_1 alone.  Sits in
                                the padding after use_bounds: zero-initialised configurations keep their meaning */
    double sd_amplifier;     /* step 22 (clear_noise_via_ref_mean_sd)              */
    double noise_filter;     /* step 22: NaN = sd-based; else clear_noise(threshold) */
    uint32_t stage_mask;     /* ICNV_ST_* bits                                     */
    int32_t noise_logistic;  /* step 22 with noise_logistic = TRUE (R/inferCNV_ops.R:2249-2252, 2326-2330;
                                .apply_logistic_val_adj, R/inferCNV_heatmap.R:2791-2810): instead of the select,
                                x <- m +- p |x - m|, p = 1 / (1 + exp(-20 (|x - m| - s))), m and s = the select's centre
                                and half width.  Sits in the padding after stage_mask: zero-initialised
                                configurations keep their meaning */
    const int32_t *ref_idx;  /* HOST packed LOCAL reference cell indices (or, with */
    const int32_t *ref_off;  /* no references, one group of all observation cells, */
    int32_t n_ref_grp;       /* R/inferCNV_ops.R:1686-1688); HOST n_ref_grp+1      */
} icnv_chain_cfg;

/* One-call form, host buffers.  Replaces the R functions listed at the
 * ICNV_ST_* bits; with stage_mask = a single bit it is the stand-alone step
 * (so run(up_to_step=), resume files and the .hspike mirror keep working).
 * pre_denoise (nullable) receives the matrix before step 22 (the HMM's input,
 * R/inferCNV_ops.R:1237-1309 reads the step-14..16 object). */
int icnv_smooth_chain(const double *expr_in, double *expr_out, double *pre_denoise,
                      const icnv_chain_cfg *cfg);
/* Same with device-resident matrices; expr_out may alias expr_in. */
int icnv_smooth_chain_dev(const double *expr_in, double *expr_out, double *pre_denoise,
                          const icnv_chain_cfg *cfg, void *stream);

/* Split-phase form for cell-sharded multi-GPU runs (one process per GPU).
 * The chain has one "reference round" per reference-dependent stage present
 * in stage_mask (steps 8, 12, 22, in that order).  For round r the caller
 *   1. icnv_chain_round_partial_dev(): enqueues this rank's partial statistic
 *      over its LOCAL reference cells into a device buffer of *n doubles --
 *      subtract rounds: [G*n_ref_grp gene sums | n_ref_grp cell counts],
 *      denoise round:   [sum x, sum_c sd_c, n_ref_cells, n_ref_values];
 *   2. all-reduces (sum) that buffer across ranks (RCCL; nothing to do on 1 GPU);
 *   3. icnv_chain_round_finish_dev(): turns the reduced buffer into the
 *      stage's parameters (bounds / mu,s) on the device.
 * Then icnv_chain_apply_dev() streams every local cell through the fused pass.
 * The rounds and the apply must be given the SAME matrix (expr_in, unchanged in between): the round that
 * first smooths the reference cells keeps its output (one column per reference cell), and the later rounds and
 * the apply continue from it instead of smoothing those cells again.  The kept columns are tied to the expr_in
 * pointer and consumed by the apply; an apply without fresh rounds recomputes every cell from expr_in with the
 * parameters of the last rounds. */
typedef struct icnv_chain icnv_chain_t;
int icnv_chain_begin(icnv_chain_t **chain, const icnv_chain_cfg *cfg);
int icnv_chain_num_rounds(const icnv_chain_t *chain);
int icnv_chain_round_partial_dev(icnv_chain_t *chain, int round, const double *expr_in,
                                 double **partial_dev, int64_t *n, void *stream);
int icnv_chain_round_finish_dev(icnv_chain_t *chain, int round, void *stream);
int icnv_chain_apply_dev(icnv_chain_t *chain, const double *expr_in, double *expr_out,
                         double *pre_denoise, void *stream);
/* The same with a LEADING DIMENSION for the HMM input: column c of pre_denoise starts at pre_denoise + c * ld_pre (ld_pre >= G;
 * 0 or G: contiguous columns, the R layout).  A multiple of 16 puts every column on a cache line of its own, which is what
 * icnv_viterbi_cells_ld_dev reads fastest when G is not a multiple of 16 (every real, filtered gene set).  Device-resident
 * pipelines only -- an R matrix is contiguous; the host-buffer entry points pad on upload by themselves.  Fused chain with
 * step 22 only (ICNV_ERR_UNSUPPORTED otherwise).  Replaces nothing in the reference: a layout option of this library. */
int icnv_chain_apply_ld_dev(icnv_chain_t *chain, const double *expr_in, double *expr_out,
                            double *pre_denoise, int64_t ld_pre, void *stream);
/* Copies {mu, s} of the denoise stage to the host (synchronises the stream). */
int icnv_chain_get_denoise(icnv_chain_t *chain, double *mu_s, void *stream);
void icnv_chain_end(icnv_chain_t *chain);

/* get_average_bounds (R/inferCNV_ops.R:2723-2742): out2 = {mean_c min_g x,
 * mean_c max_g x}; threshold "auto" of step 9 is mean(abs(out2)).  NaN entries are skipped per cell (quantile(x,
 * na.rm = TRUE)); a cell that holds nothing but NaN makes both bounds NaN, as R's mean() over an NA does. */
int icnv_average_bounds(const double *expr, int64_t G, int64_t C, double *out2);
int icnv_average_bounds_dev(const double *expr, int64_t G, int64_t C, double *out2_host, void *stream);

/* scale_infercnv_expr (step 5 of run(), scale_data, off by default; R/inferCNV_ops.R:3174-3185): t(scale(t(x))) -- every
 * gene minus its mean over the cells, divided by sqrt(sum(centred^2) / max(1, C - 1)) (a constant gene becomes NaN, as in R).
 * expr_out may alias expr_in in the _dev form. */
int icnv_scale_genes(const double *expr_in, double *expr_out, int64_t G, int64_t C);
int icnv_scale_genes_dev(const double *expr_in, double *expr_out, int64_t G, int64_t C, void *stream);

/* remove_outliers_norm (step 16 of run(), R/inferCNV_ops.R:1969-2054; between the chain and the HMM when prune_outliers
 * is set): values below / above the bounds are set to the bounds.  Both bounds given (not NaN) = hard thresholds
 * (:2017-2022); otherwise out_method = "average_bound", the bounds of icnv_average_bounds over the input (:2029-2033).
 * bounds_used2 (nullable, host) receives {lower, upper}.  expr_out may alias expr_in in the _dev form.  NaN average
 * bounds (a cell of nothing but NaN) are passed on, not refused: bounds_used2 = {NaN, NaN} and the matrix is copied
 * unchanged, which is what R's two assignments do with an NA bound (an NA subscript assigns nothing). */
int icnv_remove_outliers(const double *expr_in, double *expr_out, int64_t G, int64_t C, double lower_bound, double upper_bound,
                         double *bounds_used2);
int icnv_remove_outliers_dev(const double *expr_in, double *expr_out, int64_t G, int64_t C, double lower_bound,
                             double upper_bound, double *bounds_used2, void *stream);

/* ---- ingest from the raw COUNT matrix: steps 2, 3, 4 of run() in one call ------------------
 * Replaces require_above_min_mean_expr_cutoff + require_above_min_cells_ref (R/inferCNV_ops.R:2128-2213; run() :560-566),
 * normalize_counts_by_seq_depth (:3064-3111) and log2xplus1 (:2756-2769).  The counts cross PCIe once as integers --
 * dense int32 (G x C column-major) or CSC (colptr [C + 1], rowidx / vals [nnz]; 0-based, any order inside a column) --
 * and the f64 matrix of the KEPT genes (G_out x C) is formed on the device.  Integer sums are exact: the result is bit
 * for bit what icnv_gene_stats + icnv_select_genes + icnv_normalize_log2 give on the f64 copy of the counts.
 *   min_mean_expr_cutoff  NaN: no filter; a gene with rowMeans(counts) < cutoff is removed
 *   min_cells_per_gene    <= 0: no filter; a gene needs counts > 0 in at least that many cells
 *   normalize_factor      NaN: median(colSums) over the kept genes (the reference's default, normalize_factor = NA)
 *   keep_idx [G], G_out   the kept genes (ascending, 0-based) and their number; "All genes removed" is an error (:2194)
 *   expr_out              capacity G x C doubles, filled G_out x C; h2d_bytes (nullable): bytes uploaded
 * CSC: a (gene, cell) pair may be stored at most once (explicitly stored zeros are fine).  Duplicates are NOT detected:
 * the statistics and the column sums would add them, apply would keep one of them. */
typedef struct icnv_counts {
    const int32_t *dense;    /* dense form, or NULL */
    const int64_t *colptr;   /* CSC form, or NULL */
    const int32_t *rowidx;
    const int32_t *vals;
    int64_t nnz;             /* CSC: stored entries */
} icnv_counts;
int icnv_ingest_counts(const icnv_counts *cnt, int64_t G, int64_t C, double min_mean_expr_cutoff, int32_t min_cells_per_gene,
                       double normalize_factor, int32_t *keep_idx, int64_t *G_out, double *expr_out, double *factor_used,
                       int64_t *h2d_bytes);
/* The same with the count arrays and the output already on the device (keep_idx stays a host array). */
int icnv_ingest_counts_dev(const icnv_counts *cnt, int64_t G, int64_t C, double min_mean_expr_cutoff, int32_t min_cells_per_gene,
                           double normalize_factor, int32_t *keep_idx_host, int64_t *G_out, double *expr_out_dev,
                           double *factor_used, void *stream);
/* Split phases for a cell-sharded caller (infercnv_amd/sharded.py: ShardedIngest):
 *   gene_stats   stats2G_dev = [G sums of the counts | G numbers of cells with count > 0] as doubles -> all-reduce(sum);
 *                a negative entry (R's NA_integer_ is INT_MIN) is ICNV_ERR_ARG: counts must be >= 0
 *   select       the filter decision from the all-reduced statistics (host arithmetic, the same on every rank)
 *   col_sums     colSums over the kept genes (keep_mask_dev: G bytes, 1 = kept)     -> all-gather, median = the factor
 *   apply        expr_out[j, c] = log2(count[keep[j], c] / col_sum[c] * factor + 1), the reference's operation order */
int icnv_ingest_gene_stats_dev(const icnv_counts *cnt, int64_t G, int64_t C, double *stats2G_dev, void *stream);
int icnv_ingest_select(const double *stats2G_host, int64_t G, int64_t C_total, double min_mean_expr_cutoff, int32_t min_cells_per_gene,
                       int32_t *keep_idx, int64_t *G_out);
int icnv_ingest_col_sums_dev(const icnv_counts *cnt, int64_t G, int64_t C, const uint8_t *keep_mask_dev, double *col_sums_dev, void *stream);
int icnv_ingest_apply_dev(const icnv_counts *cnt, int64_t G, int64_t C, const int32_t *keep_idx_dev, int64_t G_out,
                          const double *col_sums_dev, double factor, int32_t do_normalize, int32_t do_log2, double *expr_out,
                          void *stream);

/* ---- ingest: steps 3 and 4 of run() (first "next" row) -------- */
/* colSums(expr.data) per cell (R/inferCNV_ops.R:3089), device pointers. */
int icnv_col_sums_dev(const double *expr, int64_t G, int64_t C, double *sums_dev, void *stream);
/* normalize_counts_by_seq_depth (R/inferCNV_ops.R:3064-3111): x / colSum * factor, and
 * log2xplus1 (:2756-2769): log2(x + 1); either part can be switched off. */
int icnv_normalize_log2_dev(const double *expr_in, double *expr_out, int64_t G, int64_t C,
                            const double *col_sums_dev, double normalize_factor, int32_t do_normalize,
                            int32_t do_log2, void *stream);
/* Host buffers; normalize_factor NaN = median(colSums) like the reference's default
 * (normalize_factor=NA); the factor used is returned through factor_used (nullable). */
int icnv_normalize_log2(const double *expr_in, double *expr_out, int64_t G, int64_t C,
                        double normalize_factor, int32_t do_normalize, int32_t do_log2, double *factor_used);

/* ---- cell-cell distances ------------------------------------ */
/* parallelDist(t(expr.data[, cells])), method "euclidean", as the reference calls it before hclust
 * (R/inferCNV_tumor_subclusters.R:191; R/inferCNV_ops.R:1930, 3242; R/inferCNV_heatmap.R:719-1079):
 * dist_out [n x n] (symmetric, zero diagonal; the R `dist` object is its lower triangle in column order).
 * cell_idx [n] HOST, 0-based.  Bit-equal to R's sequential dist: D_ij = sqrt(d2_ij) (correctly rounded), d2_ij the fp64
 * sum over the genes in order of fl(fl(x_gi - x_gj)^2) on the raw values (no centring, no FMA); D_ii = 0.  Identical
 * cells are at distance exactly 0 and the matrix is exactly symmetric. */
int icnv_cell_distances(const double *expr, int64_t G, int64_t C, const int32_t *cell_idx, int64_t n, double *dist_out);
int icnv_cell_distances_dev(const double *expr, int64_t G, int64_t C, const int32_t *cell_idx, int64_t n, double *dist_out,
                            void *stream);

/* ---- exact k nearest neighbours ---------------------------------------- */
/* RANN::nn2(t(expr_data), k = k_nn)$nn.idx / $nn.dists with query = data, as the reference's Leiden subclustering calls it in
 * .leiden_simple_snn (R/inferCNV_tumor_subclusters.R:726; per chromosome x group at :646-697), for a BATCH of problems.
 * Problem p: genes gene_idx[gene_off[p] .. gene_off[p+1]), cells cell_idx[cell_off[p] .. cell_off[p+1]) (HOST, 0-based, any
 * order; the gene order is the summation order).  For every cell i of problem p (query row cell_off[p] + i) the k cells j of
 * the problem ordered by the key (d2_ij, j) ascending; self included (normally the first neighbour):
 *   d2_ij = the SEQUENTIAL fp64 sum over the problem's genes in list order, s = 0; s = s + t * t with t = x[g,i] - x[g,j],
 *           every operation rounded, no FMA -- bit for bit; nn_dist = sqrt(d2) (IEEE).  (That ANN, RANN's library, sums
 *           this way is believed, not verified against its source.)
 *   Ties: lower cell position first.  RANN orders exactly equal distances by its kd-tree walk, which cannot be restated;
 *   the neighbour SET equals RANN's whenever the k-th and (k+1)-th distances differ.
 * nn_idx [total cells * k] int32: positions within the problem's cell list (0-based; R's are 1-based); nn_dist likewise.
 * 1 <= k <= n_p for every problem (ICNV_ERR_ARG; the caller applies R's skip rules), k <= 128 (ICNV_ERR_UNSUPPORTED).
 * Every offset, gene and cell index is validated before any device work.  Matrix-core screen with a rigorous error bound,
 * exact recomputation of the candidates; a row with too many candidates takes an exhaustive exact pass.
 * Developer switches: ICNV_KNN_EXHAUSTIVE=1 (every row through the exhaustive pass), ICNV_KNN_SCRATCH_MB (screen
 * budget per row block, default 4096), ICNV_KNN_CAP (candidates per row, default 256, at most 1024). */
int icnv_knn(const double *expr, int64_t G, int64_t C, const int32_t *gene_idx, const int32_t *gene_off, const int32_t *cell_idx,
             const int32_t *cell_off, int32_t n_prob, int32_t k, int32_t *nn_idx, double *nn_dist);
/* Same contract on device pointers (expr, nn_idx, nn_dist) + hipStream_t; the index lists stay on the HOST
 * (R/inferCNV_tumor_subclusters.R:726). */
int icnv_knn_dev(const double *expr, int64_t G, int64_t C, const int32_t *gene_idx, const int32_t *gene_off, const int32_t *cell_idx,
                 const int32_t *cell_off, int32_t n_prob, int32_t k, int32_t *nn_idx, double *nn_dist, void *stream);
/* Counters of the kNN calls since the last reset (R/inferCNV_tumor_subclusters.R:726), n = int64 slots of `out` (<= 9 written):
 *   out[0] calls   out[1] problems   out[2] query rows   out[3] row blocks   out[4] rows through the screen
 *   out[5] candidates refined exactly   out[6] screened rows whose candidates overflowed the capacity
 *   out[7] rows through the exhaustive pass   out[8] rows sent there by ICNV_KNN_EXHAUSTIVE
 * Synchronises the devices the calls ran on. */
int icnv_knn_stats(int64_t *out, int32_t n);
void icnv_knn_stats_reset(void);   /* R/inferCNV_tumor_subclusters.R:726 */

/* ---- hierarchical clustering ---------------------------------------------- */
/* fastcluster::hclust(as.dist(D), method) (the reference's hclust, NAMESPACE:57) as the subclustering calls it on
 * parallelDist(t(x)): R/inferCNV_tumor_subclusters.R:191, 411, 474, 498, 582, 609; .random_smoothed_trees.R:76, 228, 269;
 * R/inferCNV_ops.R:1930, 3242; R/inferCNV_heatmap.R:719, 755, 1062, 1079.  Nearest-neighbour chain for every method:
 *   - Lance-Williams update when clusters x < y (sizes s, t) merge at dissimilarity c, for every other cluster k (size v),
 *     a = D[x,k], b = D[y,k], evaluated left to right exactly as written (no FMA):
 *       single  a < b ? a : b            complete  a > b ? a : b          average  (s*a + t*b) / (s+t)
 *       mcquitty (a + b) * 0.5           ward.D / ward.D2  ((v+s)*a - v*c + (v+t)*b) / (s+t+v)
 *     ward.D2 squares D on entry (d*d) and reports sqrt of each merge dissimilarity.
 *   - The chain restarts from the first active index when it is empty (after a merge leaves <= 1 element); extending it,
 *     the tip's nearest active neighbour is the minimum of the key (D[tip,j], rank j), rank(previous chain element) = -1.
 *     The merged cluster lives on at the larger index y; x is retired.
 *   - Merges are stable-sorted by dissimilarity and labelled as R does: singletons -(i+1), clusters the 1-based step that
 *     made them, per row the singleton first, two singletons by index, two clusters by creation.  order = the left-first
 *     depth-first walk from the last merge, 1-based.
 * Outputs: merge int32 [(n-1) x 2] column-major (R's layout), height double [n-1], order int32 [n].
 * Errors: n < 2 or a non-finite distance ICNV_ERR_ARG (as R / fastcluster stop), an unsupported method
 * ICNV_ERR_UNSUPPORTED, allocation failure ICNV_ERR_NOMEM.  Every argument is validated before any launch; the finiteness
 * of the distances is checked on the device before the clustering starts.  Unlike the other *_dev entry points these
 * synchronise `stream`: the finiteness check and the R labelling of the merge list go through the host.
 * Developer switch: ICNV_HCLUST_FORCE_HBM=1 sends problems of <= 200 cells down the large-problem (HBM) path. */
#define ICNV_HCLUST_WARD_D 1
#define ICNV_HCLUST_WARD_D2 2
#define ICNV_HCLUST_SINGLE 3
#define ICNV_HCLUST_COMPLETE 4
#define ICNV_HCLUST_AVERAGE 5
#define ICNV_HCLUST_MCQUITTY 6
#define ICNV_HCLUST_CENTROID 7   /* not reducible: ICNV_ERR_UNSUPPORTED */
#define ICNV_HCLUST_MEDIAN 8     /* not reducible: ICNV_ERR_UNSUPPORTED */
/* hclust(as.dist(D), method) of an n x n DEVICE distance matrix (row i at dist + i*ld, symmetric, zero diagonal; it is not
 * modified).  merge / height / order: DEVICE pointers.  (R/inferCNV_tumor_subclusters.R:191, R/inferCNV_ops.R:3242) */
int icnv_hclust_dev(const double *dist, int64_t ld, int32_t n, int32_t method, int32_t *merge, double *height, int32_t *order,
                    void *stream);
/* hclust(parallelDist(t(expr[genes_p, cells_p])), method) for a BATCH of problems described as for icnv_knn (HOST index
 * lists, 0-based; the z-score-filtered gene lists of R/inferCNV_tumor_subclusters.R:45-71): the Euclidean distances
 * bit-equal to R's sequential dist over the problem's genes in list order (as icnv_cell_distances), then the clustering; the
 * matrices never leave the device.  So merge, height and order are those of icnv_hclust_dev on that sequential dist.
 * Problem p has n_p = cell_off[p+1] - cell_off[p] >= 2 cells; its outputs start at merge + 2*(cell_off[p] - p),
 * height + (cell_off[p] - p) and order + cell_off[p].  (R/inferCNV_tumor_subclusters.R:191, 582, 609) */
int icnv_hclust_cells(const double *expr, int64_t G, int64_t C, const int32_t *gene_idx, const int32_t *gene_off,
                      const int32_t *cell_idx, const int32_t *cell_off, int32_t n_prob, int32_t method, int32_t *merge,
                      double *height, int32_t *order);
/* Same contract on device pointers (expr, merge, height, order); the index lists stay on the HOST. */
int icnv_hclust_cells_dev(const double *expr, int64_t G, int64_t C, const int32_t *gene_idx, const int32_t *gene_off,
                          const int32_t *cell_idx, const int32_t *cell_off, int32_t n_prob, int32_t method, int32_t *merge,
                          double *height, int32_t *order, void *stream);
/* Counters of the hclust calls since the last reset (R/inferCNV_tumor_subclusters.R:191), n = int64 slots (<= 6 written):
 *   out[0] calls   out[1] problems   out[2] problems clustered in LDS   out[3] problems clustered in HBM
 *   out[4] chain steps (nearest-neighbour searches)   out[5] wall time of the calls in microseconds */
int icnv_hclust_stats(int64_t *out, int32_t n);
void icnv_hclust_stats_reset(void);   /* R/inferCNV_tumor_subclusters.R:191 */

/* ---- random-trees subclustering ------------------------------------------- */
/* The permutation statistic of tumor_subcluster_partition_method = "random_trees"
 * (R/inferCNV_tumor_subclusters.random_smoothed_trees.R:217-298, .parameterize_random_cluster_heights_smoothed_trees) for
 * every clade of one recursion level (:127-213) in ONE call.  Clade p (HOST cell list, 0-based, n_p >= 2 cells, all G genes):
 *   - the observed matrix x[, S_p] and n_iter copies; copy r (0-based) permutes every gene g across the clade's cells with
 *     NumPy's Generator(Philox(key = [seed, token[p]], counter = [0, g, r, 0])).permutation(n_p)  (:233-246; R's own stream
 *     depends on its worker threads and is never seeded, so the library defines this one);
 *   - caTools::runmean(k = window, endrule = "mean") along the genes of every cell (:221, 259): k = min(window, G), k2 = k / 2,
 *     output o = the sequential sum (gene order, no FMA) of the window [max(0, o - (k - 1 - k2)), min(G - 1, o + k2)] divided by
 *     its length; k <= 1 leaves the cell unchanged;
 *   - .center_columns(, "median") per cell (:223, 261): step 11's median (ICNV_ST_CENTER);
 *   - hclust(parallelDist(t(.)), method) (:226-229, 264-269): K9's fused distances, bit-equal to R's sequential dist of the
 *     matrix above over all G genes in order, and chain (icnv_hclust_cells_dev).
 * Outputs (DEVICE): the observed trees in icnv_hclust_cells' layout and offsets (merge + 2 (cell_off[p] - p), height +
 * (cell_off[p] - p), order + cell_off[p]); rand_max_height [n_prob x n_iter] = max(h_rand$height) of copy r of clade p at
 * p * n_iter + r (:270).  Permuted trees never leave the device.  Matrices and distance matrices are built in waves within
 * ICNV_RT_SCRATCH_MB megabytes (default 8192; at least one matrix per wave); results do not depend on the waves.
 * Errors: ICNV_ERR_ARG for n_p < 2, window < 1, n_iter < 1, an index out of range or a non-finite value among the clades'
 * cells (checked on the device before anything is clustered); ICNV_ERR_UNSUPPORTED for centroid / median.  Every argument is
 * validated before any launch.  Synchronises `stream`. */
#define ICNV_RT_PERMUTE 0x1u
#define ICNV_RT_SMOOTH  0x2u
#define ICNV_RT_CENTER  0x4u
/* expr: G x C column-major DEVICE matrix; cell_idx / cell_off / token: HOST arrays.
 * (R/inferCNV_tumor_subclusters.random_smoothed_trees.R:217-298) */
int icnv_random_trees_dev(const double *expr, int64_t G, int64_t C, const int32_t *cell_idx, const int32_t *cell_off,
                          const uint64_t *token, int32_t n_prob, int32_t window, int32_t n_iter, uint64_t seed, int32_t method,
                          int32_t *merge, double *height, int32_t *order, double *rand_max_height, void *stream);
/* Same contract on HOST buffers.  (R/inferCNV_tumor_subclusters.random_smoothed_trees.R:217-298) */
int icnv_random_trees(const double *expr, int64_t G, int64_t C, const int32_t *cell_idx, const int32_t *cell_off,
                      const uint64_t *token, int32_t n_prob, int32_t window, int32_t n_iter, uint64_t seed, int32_t method,
                      int32_t *merge, double *height, int32_t *order, double *rand_max_height);
/* Diagnostic: one (clade, iteration) matrix after the stages in `stages` (ICNV_RT_*), written to the DEVICE buffer out
 * (n x G, a cell's genes contiguous).  iter = -1 is the observed matrix; ICNV_RT_PERMUTE has no effect on it.  cells: HOST.
 * (R/inferCNV_tumor_subclusters.random_smoothed_trees.R:221-223, 255-261) */
int icnv_random_trees_matrix_dev(const double *expr, int64_t G, int64_t C, const int32_t *cells, int32_t n, int32_t window,
                                 uint64_t seed, uint64_t token, int32_t iter, uint32_t stages, double *out, void *stream);
/* Counters since the last reset (R/inferCNV_tumor_subclusters.random_smoothed_trees.R:255), n = int64 slots (<= 6 written):
 *   out[0] calls   out[1] clades   out[2] permuted matrices   out[3] waves   out[4] chain steps   out[5] wall microseconds */
int icnv_random_trees_stats(int64_t *out, int32_t n);
void icnv_random_trees_stats_reset(void);   /* R/inferCNV_tumor_subclusters.random_smoothed_trees.R:255 */

/* ---- Leiden community detection (K11) -------------------------------------------------------------------------------
 * cluster_leiden(graph_from_adjacency_matrix(sparseMatrix(nn2(t(x), k)$nn.idx), mode = "undirected"), resolution, objective)
 * of .leiden_simple_snn (R/inferCNV_tumor_subclusters.R:726-741) for a BATCH of problems, on the kNN blocks of icnv_knn_dev.
 * R's cluster_leiden draws from R's RNG inside igraph's C code: the partition is not claimed equal to igraph's.  The library
 * defines the algorithm and its random stream exactly (restated in tests/leiden_restate.py);
 * "as igraph does" below is believed, not verified.
 *
 * Graph of problem p (rows node_off[p] .. node_off[p+1] of nn_idx, k positions each, 0-based within the problem):
 *   edge {i, j}, i != j, weight 1 iff j is in row i or i in row j (igraph's mode = "undirected" acts as "max" on a 0/1
 *   matrix, :733); loop at i iff i is in row i; strength s_i = #neighbours + 2 loop_i; neighbour lists ascending.
 * Weights (int64, exact): node weight 1 (CPM) or s_i (modularity); edge weights are edge counts, summed by aggregation.
 * Resolution: r = gamma (CPM) or gamma / sum(s) (modularity, R's wrapper: resolution_parameter / sum(strength)), a double
 *   division on the host.  Gain of moving v into C: diff = e_vC - ((w_v * W_C) * r) in doubles in that order, no FMA.
 * One iteration (Traag et al. 2019 as igraph's leiden.c structures it), from singletons or the previous result; per level l:
 *   1. move: queue = permutation stream (it, l, 1, 0) of the n_l nodes, all unstable; unused cluster ids on a stack
 *      (pushed in increasing order).  Pop v, take it out of its cluster c0 (push c0 if it empties); candidates: the top of
 *      the stack, then the clusters of v's neighbours by first appearance; best starts at c0 (its diff after v left),
 *      replaced on a strictly greater diff.  v goes to best, stable; if best != c0, each neighbour (list order) that is
 *      stable and not in best is appended and unstable.  At the end clusters are renumbered by first appearance: K_l.
 *   2. K_l = n_l ends the iteration.
 *   3. refine each move cluster c (nodes S_c ascending, visited in the order of permutation stream (it, l, 2, c)); every
 *      node a singleton; T_c = sum of w over S_c; ext(X) = weight of X's edges to the rest of S_c.  Visit v only if its
 *      cluster is still a singleton and ext(v) >= ((w_v * (T_c - w_v)) * r); empty it; candidates: that empty cluster,
 *      then the refined clusters of v's neighbours in S_c by first appearance.  D is admissible iff
 *      ext(D) >= ((W_D * (T_c - W_D)) * r); every admissible D with diff >= 0 adds exp_lib(diff / beta) to a sequential
 *      running sum (exp_lib: leiden_internal.h, +inf above 709).  Sum finite: t = u * sum with u the next
 *      Generator.random() of stream (it, l, 3, c), the first candidate whose running sum is > t (none: the last one that
 *      added); sum +inf: the strict maximum of the admissible diffs (starting at 0 on the empty cluster).
 *   4. refined clusters numbered by (c, first appearance in ascending node order); if there are n_l of them, aggregate on
 *      the move clusters instead (igraph: "refinement didn't aggregate").
 *   5. aggregate: one node per refined cluster, w summed, edge weights summed, no loops, rows ascending; each aggregate
 *      starts the next level in its move cluster.
 *   At the end of the iteration every node takes its aggregate's cluster, renumbered by first appearance.
 * Streams: NumPy's Generator(Philox(key = [seed, token_p], counter = [0, phase, (it << 32) | l, c])), .permutation(n) and
 *   .random() (K10's RtPhilox).
 * Limits: 1 <= k <= min(128, n_p) (k > 128: ICNV_ERR_UNSUPPORTED), monotone node_off, a known objective, resolution finite
 *   and >= 0, beta finite and > 0, 1 <= n_iterations <= 1000: ICNV_ERR_ARG before any launch.  An nn_idx entry outside
 *   [0, n_p) is ICNV_ERR_ARG from a device check before anything is clustered.  Outputs stay untouched on any error.  Caps:
 *   256 n_l + 1024 queue pops per move phase and 512 levels per iteration; more is ICNV_ERR_UNSUPPORTED (never a spin).
 * Output: membership (1-based, DEVICE, one per node) and n_clusters (HOST, one per problem).  token: HOST, one per problem
 * (NULL: all 0).  Synchronises the stream. */
#define ICNV_LEIDEN_CPM 1
#define ICNV_LEIDEN_MODULARITY 2
int icnv_leiden_dev(const int32_t *nn_idx, int32_t k, const int32_t *node_off, int32_t n_prob, int32_t objective,
                    const double *resolution, double beta, int32_t n_iterations, uint64_t seed, const uint64_t *token,
                    int32_t *membership, int32_t *n_clusters, void *stream);
/* The same with HOST nn_idx and membership. */
int icnv_leiden(const int32_t *nn_idx, int32_t k, const int32_t *node_off, int32_t n_prob, int32_t objective,
                const double *resolution, double beta, int32_t n_iterations, uint64_t seed, const uint64_t *token,
                int32_t *membership, int32_t *n_clusters);
/* Diagnostic: the graph above as one CSR over the batch (DEVICE): row_off [sum n_p + 1] (problem p's rows follow each other),
 * col [at least 2 k sum n_p] positions within the problem, strength [sum n_p].  Synchronises the stream. */
int icnv_snn_graph_dev(const int32_t *nn_idx, int32_t k, const int32_t *node_off, int32_t n_prob, int64_t *row_off,
                       int32_t *col, int64_t *strength, void *stream);
/* Counters since the last reset: out[0] calls, [1] problems, [2] levels, [3] move visits (queue pops), [4] refinement
 * visits, [5] draws, [6] wall microseconds of the calls. */
int icnv_leiden_stats(int64_t *out, int32_t n);
void icnv_leiden_stats_reset(void);   /* R/inferCNV_tumor_subclusters.R:736 */

/* ---- PCA route of the Leiden subclustering (K18) -----------------------------------------------------------------------
 * .leiden_seurat_preprocess_routine (R/inferCNV_tumor_subclusters.R:699-723), the reference's default leiden_method = "PCA"
 * (R/inferCNV_ops.R:289, R/inferCNV_tumor_subclusters.R:5): CreateSeuratObject -> FindVariableFeatures -> ScaleData ->
 * RunPCA(npcs = 10) -> FindNeighbors(k.param = k_nn) -> graph_from_adjacency_matrix(snn, mode = "min", weighted = TRUE) ->
 * cluster_leiden, for a BATCH of problems.  Seurat's loess (kd-tree interpolation), irlba (randomised, truncated), annoy
 * (approximate) and igraph's RNG cannot be restated: the library defines each stage exactly (DESIGN.md section 4 K18,
 * restated in tests/leiden_pca_restate.py); "as Seurat does" below is believed, not verified.
 * A problem is n cells (cell list, HOST) and its genes (gene list, HOST, in list order); element (gene g, cell c) at
 * expr[c * ld + g].  mean / sd / v_std are DEVICE arrays with one entry per (problem, gene), packed like gene_idx.
 *
 * icnv_lpca_vstd_dev (FindVariableFeatures, selection.method = "vst", clip.max = "auto"; :706): mean = K15's mean of the gene
 *   over the problem's cells (icnv_group_gene_tables_dev), sd = sqrt(10^fit) of the host's trend (infercnv_amd/loess_fit.py):
 *   v_std = (sum over the cells in list order of min(sqrt(n), (x - mean) / sd)^2) / (n - 1), a sequential fp64 sum, every
 *   operation rounded by itself (no FMA).  sd = 0 (a gene outside the fit: constant over the cells) gives 0.  n >= 2.
 * icnv_lpca_scale_dev (ScaleData, :707-708): z = min(10, (x - mean) / sd) with sd = sqrt(K15's variance); sd = 0 gives 0.
 *   Written feature-major: problem p's block starts at the sum over q < p of F_q ldz_q doubles, F_p rows (the listed genes in
 *   order) of ldz_p = n_p + (n_p & 1) doubles, the padding element 0.
 * icnv_lpca_gram_dev (RunPCA, :709): M_p = Z_p Z_p^T (F_p x F_p, row-major, packed one after another) on the fp64 matrix
 *   cores: the upper triangle of 64 x 64 tiles, each value written to (a, b) and (b, a): exactly symmetric.  Per entry
 *   |M - sum z_a z_b| <= gamma_n sum |z_a z_b|, gamma_n = n u / (1 - n u), u = 2^-53, whatever the summation order.
 * icnv_lpca_project_dev: E_p = Z_p^T V_p, V_p (F_p x npcs_p, row-major, packed) the eigenvectors: per (cell, component) the
 *   sequential fp64 sum over the features in ascending order of the rounded products (no FMA).  E: (sum n_p, e_ld) rows in
 *   problem order, the components >= npcs_p zero: the matrix icnv_knn_dev searches (npcs "genes").  npcs_p <= e_ld <= 64.
 * icnv_snn_begin_dev / _fill_dev / _end (Seurat's ComputeSNN, prune.SNN = 1/15, on the (n, k) index block of icnv_knn_dev):
 *   s_ij = |N(i) n N(j)| for every pair i != j that shares a neighbour; kept iff 16 s_ij >= 2 k (s / (2 k - s) >= 1/15 in
 *   integers).  begin builds the transposed lists (count, scan, fill, sort per row), counts every row and returns the exact
 *   number of entries (HOST); fill writes the CSR (DEVICE): row_off [sum n_p + 1] over the batch, col ascending positions
 *   within the problem, shared = s_ij, weight = (2 s 2^24 + d) / (2 d) with d = 2 k - s in integer division (s / d in 24-bit
 *   fixed point, rounded to nearest), loop [sum n_p] = 1 (s_ii = k: every node carries a loop of weight 2^24).  An nn_idx
 *   entry outside [0, n_p): ICNV_ERR_ARG from a device check.  N(i) is a set: an nn_idx row that repeats an entry is
 *   ICNV_ERR_ARG too, from a device check on the sorted transposed lists before any row is counted (no handle, the outputs
 *   untouched); icnv_knn_dev never makes such a row.  So s_ij <= k and d >= k.  1 <= k <= min(128, n_p).  end frees the state.
 * icnv_leiden_graph_dev: icnv_leiden_dev (K11, its contract above word for word) on a caller's weighted graphs instead of
 *   nn_idx: level 0 has the edge weights `weight` (int64 >= 1), s_i = sum of row i's weights + 2 loop_weight loop_i; node
 *   weight 1 (CPM) or s_i (modularity); r = gamma (CPM: the caller scales gamma by its weight unit) or gamma / sum s.  The CSR
 *   must be symmetric (not checked); rows ascending, without the node itself, col in [0, n_p), loop in {0, 1}: ICNV_ERR_ARG
 *   from a device check.  Total edge weight of a problem (sum s / 2) >= 2^53: ICNV_ERR_UNSUPPORTED (the int64 -> double
 *   conversions of the gain must be exact).  Scratch is sized by the entries of the CSR.  Every call synchronises. */
typedef struct icnv_snn icnv_snn_t;
int icnv_lpca_vstd_dev(const double *expr, int64_t G, int64_t C, int64_t ld, const int32_t *gene_idx, const int32_t *gene_off,
                       const int32_t *cell_idx, const int32_t *cell_off, int32_t n_prob, const double *mean, const double *sd,
                       double *v_std, void *stream);
int icnv_lpca_scale_dev(const double *expr, int64_t G, int64_t C, int64_t ld, const int32_t *gene_idx, const int32_t *gene_off,
                        const int32_t *cell_idx, const int32_t *cell_off, int32_t n_prob, const double *mean, const double *sd,
                        double *Z, void *stream);
int icnv_lpca_gram_dev(const double *Z, const int32_t *n_feat, const int32_t *n_cells, int32_t n_prob, double *M, void *stream);
int icnv_lpca_project_dev(const double *Z, const double *V, const int32_t *n_feat, const int32_t *n_cells, const int32_t *npcs,
                          int32_t n_prob, double *E, int32_t e_ld, void *stream);
int icnv_snn_begin_dev(const int32_t *nn_idx, int32_t k, const int32_t *node_off, int32_t n_prob, icnv_snn_t **out, int64_t *nnz,
                       void *stream);
int icnv_snn_fill_dev(icnv_snn_t *h, int64_t *row_off, int32_t *col, int32_t *shared, int64_t *weight, int32_t *loop, void *stream);
void icnv_snn_end(icnv_snn_t *h);   /* R/inferCNV_tumor_subclusters.R:710 */
int icnv_leiden_graph_dev(const int64_t *row_off, const int32_t *col, const int64_t *weight, const int32_t *loop, int64_t loop_weight,
                          const int32_t *node_off, int32_t n_prob, int32_t objective, const double *resolution, double beta,
                          int32_t n_iterations, uint64_t seed, const uint64_t *token, int32_t *membership, int32_t *n_clusters,
                          void *stream);

/* ---- HMM ---------------------------------------------------------------- */
/* Viterbi.dthmm.adj (R/inferCNV_HMM.R:1101-1176) for every (cell, chromosome):
 * predict_CNV_via_HMM_on_indiv_cells (R/inferCNV_HMM.R:284-324) with K = 6 and
 * i3HMM_predict_CNV_via_HMM_on_indiv_cells (R/inferCNV_i3HMM.R:180-225) with
 * K = 3.  Host-prepared parameters, exactly as the reference prepares them in
 * R: mean[K]; sd_shared = median(pm$sd) (:1122); logPi = log(Pi) K x K
 * column-major (logPi[j + K*k] = log Pi[j,k]); logDelta = log(delta).
 * states[g + G*c] in 1..K (uint8); chromosomes with < 2 genes get 3 (:1104).
 * n_underflow (nullable, HOST) receives the number of sequences for which the
 * reference would stop("Problems With Underflow"); the host flavour returns
 * ICNV_ERR_UNDERFLOW when it is non-zero. */
int icnv_viterbi_cells(const double *expr, uint8_t *states, int64_t G, int64_t C,
                       const int32_t *chr_start, int32_t n_chr, int32_t K, const double *mean,
                       double sd_shared, const double *logPi, const double *logDelta);
int icnv_viterbi_cells_dev(const double *expr, uint8_t *states, int64_t G, int64_t C,
                           const int32_t *chr_start, int32_t n_chr, int32_t K, const double *mean,
                           double sd_shared, const double *logPi, const double *logDelta,
                           int32_t *n_underflow_dev, void *stream);
/* The same on matrices with LEADING DIMENSIONS: expr[g + ld_expr * c], states[g + ld_states * c] (both >= G).  The per-cell
 * kernels read one cache line per cell and request and write the states in 16-byte words: with columns that start on line /
 * word boundaries (ld a multiple of 16) a gene count that is not a multiple of 16 runs as fast as one that is (+27 % otherwise,
 * profiles/r05_sweep.json).  icnv_viterbi_cells (host buffers -- what R hands over) uploads into such a layout by itself. */
int icnv_viterbi_cells_ld_dev(const double *expr, int64_t ld_expr, uint8_t *states, int64_t ld_states, int64_t G, int64_t C,
                              const int32_t *chr_start, int32_t n_chr, int32_t K, const double *mean,
                              double sd_shared, const double *logPi, const double *logDelta,
                              int32_t *n_underflow_dev, void *stream);

/* Certified fast path of the per-cell Viterbi (DESIGN.md "Certified fast Viterbi").  With a shared sd and the
 * transition structure of .get_HMM / .i3HMM_get_HMM (R/inferCNV_HMM.R:230-265, R/inferCNV_i3HMM.R:99-156: one
 * off-diagonal and one diagonal probability) icnv_viterbi_cells[_dev] computes the emission scores from a
 * verified polynomial table, tests every arg-max decision against a certified error band and recomputes the
 * flagged sequences with the exact kernel: the states are those of the exact kernel, bit for bit.
 * A column batch with more than 2 % of its sequences flagged is recomputed as a whole by the exact kernel instead
 * (decided on the device from that batch's own flag count: no state carries over from one call to the next).
 * Two kernels serve the fast path: the staged one (observations requested by whole cache lines through LDS-DMA, a short
 * table: tails of >= 4 sd beyond the outer state means) is tried first; a column batch whose data leave its table is redone
 * by the register kernel with the full table (tails up to 19 sd), and only a batch that still has > 2 % flagged goes to the
 * exact kernel -- all decided on the device.
 *   icnv_viterbi_set_mode   0 = auto (default), 1 = exact kernel only, 2 = auto without the staged kernel (developer A/B);
 *                           process-wide
 *   icnv_viterbi_last_stats out4 = {path of the calling thread's device's last call (0 exact / 1 fast, register kernel /
 *                           2 fast, last column batch recomputed by the exact kernel / 3 fast, staged kernel / 4 staged
 *                           kernel, last column batch redone with the full table), sequences, flagged sequences of
 *                           the last column batch, table intervals}; synchronises with that call
 *   icnv_hmm_emission_table host-only: the table for (K, mean, sd); meta8 = {n_records, x_lo, x_hi, eps_tab,
 *                           s_max, degree, 1, eps_spec}; seg_out [4] = the uniform grid {origin, 1/width, 0, grid
 *                           intervals - 1} (n_records = grid intervals + K: an interval with a state mean has two);
 *                           coef_out [n_records*K*(degree+1)] (nullable; polynomials of s_k - s_1, row k = 0 zero);
 *                           eps_tab bounds |table - (s_k - s_1)|, s_max bounds |s_k| and |s_k - s_1|
 *   icnv_hmm_emission_scores host-only: which = 0 the exact scores of R/inferCNV_HMM.R:1129-1133 in 80-bit
 *                           arithmetic, which = 1 the table's values through the kernel's double operations: the
 *                           scores RELATIVE TO STATE 1, s_k - s_1 (column 0 is 0; a term common to all states
 *                           changes no decision of the recurrence, so the table does not carry it)
 *                           (ok_out[i] = 0 and NaN where x[i] is outside the table's domain); out [n*K] */
int icnv_viterbi_set_mode(int mode);
int icnv_viterbi_last_stats(int64_t *out4);
int icnv_hmm_emission_table(int32_t K, const double *mean, double sd, double *meta8, double *seg_out, double *coef_out,
                            int64_t coef_cap);
int icnv_hmm_emission_scores(int32_t K, const double *mean, double sd, const double *x, int64_t n, int32_t which,
                             double *out, uint8_t *ok_out);

/* predict_CNV_via_HMM_on_tumor_subclusters / _whole_tumor_samples
 * (R/inferCNV_HMM.R:345-408, 509-567) and the i3 variants
 * (R/inferCNV_i3HMM.R:249-389): Viterbi on rowMeans over each group's cells
 * with that group's shared sd, trace broadcast to all member cells.  Cells in
 * no group get 0xFF (the reference leaves -1).  For the per-chromosome
 * grouping of ..._tumor_subclusters_per_chr (:412-487) call once per
 * chromosome with n_chr = 1 windows. */
int icnv_viterbi_groups(const double *expr, uint8_t *states, int64_t G, int64_t C,
                        const int32_t *chr_start, int32_t n_chr, const int32_t *grp_idx,
                        const int32_t *grp_off, int32_t n_grp, int32_t K, const double *mean,
                        const double *sd_shared_per_grp, const double *logPi,
                        const double *logDelta);
int icnv_viterbi_groups_dev(const double *expr, uint8_t *states, int64_t G, int64_t C,
                            const int32_t *chr_start, int32_t n_chr, const int32_t *grp_idx,
                            const int32_t *grp_off, int32_t n_grp, int32_t K, const double *mean,
                            const double *sd_shared_per_grp, const double *logPi,
                            const double *logDelta, int32_t *n_underflow_dev, void *stream);

/* rowMeans(expr.data[, group_cells]) per group (R/inferCNV_HMM.R:383):
 * out[g + G*q], device pointers. */
int icnv_group_means_dev(const double *expr, int64_t G, int64_t C, const int32_t *grp_idx,
                         const int32_t *grp_off, int32_t n_grp, double *out, void *stream);

/* Gene filters of the ingest (first "next" row).  icnv_gene_stats: per gene the sum over all cells
 * and the number of cells with expr > 0 -- what require_above_min_mean_expr_cutoff (rowMeans(expr) < cutoff,
 * R/inferCNV_ops.R:2128-2163) and require_above_min_cells_ref (sum(x > 0 & !is.na(x)) >= min_cells, :2182-2213)
 * decide on; a cell-sharded caller all-reduces both vectors.  icnv_select_genes: remove_genes on the matrix,
 * expr_out[j + G_out*c] = expr_in[keep_idx[j] + G_in*c] (0-based, any order). */
int icnv_gene_stats(const double *expr, int64_t G, int64_t C, double *gene_sums, int32_t *gene_nnz);
int icnv_gene_stats_dev(const double *expr, int64_t G, int64_t C, double *gene_sums, int32_t *gene_nnz, void *stream);
int icnv_select_genes(const double *expr_in, int64_t G_in, int64_t C, const int32_t *keep_idx, int64_t G_out,
                      double *expr_out);
int icnv_select_genes_dev(const double *expr_in, int64_t G_in, int64_t C, const int32_t *keep_idx, int64_t G_out,
                          double *expr_out, void *stream);

/* mean() and sd() over the block expr[gene_idx, cell_idx] (gene_idx NULL = all genes): the per-CNV-level emission
 * statistics of get_spike_dists (R/inferCNV_HMM.R:15-99; SURVEY.md 8f, third "next" row).  out2 = {mean, sd} on the
 * host; index lists are host arrays, 0-based. */
int icnv_block_mean_sd(const double *expr, int64_t G, int64_t C, const int32_t *gene_idx, int64_t n_genes,
                       const int32_t *cell_idx, int64_t n_cells, double *out2);
int icnv_block_mean_sd_dev(const double *expr, int64_t G, int64_t C, const int32_t *gene_idx, int64_t n_genes,
                           const int32_t *cell_idx, int64_t n_cells, double *out2_host, void *stream);

/* .get_state_consensus (R/inferCNV_HMM.R:977-987): per gene the most frequent state among each group's
 * cells (ties -> smallest state, -1/0xFF first, as table()+order() do).  consensus (nullable): uint8
 * [g + G*q].  states_out (nullable, may alias states): every member cell receives its group's consensus
 * -- the overwrite that predict_CNV_via_HMM_on_tumor_subclusters_per_chr (R/inferCNV_HMM.R:473-483) and
 * get_predicted_CNV_regions (:706-764) are built on (second "next" row). */
int icnv_state_consensus(const uint8_t *states, int64_t G, int64_t C, const int32_t *grp_idx,
                         const int32_t *grp_off, int32_t n_grp, uint8_t *consensus, uint8_t *states_out);
int icnv_state_consensus_dev(const uint8_t *states, int64_t G, int64_t C, const int32_t *grp_idx,
                             const int32_t *grp_off, int32_t n_grp, uint8_t *consensus,
                             uint8_t *states_out, void *stream);

/* assign_HMM_states_to_proxy_expr_vals (R/inferCNV_HMM.R:1191-1206; K = 6:
 * {0,0.5,1,1.5,2,3}) and i3HMM_assign_... (R/inferCNV_i3HMM.R:405-417; K = 3:
 * {0.5,1,1.5}).  n = G*C elements. */
int icnv_states_to_proxy(const uint8_t *states, double *out, int64_t n, int32_t K);
int icnv_states_to_proxy_dev(const uint8_t *states, double *out, int64_t n, int32_t K, void *stream);

/* Mean and sd over ALL values of the listed cells (i3 parameters,
 * R/inferCNV_i3HMM.R:17-80; also clear_noise's centre).  out2_host = {mu, sigma}. */
int icnv_cells_mean_sd_dev(const double *expr, int64_t G, int64_t C, const int32_t *cell_idx,
                           int64_t n_cells, double *out2_host, void *stream);
int icnv_cells_mean_sd(const double *expr, int64_t G, int64_t C, const int32_t *cell_idx, int64_t n_cells, double *out2);
/* The same statistic split in two for a cell-sharded caller ("i3: [sum x, sum x^2, n] over reference
 * values"; in the two-pass form R's sd() uses):
 *   phase 0: out3_host = {sum of the values, number of values, 0}                 -> all-reduce(sum) -> mean = sum / n
 *   phase 1: out3_host = {sum of (x - mean)^2 over the values, number, 0}         -> all-reduce(sum) -> sd = sqrt(ss / (n - 1))
 * A rank that holds none of the cells passes n_cells = 0 (expr may then be NULL) and contributes zeros.
 * Replaces the mean(ref values) / sd(ref values) of .i3HMM_get_sd_trend_by_num_cells_fit, R/inferCNV_i3HMM.R:38-52. */
int icnv_cells_moments_partial_dev(const double *expr, int64_t G, int64_t C, const int32_t *cell_idx, int64_t n_cells,
                                   int32_t phase, double mean, double *out3_host, void *stream);

/* The i3 HMM at group level as a PLAN with device-resident parameters (round 6).  i3HMM_predict_CNV_via_HMM_on_tumor_subclusters /
 * _whole_tumor_samples (R/inferCNV_i3HMM.R:249-389) compute mean(ref) and sd(ref) of the reference cells' values
 * (.i3HMM_get_sd_trend_by_num_cells_fit, :38-52), place the three state means at mu and mu +- delta (:435-445) and run the
 * Viterbi on every group's mean profile.  The plan uploads the group structure ONCE; a step is
 *   icnv_group_hmm_i3_partial_dev(): group means + the reference cells' shifted moments {sum (x - 1), sum (x - 1)^2, n} in ONE pass
 *       over the matrix; *moments_dev points at the three doubles on the device -- all-reduce(sum) them in a cell-sharded run;
 *   icnv_group_hmm_i3_finish_dev(): mu, sigma, delta from the moments ON THE DEVICE (delta = delta_abs when it is a number -- the
 *       KS-based value of use_KS = TRUE, computed by the caller from sigma --, sigma * z_abs otherwise: |qnorm(p, 0, sigma)| =
 *       sigma |qnorm(p)|), Viterbi per group with its parameters read from device memory, broadcast to the cells.
 * No upload, download or stream synchronisation inside a step.  Every cell in at most one group, every reference cell in exactly
 * one, at most 8192 (group, chromosome) sequences (ICNV_ERR_UNSUPPORTED otherwise: icnv_viterbi_groups_dev serves those).  The
 * moments are shifted around 1, the level the chain's output is centred at: mu and sigma agree with the two-pass long-double values
 * of icnv_cells_moments_partial_dev to ~1e-15 relative. */
typedef struct icnv_group_hmm icnv_group_hmm_t;
int icnv_group_hmm_begin(icnv_group_hmm_t **plan, int64_t G, int64_t C, const int32_t *chr_start, int32_t n_chr,
                         const int32_t *grp_idx, const int32_t *grp_off, int32_t n_grp, const int32_t *ref_idx, int64_t n_ref);
int icnv_group_hmm_i3_partial_dev(icnv_group_hmm_t *plan, const double *expr, double **moments_dev, void *stream);
int icnv_group_hmm_i3_finish_dev(icnv_group_hmm_t *plan, uint8_t *states, const double *logPi /* 3 x 3, column-major */,
                                 const double *logDelta /* [3] */, double z_abs, double delta_abs,
                                 int32_t *n_underflow_dev, void *stream);
/* {mu, sigma, delta} of the last finish (synchronises the stream). */
int icnv_group_hmm_get_i3_params(icnv_group_hmm_t *plan, double *mu_sigma_delta, void *stream);
void icnv_group_hmm_end(icnv_group_hmm_t *plan);

/* Values of the matrix at element offsets g + G c (host list in, host values out): the draws of
 * sample(expr_vals, size = ncells, replace = TRUE) in get_hspike_cnv_mean_sd_trend_by_num_cells_fit
 * (R/inferCNV_HMM.R:164) taken from the resident hidden-spike matrix; the index stream itself is R's RNG, restated on the
 * host (infercnv_amd/r_rng.py). */
int icnv_gather_values_dev(const double *expr, int64_t n_elements, const int64_t *offsets_host, int64_t n, double *out_host, void *stream);
int icnv_gather_values(const double *expr, int64_t G, int64_t C, const int64_t *offsets, int64_t n, double *out);

/* ---- non-DE gene masking (K12) --------------------------------------------------------------------------------------
 * get_DE_genes_basic / .mask_DE_genes (R/inferCNV_mask_non_DE.R:28-258, step 21 of run()): per gene and per comparison
 * (x group, y group) = (normal type, tumour subcluster), wilcox.test(x, y) or t.test(x, y), then p.adjust(, "BH") over the
 * genes of each comparison.  DESIGN.md section 4 K12, restated in tests/de_restate.py; R's arithmetic is read, not run.
 * Groups: cell_idx / cell_off (HOST, int32, 0-based columns of the matrix, cell_off[0] = 0); cmp: HOST, n_cmp pairs of
 * group numbers (x first).  Element (gene g, cell c) at expr[c * ld + g].  Outputs [n_cmp x G] (row k = comparison k):
 * stat (W, or t), p and padj.
 * ICNV_DE_WILCOXON: per (gene, cell) jitter j = 1e-4 + 1e-4 z (jitter != 0), z from NumPy's
 *   Generator(Philox(key = [seed, ICNV_DE_JITTER_TOKEN], counter = [0, g, c, 0])): u1, u2 = two .random() draws,
 *   z = qnorm((floor(2^27 u1) + u2) / 2^27) (R's INVERSION; AS 241 with the library's table log).  The same cell has the same
 *   jitter in every comparison of a call.  Values x + j; non-finite values dropped; an empty sample is ICNV_ERR_ARG naming the
 *   comparison and the gene.  Midranks of the pooled sample (-0 == +0); 2W = 2 sum(ranks of x) - n.x (n.x + 1), exact;
 *   T = sum(t^3 - t) over the pooled tie groups, exact.  n.x < 50, n.y < 50 and T = 0: p = min(2 P, 1), P the exact
 *   Mann-Whitney tail on W's side (upper P(W' >= W) if 2W > n.x n.y, else lower P(W' <= W)) CORRECTLY ROUNDED from 128-bit
 *   integer counts (R sums rounded cwilcox terms over a choose() from lgamma: it may differ in the last bits).  Otherwise
 *   z = W - n.x n.y / 2; SIGMA = sqrt((n.x n.y / 12) ((n.x + n.y + 1) - T / ((n.x + n.y) (n.x + n.y - 1))));
 *   z = (z - sign(z) 0.5) / SIGMA; p = 2 min(pnorm(z), pnorm(z, lower = FALSE)), pnorm_both's non-log branches with exp_lib
 *   (lib_math.h, 0 below -708).
 * ICNV_DE_T: Welch, NaN dropped, +-Inf kept.  mean = correctly rounded sum / n; var = (correctly rounded sum of
 *   round(round(x - mean)^2)) / (n - 1); sx = sqrt(vx / nx); se = sqrt(sx sx + sy sy); df = (se^2)^2 / ((sx^2)^2 / (nx - 1) +
 *   (sy^2)^2 / (ny - 1)) (R: powl(se, 4)); t = (mx - my) / se; p = I_{df / (df + t^2)}(df / 2, 1 / 2) = 2 pt(-|t|, df) by the
 *   continued fraction of the regularized incomplete beta (modified Lentz, at most ICNV_DE_CF_MAX_ITER steps, symmetric form
 *   above (a + 1) / (a + b + 2)), its prefactor exp_lib(a log x + b log(1 - x) - lbeta) from the table log, a series log1p and
 *   Stirling's series for lgamma(a) - lgamma(a + 1/2).  p is NaN (R: NA) when nx < 2, ny < 2, either sample holds +-Inf, or
 *   se < 10 eps max(|mx|, |my|).
 * BH per row: n = # non-NaN p; padj = min(1, min over q >= p of fl(n / #(p' <= q)) q); NaN stays NaN.
 * Genes run in waves within ICNV_DE_SCRATCH_MB (default 8192) of sort scratch; no wave split changes a bit.
 * Limits: 1 <= G, C < 2^31, groups non-empty, indices in range, known test: ICNV_ERR_ARG before any launch.  Synchronises. */
#define ICNV_DE_WILCOXON 1
#define ICNV_DE_T 2
#define ICNV_DE_JITTER_TOKEN 0x6E6F6E44456A6974ull   /* "nonDEjit" */
#define ICNV_DE_CF_MAX_ITER 20000
int icnv_de_tests_dev(const double *expr, int64_t G, int64_t C, int64_t ld, const int32_t *cell_idx, const int32_t *cell_off,
                      int32_t n_groups, const int32_t *cmp, int32_t n_cmp, int32_t test, int32_t jitter, uint64_t seed,
                      double *stat, double *p, double *padj, void *stream);
/* The same with a HOST matrix (ld = G) and HOST outputs. */
int icnv_de_tests(const double *expr, int64_t G, int64_t C, const int32_t *cell_idx, const int32_t *cell_off, int32_t n_groups,
                  const int32_t *cmp, int32_t n_cmp, int32_t test, int32_t jitter, uint64_t seed, double *stat, double *p,
                  double *padj);
/* .mask_DE_genes (R/inferCNV_mask_non_DE.R:77-134): count(g, c) = base[c] + #{k in the comparisons of cell c
 * (cc_idx[cc_off[c] .. cc_off[c+1]]): padj[k, g] < p_val_thresh} (the caller sets base = N for reference cells and the cells
 * of subclusters under 5 cells, and lists only the comparisons of the other subclusters); out = mask value where
 * count == 0 (ANY), count < N / 2 (MOST) or count != N (ALL), expr elsewhere.  use_mean: the mask value is the correctly
 * rounded mean of the whole G x C matrix, else mask_val; *mean_out (HOST, optional) receives the value used.  out may be
 * expr (same ld).  padj, expr, out: DEVICE; base, cc_off, cc_idx: HOST.  Synchronises. */
#define ICNV_DE_MASK_ANY 0
#define ICNV_DE_MASK_MOST 1
#define ICNV_DE_MASK_ALL 2
int icnv_mask_non_de_dev(const double *expr, int64_t G, int64_t C, int64_t ld, const double *padj, int32_t n_cmp,
                         double p_val_thresh, const int32_t *base, const int32_t *cc_off, const int32_t *cc_idx, int32_t n_normal,
                         int32_t rule, int32_t use_mean, double mask_val, double *out, int64_t ld_out, double *mean_out,
                         void *stream);
/* The same with HOST expr / padj / out (ld = ld_out = G). */
int icnv_mask_non_de(const double *expr, int64_t G, int64_t C, const double *padj, int32_t n_cmp, double p_val_thresh,
                     const int32_t *base, const int32_t *cc_off, const int32_t *cc_idx, int32_t n_normal, int32_t rule,
                     int32_t use_mean, double mask_val, double *out, double *mean_out);
/* Counters since the last reset: out[0] calls, [1] comparisons, [2] genes, [3] segments sorted in LDS (<= 4096 values),
 * [4] segments merged through HBM, [5] waves, [6] wall microseconds of the test calls. */
int icnv_de_stats(int64_t *out, int32_t n);
void icnv_de_stats_reset(void);

/* ---- Bayesian filter of the predicted CNV regions (K13) -----------------------------------------------------------------
 * inferCNVBayesNet (R/inferCNV_BayesNet.R:1054-1107 with the model file inst/BUGS_Mixture_Model, steps 18-19 of run()): per
 * predicted region -- one contiguous gene run x the cells of one cell group -- a K-state mixture with FIXED state means
 * mu[k] and precisions tau[k]: every cell has one state eps[c], the values of its genes are Normal(mu[eps[c]], 1 / tau[eps[c]]),
 * eps[c] ~ Categorical(theta), theta ~ Dirichlet(1, .., 1).  The reference samples it with JAGS; this library owns a Gibbs
 * sampler of the same posterior with its own documented random stream, so results are reproducible here and statistically,
 * not bit-wise, those of JAGS.  DESIGN.md section 4 K13, restated in tests/bayes_restate.py.
 * Regions: gene_start / gene_count (HOST, rows gene_start[r] .. + gene_count[r] - 1), cell_idx / cell_off (HOST, int32 columns
 * and int64 offsets, cell_off[0] = 0); region r's cells are the rows cell_off[r] .. cell_off[r + 1] - 1 of every per-cell
 * output, in the order given.  Element (gene g, cell c) at expr[c * ld + g]; the values of a region must be finite.
 * icnv_bayes_loglik: per (row, state k), every operation rounded by itself:
 *   ssq = 0; for g in gene order: d = x - mu[k]; ssq = ssq + d * d
 *   ll[row, k] = (gene_count * 0.5) * log_lib(tau[k]) - (tau[k] * 0.5) * ssq          (log_lib: the library's table log)
 *   m = max_k ll[row, .];  L[row, k] = exp_lib(ll[row, k] - m)     (exp_lib of lib_math.h: 0 below -708, so L is 1 at the
 *   maximum and exactly 0 for every state more than 708 below it).  ll, L: DEVICE [rows x K] doubles, row-major.
 * icnv_bayes_sample: K chains per region; chain ch starts from eps == ch (n[ch] = the region's cell count, 0 elsewhere) and
 *   runs n_adapt + n_burn discarded and then n_keep kept iterations t = 0, 1, ..  Every draw is the start of its own stream
 *   of NumPy's Generator(Philox(key = [seed, token[r]], counter = [0, w1, t, w3])).random(); token[r] identifies the region
 *   (the callers here pass fnv1a64 of its name), so a region's output does not depend on the other regions of the call.
 *   theta: for k = 0 .. K-1, g[k] ~ Gamma(1 + n[k], 1) by Marsaglia-Tsang: d = shape - 1/3, c = 1 / sqrt(9 d); attempt
 *     j = 0, 1, .. takes u1, u2 from the stream w1 = k, w3 = ch 2^40 + 2^32 + j: u1 = 0 rejects; x = qnorm(u1) (AS 241 with
 *     log_lib); v = 1 + c x; v <= 0 rejects; v = (v v) v; accept d v if u2 < 1 - 0.0331 ((x x) (x x)), else if
 *     log_lib(u2) < 0.5 (x x) + d ((1 - v) + log_lib(v)) (u2 = 0: log_lib gives -inf, which accepts).  After
 *     ICNV_BAYES_GAMMA_ATTEMPTS rejections g[k] = d.  S = ((g[0] + g[1]) + ..) + g[K-1]; theta[k] = g[k] / S.
 *   cells: for row i of the region (0-based), u from the stream w1 = i, w3 = ch 2^40; w[k] = theta[k] L[i, k];
 *     cum[k] = cum[k-1] + w[k] (cum[-1] = 0); eps = the first k with cum[k] > u cum[K-1]; if there is none the last k with
 *     w[k] > 0, else the last k with L[i, k] > 0, else 0.  Then n[k] = #{i: eps[i] = k}.
 *   kept iterations: theta goes to theta_samples[r, ch, t - n_adapt - n_burn, .] (DEVICE, optional), is added to
 *   theta_sum[r, ch, .] (sequentially in t, from 0), and freq[row, eps] += 1 (DEVICE int32 [rows x K], all chains together).
 *   A region without cells: NaN theta_sum and theta_samples, nothing else.
 *   A cell with exactly one L > 0 has the same eps whatever theta and u are; it is counted once and never visited.
 *   ICNV_BAYES_DECIDED=0 (environment) visits every cell instead: the output is identical.
 *   Residency classes, by a region's undecided cells: more than 512 stream their L rows from memory, up to 512 keep them in
 *   LDS (one workgroup per (region, chain)), and a region with cells of which at most 8 are undecided -- every region of a
 *   per-cell report -- is sampled by an 8-lane group, eight (region, chain) pairs to a wavefront, in registers (K25).  Every
 *   draw has its own counter, S and the kept-theta sums are sequential, freq is integer: the class does not show in the output.
 *   ICNV_BAYES_PACKED=0 (environment, read per call) sends the third class down the LDS path.
 * Limits: 2 <= K <= 8 (more: ICNV_ERR_UNSUPPORTED), tau > 0, indices in range: ICNV_ERR_ARG before any launch.  Synchronises. */
#define ICNV_BAYES_GAMMA_ATTEMPTS 64
int icnv_bayes_loglik_dev(const double *expr, int64_t G, int64_t C, int64_t ld, const int32_t *gene_start, const int32_t *gene_count,
                          const int32_t *cell_idx, const int64_t *cell_off, int32_t n_regions, int32_t K, const double *mu,
                          const double *tau, double *ll, double *L, void *stream);
/* The same with a HOST matrix (ld = G) and HOST outputs. */
int icnv_bayes_loglik(const double *expr, int64_t G, int64_t C, const int32_t *gene_start, const int32_t *gene_count,
                      const int32_t *cell_idx, const int64_t *cell_off, int32_t n_regions, int32_t K, const double *mu, const double *tau,
                      double *ll, double *L);
int icnv_bayes_sample_dev(const double *L, const int64_t *cell_off, const uint64_t *token, int32_t n_regions, int32_t K, int32_t n_adapt,
                          int32_t n_burn, int32_t n_keep, uint64_t seed, double *theta_sum, double *theta_samples, int32_t *freq,
                          void *stream);
/* The same with HOST L and HOST outputs. */
int icnv_bayes_sample(const double *L, const int64_t *cell_off, const uint64_t *token, int32_t n_regions, int32_t K, int32_t n_adapt,
                      int32_t n_burn, int32_t n_keep, uint64_t seed, double *theta_sum, double *theta_samples, int32_t *freq);
/* Counters since the last reset: out[0] sample calls, [1] regions, [2] (region, cell) rows, [3] undecided rows, [4] regions
 * with <= 512 undecided cells (the packed ones included), [5] regions streamed, [6] wall microseconds of the sample calls,
 * [7] of the likelihood calls, [8] regions sampled by the packed kernel (cells, <= 8 of them undecided). */
int icnv_bayes_stats(int64_t *out, int32_t n);
void icnv_bayes_stats_reset(void);

/* The rectangle rewrite of the Bayesian filter (removeCNV / reassignCNV, R/inferCNV_BayesNet.R:562-630, 491-540) for every
 * region of a run in one launch (K25).  states: DEVICE uint8, element (gene g, cell c) at states[c * ld + g], ld >= G.  Region
 * r is the genes gene_first[r] .. + gene_count[r] - 1 (gene_count >= 1) x the cells cell_idx[cell_off[r] .. cell_off[r + 1] - 1];
 * every byte of the rectangle becomes value[r], and value[r] == 0 leaves it alone.  gene_first, gene_count (int32), cell_off
 * (int64, n_regions + 1, from 0, monotone), cell_idx (int32, n_idx entries, cell_off[n_regions] <= n_idx) and value (uint8)
 * are DEVICE arrays.  The rectangles of one call must be DISJOINT: overlap is not detected, and which value an overlapped
 * byte keeps is not defined.  Every index is checked on the device before anything is written: ICNV_ERR_ARG leaves states
 * untouched.  The check synchronises the stream; the fill itself is left running on it. */
int icnv_state_fill_regions_dev(uint8_t *states, int64_t G, int64_t C, int64_t ld, int32_t n_regions, const int32_t *gene_first,
                                const int32_t *gene_count, const int64_t *cell_off, const int32_t *cell_idx, int64_t n_idx,
                                const uint8_t *value, void *stream);

/* ---- MCMC convergence diagnostics of the Bayesian filter's chains (K31) ---------------------------------------------------
 * What mcmcDiagnosticPlots (R/inferCNV_BayesNet.R:866-990, diagnostics = TRUE) asks of coda, as numbers: per region, state and
 * chain the mean, variance, spectral density at zero, Geweke score and autocorrelations; per region and state the pooled
 * moments and quantiles, Gelman-Rubin's potential scale reduction factor and the effective sample size.  The contract is THIS
 * LIBRARY'S OWN, modelled on coda (spectrum0.ar, geweke.diag, autocorr, gelman.diag, effectiveSize as read from its sources):
 * believed, not verified against coda -- no R run stands behind it.  DESIGN.md section 4 K31, restated in
 * tests/mcmc_diag_restate.py.  Plots (trace, density, autocorrelation, Gelman) stay in R.  Not bound in the R shim.
 * theta_samples: DEVICE doubles [n_regions, n_chains, n_keep, K] exactly as icnv_bayes_sample_dev lays them out (there
 *   n_chains == K; here it is a parameter of its own).  Outputs, DEVICE doubles:
 *   chain_stats [n_regions, K, n_chains, 9]: mean, var, spec0, order, geweke, acf1, acf5, acf10, acf50
 *   pooled      [n_regions, K, 7]:           mean, sd, q2.5, q50, q97.5, psrf, ess
 * Every operation below is one rounded IEEE-754 double operation, every sum runs sequentially in t from s = 0 (no FMA).
 * One series x[0 .. n-1] (region, state k, chain ch; n = n_keep).  A WINDOW is a range t = lo .. lo + m - 1 of it:
 *   mean  = (sum_t x[t]) / m
 *   c[l]  = (sum_{t = lo .. lo + m - 1 - l} (x[t] - mean) * (x[t + l] - mean)) / m     for l = 0 .. P,
 *           P = min(m - 1, floor(10 log10 m)), the floor in integers: the largest p with 10^p <= m^10
 *   AR fit (spectrum0.ar: Yule-Walker by Levinson-Durbin, order by AIC).  c[0] == 0: spec0 = 0, order = 0, nothing is fitted.
 *     c[0] NaN: both NaN.  Else v_0 = c[0], crit_0 = m * log_lib(v_0) + 0, and for p = 1 .. P:
 *       acc = c[p]; for j = 1 .. p-1: acc = acc - phi_{p-1}[j] * c[p - j];   k = acc / v_{p-1}
 *       phi_p[j] = phi_{p-1}[j] - k * phi_{p-1}[p - j]  (j = 1 .. p-1),  phi_p[p] = k;   v_p = v_{p-1} * (1 - k * k)
 *       crit_p = m * log_lib(v_p) + 2 * p                      (log_lib: the library's table log, K13)
 *     order = the p with the smallest crit_p, the first on ties (a NaN crit_p is never chosen);
 *     var_pred = (v_p * m) / (m - (p + 1));  S = ((phi_p[1] + phi_p[2]) + ..) + phi_p[p] (0 for p = 0);  d = 1 - S;
 *     spec0 = var_pred / (d * d)
 *   Windows: the whole series (lo = 0, m = n); Geweke's A: t in [0, ceil((n - 1) / 10)]; B: t in [floor((n - 1) / 2), n - 1]
 *   (integer arithmetic; each with its own mean, c, P and AR fit).
 *   chain_stats: mean, spec0 and order of the whole series;  var = (the sum of c[0], before its division by n) / (n - 1);
 *     geweke = (mean_A - mean_B) / sqrt(spec0_A / m_A + spec0_B / m_B);
 *     acf1, acf5, acf10 = c[1], c[5], c[10] over c[0];  acf50 = ((sum as for c[50]) / n) / c[0], NaN when n <= 50.
 * Pooled, over the N = n_chains n draws of a (region, state) in (chain, t) order:
 *   mean = (sum x) / N;  sd = sqrt((sum (x - mean) * (x - mean)) / (N - 1))
 *   q2.5, q50, q97.5: quantile(type = 7) at 0.025, 0.5, 0.975 in the operation order of icnv_quantiles_excluding (-0.0 counts
 *     as +0.0); NaN when any draw is NaN.
 *   psrf (gelman.diag's point estimate, transform = FALSE), from the chains' mean_i and var_i (m = n_chains), sums in chain order:
 *     W = (sum var_i) / m;  W not > 0: psrf = NaN.  mu = (sum mean_i) / m;  B = n * ((sum (mean_i - mu)^2) / (m - 1))
 *     var_w = ((sum (var_i - W)^2) / (m - 1)) / m;  var_b = (2 * (B * B)) / (m - 1);  q = (sum mean_i * mean_i) / m
 *     cov_wb = (n / m) * ((sum (var_i - W) * (mean_i * mean_i - q)) / (m - 1) - (2 * mu) * ((sum (var_i - W) * (mean_i - mu)) / (m - 1)))
 *     f = 1 + 1 / m;  V = ((n - 1) * W) / n + (f * B) / n
 *     var_V = ((((n-1) * (n-1)) * var_w + (f * f) * var_b) + ((2 * (n-1)) * f) * cov_wb) / (n * n);  df = (2 * (V * V)) / var_V
 *     psrf = sqrt(((df + 3) / (df + 1)) * ((n - 1) / n + (f * (1 / n)) * (B / W)))
 *   ess = sum over the chains, in order, of (n * var_i) / spec0_i; a chain with spec0_i == 0 contributes 0.
 * Degenerate input is ordinary input.  A region without cells has NaN samples: every output is NaN.  A constant series (the
 *   sum of its draws divides back to the draw exactly, so c[0] == 0): mean = the value, var = 0, spec0 = 0, order = 0, geweke
 *   and the acf NaN (0 / 0), ess contribution 0; all chains constant: W = 0 and psrf = NaN.  Chains with equal means and
 *   variances give var_V = 0 and psrf = NaN, as the formula does in coda.
 * Deviations from coda: psrf is computed over ALL kept iterations (gelman.diag's autoburnin halves the chain first; the burn-in
 *   is already discarded here); the upper confidence limit of the psrf (an F quantile) is not built; the window ends are
 *   integers, where coda matches times with a tolerance.
 * Refusals before any launch: a null pointer, n_regions < 1, K or n_chains outside 2 .. 8, n_keep < 20 (the Geweke windows
 *   need it): ICNV_ERR_ARG.  n_chains * n_keep > 8192 (the pooled draws are sorted in LDS; no memory fallback), or more than
 *   2^31 - 1 (region, state) pairs: ICNV_ERR_UNSUPPORTED.  Synchronises.  Timer name: "mcmc_diag". */
int icnv_mcmc_diag_dev(const double *theta_samples, int32_t n_regions, int32_t n_chains, int32_t n_keep, int32_t K, double *chain_stats,
                       double *pooled, void *stream);
/* The same with HOST samples and HOST outputs. */
int icnv_mcmc_diag(const double *theta_samples, int32_t n_regions, int32_t n_chains, int32_t n_keep, int32_t K, double *chain_stats,
                   double *pooled);

/* ---- Probability heatmaps and tables of the Bayesian filter (K33) ---------------------------------------------------------
 * The numbers under postProbNormal's heatmaps and plotProbabilities' PDFs (R/inferCNV_BayesNet.R:757-844, 1110-1190).  The
 * pages, axes and text stay in R.  Not bound in the R shim.
 *
 * icnv_paint_regions_dev: postProbNormal's matrix -- expr.data[,] <- 0, then for region r in order
 * expr.data[Genes_r, Cells_r] <- value[r] -- for every region of a run at once.  The float64 sibling of
 * icnv_state_fill_regions_dev, with its argument conventions: out is DEVICE doubles, element (gene g, cell c) at
 * out[c * ld + g], ld >= G; gene_first, gene_count (int32), cell_off (int64, n_regions + 1, from 0, monotone), cell_idx
 * (int32, n_idx entries, cell_off[n_regions] <= n_idx) and value (doubles) are DEVICE arrays.  Region r covers the genes
 * gene_first[r] .. + gene_count[r] - 1 of the cells cell_idx[cell_off[r] .. cell_off[r + 1] - 1].  Afterwards, for g < G:
 *   out[c * ld + g] = +0.0 where no region covers (g, c), else value[r] of the HIGHEST r that covers it (R's loop: the last
 *   writer wins), with value[r]'s bits as they are (-0.0, NaN).  Regions may overlap and may list a cell twice.
 *   The padding columns g >= G are not touched.  gene_count[r] == 0 or an empty cell list paints nothing; n_regions == 0
 *   gives the zero matrix (the region arrays may then be null).
 * Every index is checked on the device before a byte of out is written (0 <= gene_first, 0 <= gene_count, gene_first +
 * gene_count <= G, 0 <= cell < C, the offsets' rules above): ICNV_ERR_ARG leaves out untouched.  The result does not depend on
 * the launch geometry and no floating-point atomic is used: on the zeroed matrix every covered element takes the unsigned
 * 64-bit integer maximum of r + 1 over its regions, and a second pass replaces every non-zero owner o by value[o - 1].  The
 * check synchronises the stream; the paint itself is left running on it.  Timer names: "paint_check", "paint_regions". */
int icnv_paint_regions_dev(double *out, int64_t G, int64_t C, int64_t ld, int32_t n_regions, const int32_t *gene_first,
                           const int32_t *gene_count, const int64_t *cell_off, const int32_t *cell_idx, int64_t n_idx,
                           const double *value, void *stream);

/* icnv_theta_box_dev: the box statistics of plot_cnv_prob's box plot, per (region, state) over the pooled kept theta draws.
 * The library's own contract, modelled on ggplot2's stat_boxplot (coef = 1.5): believed, not verified against ggplot2.
 * Restated sequentially in tests/bayes_probs_restate.py.
 * theta_samples: DEVICE doubles [n_regions, n_chains, n_keep, K] exactly as icnv_bayes_sample_dev lays them out.
 * box: DEVICE doubles [n_regions, K, 7] = ymin, lower, middle, upper, ymax, n_low, n_high.
 * Over the N = n_chains n_keep draws y of a (region, state), ascending with -0.0 counted as +0.0:
 *   lower, middle, upper = quantile(type = 7) at 0.25, 0.5, 0.75 in the operation order of icnv_quantiles_excluding, as the
 *     pooled quantiles of icnv_mcmc_diag_dev (stat_boxplot's quantiles at 0 and 1 are the extremes, which it then replaces by
 *     ymin and ymax below: they are not formed);
 *   iqr = upper - lower;  lo = lower - 1.5 * iqr;  hi = upper + 1.5 * iqr   (every operation rounded by itself, no FMA);
 *   n_low = #{y < lo}, n_high = #{y > hi} (strict comparisons; stored as doubles);
 *   ymin, ymax = the smallest and the largest draw inside [lo, hi] (NaN if there is none, which needs infinite draws).
 * A (region, state) with a NaN draw -- a region without cells -- gives NaN in all seven fields.  A constant series gives five
 * equal numbers and no outliers.
 * Refusals before any launch: a null pointer, n_regions < 0, n_keep < 1, K or n_chains outside 2 .. 8: ICNV_ERR_ARG.
 * N > 8192 (the draws are sorted in LDS by the sort of icnv_mcmc_diag_dev; no memory fallback) or more than 2^31 - 1 (region,
 * state) pairs: ICNV_ERR_UNSUPPORTED.  n_regions == 0 does nothing.  Synchronises.  Timer name: "theta_box". */
int icnv_theta_box_dev(const double *theta_samples, int32_t n_regions, int32_t n_chains, int32_t n_keep, int32_t K, double *box,
                       void *stream);

/* ---- per-cell CNV features and run-length segmentation (K14) -------------------------------------------------------------
 * The numbers behind add_to_seurat's map_metadata_from_infercnv.txt (.get_features, R/seurat_interaction.R:244-353) and the
 * segmentation of state columns into CNV regions (.define_cnv_gene_regions, R/inferCNV_HMM.R:1005-1057, called per cell
 * group by get_predicted_CNV_regions, :706-764).  DESIGN.md section 4 K14, restated in tests/cnv_summary_restate.py.
 * states: uint8, element (gene g, column c) at states[c * ld + g], ld >= G (a leading dimension that is a multiple of 16 on a
 * 16-byte aligned base is read with 16-byte loads); chr_start: HOST, n_chr + 1 entries from 0 to G, non-decreasing (the
 * kernels see contiguous chromosomes only).  A chromosome of fewer than two genes never appears in a report
 * (R/inferCNV_HMM.R:1013): it counts nothing, produces no run and does not advance the region counter.
 * icnv_cnv_features: per (chromosome k, column c) four int32 at counts[(k * C + c) * 4 ..] (DEVICE and 16-byte aligned in the
 *   _dev flavour, else ICNV_ERR_ARG: a group of four is stored at once):
 *   n_loss = #{genes of k with state < s0}, n_gain = #{state > s0}, d_loss = sum of s0 - state over the former, d_gain = sum
 *   of state - s0 over the latter.  s0 is the centre state (3 for i6, 2 for i3).  The nine features of the reference are
 *   has_loss = n_loss > 0, has_dupli = n_gain > 0, has_cnv = n_loss + n_gain > 0, proportion_loss = n_loss / n_k,
 *   proportion_dupli = n_gain / n_k, proportion_cnv = (n_loss + n_gain) / n_k and, for i6, proportion_scaled_loss =
 *   d_loss / (2 n_k), _dupli = d_gain / (2 n_k), _cnv = (d_loss + d_gain) / (2 n_k): one correctly rounded division each.
 *   The reference's reports hold a cell group's CONSENSUS state, so in group mode the columns passed here are the consensus
 *   columns of icnv_state_consensus and the caller broadcasts the result to the member cells; groups must not overlap.
 *   run_counts (nullable; DEVICE in the _dev flavour): per column c, run_counts[2 c] = runs of equal states within the
 *   chromosomes of two or more genes (a run ends at a chromosome border whatever the states are), run_counts[2 c + 1] =
 *   those whose state is not s0.  Every byte of the matrix must be a state 1 .. K (2 <= K <= 7): any other byte, the
 *   library's 0xFF "invalid" included, gives ICNV_ERR_ARG and no number.
 * icnv_cnv_runs: the runs themselves.  col_idx (HOST, nullable = every column in order): the columns to visit, in report order
 *   (by cell that is reference groups first, then observation groups, R/inferCNV_HMM.R:713-733).  One record per run whose
 *   state is not `neutral` (neutral = 0: every run), ordered by (list position, gene), as six int32 arrays of `capacity`
 *   entries each, records[f * capacity + r]: f = 0 list position, 1 chromosome index, 2 first gene, 3 last gene (0-based,
 *   inclusive), 4 state, 5 ordinal = the 1-based counter of "<chr>-region_<k>": it counts neutral runs too and runs on across
 *   the list.  *n_records receives the number of records, *n_runs (nullable) the number of runs of every state.
 *   records = NULL is the count-only call.  capacity < *n_records: ICNV_ERR_ARG, nothing written.  run_counts (_dev, DEVICE
 *   [2 C], nullable): receives the per-column counts; with counts_valid != 0 it holds them already (from icnv_cnv_features_dev
 *   with s0 = neutral, or from the count-only call) and the counting pass is skipped.  K = 0: bytes are compared as they
 *   are (0xFF is a state like any other); K >= 1: as above, ICNV_ERR_ARG for a byte outside 1 .. K.
 *   Ties between regions of equal gene count are not decided here: infercnv_amd/seurat_interaction.py orders them by the
 *   bytes of the region name ("chr1-region_9" before "chr10-region_2"), where the reference's order depends on R's locale.
 * Both synchronise. */
int icnv_cnv_features_dev(const uint8_t *states, int64_t G, int64_t C, int64_t ld, const int32_t *chr_start, int32_t n_chr, int32_t K,
                          int32_t s0, int32_t *counts, int32_t *run_counts, void *stream);
/* The same with a HOST matrix (ld = G) and HOST outputs. */
int icnv_cnv_features(const uint8_t *states, int64_t G, int64_t C, const int32_t *chr_start, int32_t n_chr, int32_t K, int32_t s0,
                      int32_t *counts, int32_t *run_counts);
int icnv_cnv_runs_dev(const uint8_t *states, int64_t G, int64_t C, int64_t ld, const int32_t *chr_start, int32_t n_chr,
                      const int32_t *col_idx, int64_t n_cols, int32_t K, int32_t neutral, int32_t *run_counts, int32_t counts_valid,
                      int64_t capacity, int32_t *records, int64_t *n_records, int64_t *n_runs, void *stream);
/* The same with a HOST matrix (ld = G) and HOST records. */
int icnv_cnv_runs(const uint8_t *states, int64_t G, int64_t C, const int32_t *chr_start, int32_t n_chr, const int32_t *col_idx,
                  int64_t n_cols, int32_t K, int32_t neutral, int64_t capacity, int32_t *records, int64_t *n_records, int64_t *n_runs);

/* ---- hidden spike-in of the i6 HMM (K15) ---------------------------------------------------------------------------------
 * .build_and_add_hspike (R/inferCNV_hidden_spike.R:3-165, step 3 of run()): the per-group gene tables the two smoothing
 * splines are fitted to, and the simulation of the normal and CNV-spiked cells from them.  The splines themselves are fitted
 * on the host (infercnv_amd/smooth_spline.py).  R's draws are unseeded, so the library owns a documented Philox stream.
 * DESIGN.md section 4 K15, restated in tests/hspike_restate.py.
 * icnv_group_gene_tables: .get_mean_var_table / .get_mean_vs_p0_table (R/inferCNV_meanVarSim.R:178-211,
 *   R/inferCNV_simple_sim.R:100-154).  Groups: cell_idx / cell_off (HOST, int32, 0-based columns, cell_off[0] = 0, no group
 *   empty; groups may overlap, cells in no group are never read).  Element (gene g, cell c) at expr[c * ld + g].  Outputs
 *   [n_grp x G] (row q = group q): m = rowMeans, v = apply(, 1, var), nzero = sum(x == 0) (int32; -0 counts).  The arithmetic
 *   is ICNV_DE_T's: m = correctly rounded sum / n (bit-equal to icnv_group_means_dev); v = (correctly rounded sum of
 *   round(round(x - m)^2)) / (n - 1); n = 1 gives v = NaN as R's var does.  R's var accumulates in long double around a
 *   long-double mean: it may differ from v in the last bits.  p0 = nzero / n is one division on the host.  A non-finite value
 *   makes m and v of its (group, gene) non-finite by plain IEEE sums; their bits are not part of the contract.  Every
 *   (group, cell) membership is read twice (sums, then squared deviations): disjoint groups read the matrix at most twice.
 *   1 <= n_grp <= 65535, 1 <= G, C < 2^31: ICNV_ERR_ARG before any launch.  Synchronises.
 * spline evaluation S(x) of (knots [nk + 4], coef [nk], nk >= 4, xmin, range): a cubic B-spline on the scaled abscissa
 *   t = (x - xmin) / range with knots[0..3] = 0, knots[nk..nk+3] = 1 and knots[3..nk] strictly increasing.
 *   t < 0: coef[0] + ((3 (coef[1] - coef[0])) / (knots[4] - knots[3])) t;
 *   t > 1: coef[nk-1] + ((3 (coef[nk-1] - coef[nk-2])) / (knots[nk] - knots[nk-1])) (t - 1) -- the boundary value and the first
 *   derivative in t, as predict.smooth.spline.fit extends linearly;
 *   else i = the largest index in 3 .. nk - 1 with knots[i] <= t (bisection) and de Boor's recurrence on d[j] = coef[i - 3 + j]:
 *   for r = 1, 2, 3: for j = 3 down to r: a = (t - knots[i-3+j]) / (knots[i+1+j-r] - knots[i-3+j]);
 *   d[j] = ((1 - a) d[j-1]) + (a d[j]); S = d[3].  Every operation is rounded by itself, in this order.
 * icnv_hspike_simulate: .get_simulated_cell_matrix_using_meanvar_trend_helper + .apply_dropout
 *   (R/inferCNV_meanVarSim.R:23-55, 105-161) for n_mat matrices at once.  means [n_mat x n_genes] (HOST), tokens [n_mat] (HOST),
 *   the variance spline S_var (log(v + 1) over log(m + 1)) and the dropout spline S_p0 (p0 over log(m)) (HOST arrays); out:
 *   n_mat matrices of n_genes x num_cells, column-major, element (g, c) of matrix k at out[(k num_cells + c) n_genes + g]
 *   (DEVICE in the _dev flavour).  Per gene row g with mean m: m <= 0: every value is 0.  Else logm = lib_log(m + 1),
 *   var = max(lib_exp(S_var(logm)) - 1, 0), sd = sqrt(var); per cell c: u1, u2 = two .random() draws of NumPy's
 *   Generator(Philox(key = [seed, token_k], counter = [0, g, c, 0])), z = lib_qnorm((floor(2^27 u1) + u2) / 2^27) (K12's normal
 *   draw), w = m + sd z, val = rint(w > 0 ? w : 0) (R >= 4 rounds half to even).  Dropout of the row: sum = the sequential double
 *   sum of val over c (exact below 2^53; means above 2^40 are refused), nz = #(val == 0); nz = num_cells: the row stays (R
 *   divides by zero there: a deviation); p = S_p0(lib_log(sum / n)), padj = (p n - nz) / (n - nz); padj > 0: the element becomes 0
 *   where u <= padj, u the first .random() draw of counter = [1, g, c, 0] (R draws for every element; with padj <= 0 nothing can
 *   drop, so no draw is taken).  lib_log / lib_exp / lib_qnorm: csrc/lib_math.h.
 *   ICNV_ERR_ARG with a message before any launch: nk < 4, a non-finite coefficient, xmin or range, range <= 0, knots that are
 *   not as above, a non-finite mean, a mean above 2^40, n_mat outside 1 .. 65535.  Synchronises. */
#define ICNV_HSPIKE_GENES_TOKEN 0x6873706B67656E65ull   /* "hspkgene": the stream of genes_means_use_idx (hidden_spike.py) */
int icnv_group_gene_tables_dev(const double *expr, int64_t G, int64_t C, int64_t ld, const int32_t *cell_idx, const int32_t *cell_off,
                               int32_t n_grp, double *m, double *v, int32_t *nzero, void *stream);
/* The same with a HOST matrix (ld = G) and HOST outputs. */
int icnv_group_gene_tables(const double *expr, int64_t G, int64_t C, const int32_t *cell_idx, const int32_t *cell_off, int32_t n_grp,
                           double *m, double *v, int32_t *nzero);
int icnv_hspike_simulate_dev(const double *means, int64_t n_genes, int32_t num_cells, int32_t n_mat, const double *var_knots,
                             const double *var_coef, int32_t var_nk, double var_xmin, double var_range, const double *p0_knots,
                             const double *p0_coef, int32_t p0_nk, double p0_xmin, double p0_range, uint64_t seed,
                             const uint64_t *tokens, double *out, void *stream);
/* The same with a HOST output. */
int icnv_hspike_simulate(const double *means, int64_t n_genes, int32_t num_cells, int32_t n_mat, const double *var_knots,
                         const double *var_coef, int32_t var_nk, double var_xmin, double var_range, const double *p0_knots,
                         const double *p0_coef, int32_t p0_nk, double p0_xmin, double p0_range, uint64_t seed, const uint64_t *tokens,
                         double *out);

/* ---- window smoothers of step 10 (K16) -----------------------------------------------------------------------------------
 * smooth_method = "runmeans" (smooth_by_chromosome_runmeans, R/inferCNV_ops.R:2679-2704) and "coordinates"
 * (smooth_by_chromosome_coordinates, :2534-2622) are one banded window operator; the windows and weights do not depend on
 * the cell and are built on the host (infercnv_amd/smooth_windows.py).  DESIGN.md section 4 K16, restated in
 * tests/smooth_windows_restate.py.  Not yet bound in the R shim.
 *   out[g, c] = ( sum over t = 0 .. len[g] - 1 of  x[lo[g] + t, c] * w[w_off[g] + t] ) / denom[g]
 * The sum starts at +0.0 and runs SEQUENTIALLY in t, in doubles: one rounding per product, one per add (no FMA), and one
 * division at the end.  w = NULL means all weights 1.0 (w_off is then not read); x * 1.0 is exact, so both forms give the
 * same bits.  Bit equality with R is not claimed: caTools::runmean keeps a compensated running sum and R's sum() accumulates
 * in long double.
 * Tables (HOST arrays; the library uploads them): lo, len [G] int32; w_off [G + 1] int64, window g's weights at
 * w[w_off[g] .. w_off[g] + len[g]) with w_off[g + 1] >= w_off[g] + len[g] (a CSR: the rows of neighbouring genes follow each
 * other); w [w_off[G]]; denom [G].
 * _dev flavour: expr_in / expr_out are DEVICE matrices, element (g, c) at expr_in[c * ld_in + g] / expr_out[c * ld_out + g]
 * (ld >= G: the padded_matrix layout of infercnv_amd/device.py); the padding is never read or written.
 * ICNV_ERR_ARG before any launch, outputs untouched: a null argument, G or C outside 1 .. 2^31 - 1, ld < G, lo < 0, len < 1,
 *   lo + len > G, a w_off that is not monotone as above, a denom that is zero or not finite, expr_out overlapping expr_in (a
 *   window reads its neighbours, so the operator does NOT work in place).
 * ICNV_ERR_ARG after the launch, output unspecified: a value of the input that is not finite.  The kernel raises a flag word
 *   when it stages or sums such a value (every value inside a window is seen; no extra pass over the matrix).  caTools would
 *   skip such values and the reference's coordinate smoother says "No handling of NAs" (:2596); the library refuses the
 *   input, as K10 does, and does not improvise.
 * Synchronises the stream.  Timer name: "smooth_windows". */
int icnv_smooth_windows_dev(const double *expr_in, int64_t ld_in, double *expr_out, int64_t ld_out, int64_t G, int64_t C,
                            const int32_t *lo, const int32_t *len, const int64_t *w_off, const double *w, const double *denom,
                            void *stream);
/* The same with HOST matrices (ld = G).  (R/inferCNV_ops.R:2594-2622, 2691) */
int icnv_smooth_windows(const double *expr_in, double *expr_out, int64_t G, int64_t C, const int32_t *lo, const int32_t *len,
                        const int64_t *w_off, const double *w, const double *denom);
/* Counters since the last reset (R/inferCNV_ops.R:858-868), n = int64 slots (<= 6 written):
 *   out[0] calls   out[1] gene tiles staged in LDS   out[2] gene tiles read from HBM (span beyond the LDS budget)
 *   out[3] calls with weights   out[4] window rows (sum of len)   out[5] wall microseconds */
int icnv_smooth_windows_stats(int64_t *out, int32_t n);
void icnv_smooth_windows_stats_reset(void);   /* R/inferCNV_ops.R:858-868 */

/* ---- data layer of plot_cnv (K17) ---------------------------------------------------------------------------------------
 * What plot_cnv (R/inferCNV_heatmap.R) computes from the matrix: the "auto" x.range quantiles (:159), the colour key's
 * hist() (:2524) and the binned panel that image() draws.  DESIGN.md section 4 K17, restated in tests/heatmap_restate.py.
 * Not yet bound in the R shim.
 * Matrices: _dev flavours take a DEVICE matrix, element (g, c) at x[c * ld + g] with ld >= G (the padded_matrix layout of
 * infercnv_amd/device.py; the padding is never read); the flavours without _dev take a HOST matrix with ld = G.  Every other
 * array is a HOST array unless it says otherwise (the library uploads cell lists and breaks).  Element offsets are int64.
 * Common refusals, ICNV_ERR_ARG before any launch: a null argument, G or C outside 1 .. 2^31 - 1, ld < G.
 * On ANY error every output is left exactly as it was.  All calls synchronise the stream.
 *
 * icnv_quantiles_excluding: quantile(x[x != exclude], probs, type = 7), exactly.
 *   Kept values: x != exclude under IEEE comparison (exclude = NaN keeps everything; exclude = 0.0 drops -0.0 too).
 *   Order: -0.0 is canonicalised to +0.0 first, so both are one value, reported as +0.0.
 *   With n = n_kept and, per probability p:  index = (n - 1) * p  in double, lo = floor(index), hi = ceil(index), h = index - lo,
 *     quantile = x_(lo)  if index == lo or x_(hi) == x_(lo),  else (1 - h) * x_(lo) + h * x_(hi)
 *   (x_(k): the k-th smallest kept value, 0-based), evaluated on the host in that operation order, without FMA.  This is
 *   R's arithmetic as read from its sources, not checked against an R run.
 *   Outputs: quantiles [n_probs]; order_stats [2 * n_probs] = x_(lo), x_(hi) per probability (nullable); counts [2] = n_kept,
 *   n_excluded (nullable); minmax [2] = min and max over ALL values, excluded ones included (nullable; plot_cnv logs them, :131-136).
 *   ICNV_ERR_ARG: n_probs outside 1 .. 8, a probability outside [0, 1] or NaN (before any launch); a value of x that is not
 *   finite, or n_kept == 0 (found by the first pass).
 *   Method: radix selection on the order-preserving 64-bit key, 8 bits per pass.  A pass reads the matrix once and counts one
 *   digit under every tracked prefix (at most 16: a probability's lo and hi may part) into int64 totals, so the result does
 *   not depend on arrival order; the first pass also makes the non-finite check, n_kept and min / max.  Once the bins that
 *   hold the wanted ranks count <= 4096 values together, one more pass compacts them and one workgroup sorts them; a bin
 *   that never shrinks (most of the matrix is one value) is followed through all 8 digits instead.  Timer names:
 *   "heatmap_radix", "heatmap_compact", "heatmap_sort". */
int icnv_quantiles_excluding_dev(const double *x, int64_t ld, int64_t G, int64_t C, double exclude, const double *probs,
                                 int32_t n_probs, double *quantiles, double *order_stats, int64_t *counts, double *minmax,
                                 void *stream);
int icnv_quantiles_excluding(const double *x, int64_t G, int64_t C, double exclude, const double *probs, int32_t n_probs,
                             double *quantiles, double *order_stats, int64_t *counts, double *minmax);
/* icnv_heatmap_bins: hist(x[, rows], breaks = breaks)$counts (R/inferCNV_heatmap.R:2524) over the cells listed in rows
 *   [n_rows] (any order or subset; a cell listed twice counts twice).  Each value is first forced into
 *   [breaks[0], breaks[nb - 1]] (:1934-1935); bin b holds breaks[b] < v <= breaks[b + 1] and v == breaks[0] goes in bin 0
 *   (.bincode(right = TRUE, include.lowest = TRUE)).  counts [nb - 1] int64, exact, from one read of the listed rows.
 *   ICNV_ERR_ARG: nb outside 2 .. 257, a break that is not finite, breaks not strictly ascending, n_rows outside
 *   1 .. 2^31 - 1, a list entry outside 0 .. C - 1 (before any launch); a NaN in a listed row (+-Inf is clamped like any
 *   other value).  Timer name: "heatmap_bins". */
int icnv_heatmap_bins_dev(const double *x, int64_t ld, int64_t G, int64_t C, const int32_t *rows, int64_t n_rows,
                          const double *breaks, int32_t nb, int64_t *counts, void *stream);
int icnv_heatmap_bins(const double *x, int64_t G, int64_t C, const int32_t *rows, int64_t n_rows, const double *breaks, int32_t nb,
                      int64_t *counts);
/* icnv_heatmap_raster: the panel as an H x W uint8 image of bin indices (same binning), row-major, nearest-neighbour sampled
 *   as R's useRaster = TRUE at device resolution is believed to behave:
 *     pixel row i shows cell order[((2 i + 1) * n) / (2 H)],  pixel column j shows gene ((2 j + 1) * G) / (2 W)
 *   in int64 integer arithmetic; H and W may be smaller or larger than n and G.  image: DEVICE [H * W] in the _dev flavour,
 *   HOST otherwise.  Refusals as icnv_heatmap_bins, plus H or W outside 1 .. 2^31 - 1; a sampled NaN is ICNV_ERR_ARG (the
 *   panel is rendered aside and copied only on success).  Timer name: "heatmap_raster". */
int icnv_heatmap_raster_dev(const double *x, int64_t ld, int64_t G, int64_t C, const int32_t *order, int64_t n,
                            const double *breaks, int32_t nb, int64_t H, int64_t W, uint8_t *image, void *stream);
int icnv_heatmap_raster(const double *x, int64_t G, int64_t C, const int32_t *order, int64_t n, const double *breaks, int32_t nb,
                        int64_t H, int64_t W, uint8_t *image);
/* Counters since the last reset, n = int64 slots (<= 4 written):
 *   out[0] calls (of the three entry points)   out[1] radix passes   out[2] compacted candidates   out[3] wall microseconds */
int icnv_heatmap_stats(int64_t *out, int32_t n);
void icnv_heatmap_stats_reset(void);

/* ---- matrix files of plot_cnv (K20) ---------------------------------------------------------------------------------------
 * The text of `expr.<name>.dat`, `<name>.observations.txt`, `<name>.references.txt` and `General_HCL_<g>_members.txt`, which
 * plot_cnv writes with write.table (R/inferCNV_heatmap.R:147 expr.<name>.dat, :672 and :774 the members files, :906 the
 * observations, :1197 the references).  DESIGN.md section 4 K20, restated in tests/table_text_restate.py.  Not yet bound in
 * the R shim.  R's own bytes are believed, not verified against an R run: the rule below is the one K17's host writer states.
 *
 * The text of one field, for a double x:
 *   NaN gives `NaN`, +-Inf gives `Inf` / `-Inf`, +-0 gives `0`.
 *   Otherwise take the 15 significant decimal digits of |x|, correctly rounded, ties to even on the exact binary value
 *   (this is what "%.14e" gives): digits D, decimal exponent E.  Drop trailing zeros.  Use fixed notation unless scientific
 *   notation is strictly narrower.  Scientific notation is d[.ddd]e+-XX, with a two-digit exponent and three digits from 100
 *   on.  A negative number starts with `-`.  A field is at most 22 bytes.
 * A file row is the optional label bytes and the separator, then the fields joined by the separator, then `\n`.
 * Element (gene g, cell c) sits at x[c * ld + g].  Two orientations:
 *   ICNV_TABLE_GENE_ROWS  the table has G rows; file row i is gene i, its fields run over cells[0 .. n_cells) in that order.
 *   ICNV_TABLE_CELL_ROWS  the table has n_cells rows; file row i is cell cells[i], its fields run over the genes 0 .. G - 1.
 * The call formats the file rows row0 .. row0 + n_rows - 1 into `out` (capacity bytes; DEVICE in the _dev flavour, HOST
 * otherwise) and stops before the first row that does not fit: *rows_done rows (>= 1) take *n_bytes bytes, row i of them at
 * row_offsets[i] .. row_offsets[i + 1] (HOST [n_rows + 1], nullable; entries 0 .. *rows_done are written).  A caller streams a
 * file in chunks of whole rows by calling again with row0 + *rows_done.  One call attempts as many rows as fit when every
 * field takes its 22 bytes (at least one row), so it may stop before the capacity is used up.
 * cells, labels and label_off are HOST arrays.  label_off [n_rows + 1] (nullable: no labels, and then labels must be null):
 * the label of file row row0 + i is labels[label_off[i] .. label_off[i + 1]), written as it is (the caller quotes);
 * label_off[0] = 0.  An empty label is still followed by the separator.  sep: a C string of exactly one byte.
 * ICNV_ERR_ARG before any launch: a null x, cells, sep, out, rows_done or n_bytes; G or C outside 1 .. 2^31 - 1; ld < G; an
 *   unknown orientation; n_cells outside 1 .. 2^31 - 1; a list entry outside 0 .. C - 1; an empty row range or one that leaves
 *   the table; sep not one byte; label offsets that do not start at 0 or descend, or come without label bytes (or bytes
 *   without offsets); a capacity below the shortest row possible (label, separator, one-byte fields).  A capacity below
 *   the actual first row is ICNV_ERR_ARG too, found after the lengths pass.  ICNV_ERR_UNSUPPORTED: a chunk of more than
 *   2^31 - 1 elements.  On an error *rows_done, *n_bytes and row_offsets are left as they were; `out` is written only by
 *   a call that succeeds.  The call synchronises the stream.
 * Method: a digits pass computes D = round(|x| 10^(14 - E)) in integer arithmetic from a 128-bit power-of-ten table and
 *   certifies the rounding; the elements it cannot certify -- every exact tie among them -- are formatted on the host with
 *   snprintf("%.14e") and their records replaced before any length is used.  A lengths pass sums the bytes of 256-field
 *   segments and of rows; the rows' offsets are scanned on the host.  An emit pass assembles each segment in LDS and stores
 *   it in aligned 16-byte words.  Timer names: "table_text_digits", "table_text_collect", "table_text_lengths",
 *   "table_text_emit". */
#define ICNV_TABLE_GENE_ROWS 0
#define ICNV_TABLE_CELL_ROWS 1
int icnv_format_table_dev(const double *x, int64_t ld, int64_t G, int64_t C, int32_t orientation, int64_t row0, int64_t n_rows,
                          const int32_t *cells, int64_t n_cells, const uint8_t *labels, const int64_t *label_off, const char *sep,
                          uint8_t *out, int64_t capacity, int64_t *row_offsets, int64_t *rows_done, int64_t *n_bytes, void *stream);
int icnv_format_table(const double *x, int64_t G, int64_t C, int32_t orientation, int64_t row0, int64_t n_rows, const int32_t *cells,
                      int64_t n_cells, const uint8_t *labels, const int64_t *label_off, const char *sep, uint8_t *out, int64_t capacity,
                      int64_t *row_offsets, int64_t *rows_done, int64_t *n_bytes);
/* Counters since the last reset, n = int64 slots (<= 7 written); a refused call counts nowhere:
 *   out[0] calls   out[1] rows written   out[2] elements that went through the digits pass   out[3] elements formatted on the host
 *   out[4] bytes written   out[5] extra collection rounds (more than 65536 flagged elements at once)   out[6] wall microseconds */
int icnv_table_text_stats(int64_t *out, int32_t n);
void icnv_table_text_stats_reset(void);

/* ---- count matrices from text (K21) -----------------------------------------------------------------------------------------
 * The inverse of the entries above: a chunk of a text table, as read.table(sep = <one byte>, header = TRUE, row.names = 1)
 * takes it in CreateInfercnvObject (R/inferCNV.R:146-156), becomes doubles in the library's layout.  DESIGN.md section 4 K21,
 * restated in tests/create_object_restate.py.  Not bound in the R shim.  Agreement with the bits of R's own R_strtod, which
 * works in long double, is believed for short decimals and not verified; the values here are C's strtod, bit for bit.
 *
 * The chunk: n_bytes (1 .. 2^31 - 2) of text that consists of whole lines, without the file's header line (the caller reads
 * that).  text_dev is the DEVICE copy (16-byte aligned), text_host the HOST copy of the same bytes; the host flavour takes one.
 * text_host may be NULL (K30: the chunk is a piece of a file that was inflated on the device): the library then fetches the
 * chunk from text_dev itself, once, and only if a field the device pass does not certify or a refusal asks for it; the label
 * ranges it returns then still include a label's enclosing quotes (the caller slices the labels it fetches).  The same holds
 * for icnv_parse_table_cols_dev.
 * Grammar -- everything else is refused, nothing is quietly misparsed:
 *   lines     end in "\n" or "\r\n"; the last line may lack the terminator.  A line that is empty (or a lone "\r") is skipped.
 *   row       a label and n_cols numeric fields, separated by the one byte of `sep` (not a line end, not a quote).
 *   label     the row's first field, opaque bytes up to the first separator; it may be enclosed in a pair of `"`, which the
 *             reported range leaves out.  A quote anywhere else in a label is refused, and a separator inside a quoted label
 *             is a separator (so such a row is refused for its field count or for the field that follows).
 *   number    [+-] (digits [. [digits]] | . digits) [(e|E) [+-] digits], or NaN, Inf, +Inf, -Inf, or NA or the empty field.
 *             NA and the empty field give R's NA_real_ (bits 0x7FF00000000007A2, as K19 stores it), NaN gives
 *             0x7FF8000000000000.  Hex floats, quoted numbers, blanks around a number and other spellings are refused.
 * Value: every number becomes the correctly rounded double (ties to even), what strtod returns.
 * Output: row i (counting the chunk's rows that are not blank), column c goes to out[c * ld + row0 + i] -- DEVICE in the _dev
 *   flavour, HOST otherwise --, the (cells, genes) matrix of every *_dev entry when the file has a line per gene.
 *   label_ranges (HOST, [2 * max_rows]): the label of row i is the chunk's bytes label_ranges[2 i] .. label_ranges[2 i + 1].
 *   *n_rows: the rows found (0 for a chunk of blank lines).
 * ICNV_ERR_ARG before any launch: a null pointer; n_bytes out of range; a device text that is not 16-byte aligned; a bad sep;
 *   n_cols outside 1 .. 2^31 - 1; line0 < 1; row0 < 0, max_rows < 1 or row0 + max_rows > ld.  ICNV_ERR_ARG after the passes:
 *   more rows than max_rows, or a refusal, whose message reads "parse_table: line L, field K: <what>: '<bytes>'" with L the
 *   1-based file line (line0 is the file line of the chunk's first line, blank lines count), K the 1-based field of that line
 *   (the label is field 1; for a row with a field count other than n_cols + 1: the count).  Of several refusals the one at the
 *   smallest byte offset is reported (a ragged row counts at its first byte; among more than 65536 uncertified fields only
 *   those of the first round are looked at).  On any error out, label_ranges and *n_rows are
 *   left as they were: the values are staged and reach `out` only when every field of the chunk is known.  Synchronises.
 * Method: a structure pass marks row and field starts, 16 positions per lane, counts them per 4096-byte segment and scans the
 *   counts; an index pass lists the starts; a rows pass checks field counts and labels; a parse pass runs one lane per field:
 *   at most 19 significant digits with a significand below 2^53 and a decimal exponent within +-22 take one exact multiply or
 *   divide, other fields of at most 19 digits a product with a 128-bit power of ten (csrc/tp_pow10_table.h, exponents -342 ..
 *   308) that is stored only when its rounding is certified (csrc/table_parse_num.h).  Everything else -- exact ties, more
 *   than 19 digits, fields longer than 40 bytes, subnormal results, underflow, overflow -- is parsed here with strtod from
 *   text_host and patched in.  A transpose pass moves the staged values to `out` through 64 x 64 LDS tiles.
 *   Timer names: "table_parse_structure", "table_parse_index", "table_parse_fields", "table_parse_collect",
 *   "table_parse_transpose". */
int icnv_parse_table_dev(const uint8_t *text_dev, const uint8_t *text_host, int64_t n_bytes, const char *sep, int64_t n_cols,
                         int64_t line0, double *out, int64_t ld, int64_t row0, int64_t max_rows, int64_t *label_ranges, int64_t *n_rows,
                         void *stream);
int icnv_parse_table(const uint8_t *text, int64_t n_bytes, const char *sep, int64_t n_cols, int64_t line0, double *out, int64_t ld,
                     int64_t row0, int64_t max_rows, int64_t *label_ranges, int64_t *n_rows);
/* Counters since the last reset, n = int64 slots (<= 7 written); a refused call counts nowhere:
 *   out[0] calls   out[1] rows   out[2] numeric fields   out[3] fields parsed on the host   out[4] bytes
 *   out[5] extra collection rounds (more than 65536 uncertified fields at once)   out[6] wall microseconds */
int icnv_table_parse_stats(int64_t *out, int32_t n);
void icnv_table_parse_stats_reset(void);
/* The last step of CreateInfercnvObject: out[j * ld_out + i] = in[cells[j] * ld_in + genes[i]] for a (C_in, G_in) DEVICE matrix
 * whose rows lie ld_in apart; genes / cells are HOST lists, 0-based, in any order (null: all of them, in order, and the
 * count is ignored).  `out` must not overlap `in`.  ICNV_ERR_ARG: a null matrix, dimensions outside 1 .. 2^31 - 1, ld_in < G_in,
 * ld_out < n_genes, an empty list or an entry that is not a gene / cell.  Synchronises.  Timer name: "gather_matrix". */
int icnv_gather_matrix_dev(const double *in, int64_t ld_in, int64_t G_in, int64_t C_in, const int32_t *genes, int64_t n_genes,
                           const int32_t *cells, int64_t n_cells, double *out, int64_t ld_out, void *stream);

/* ---- exact sum of a matrix (K23) -----------------------------------------------------------------------------------------------
 * mean(infercnv_obj@expr.data), the first line of plot_per_group (R/infercnv_sampling.R:522) and plot_cnv's default x.center:
 * the sum of the G * C values of a (C, G) matrix whose rows lie ld >= G apart (the padding is never read), as the exact real sum
 * rounded to double once, to nearest with ties to even.  That is Python's math.fsum wherever math.fsum returns, and the same
 * rule where it raises "intermediate overflow".  Any NaN gives NaN; +Inf and -Inf together give NaN; infinities of one sign give
 * that infinity; a finite exact sum beyond the double range gives +-Inf; a zero sum is +0.0.  The result is the same on every
 * run and for every launch shape.  DESIGN.md section 4 K23, restated in tests/sampling_restate.py.
 * Method: every finite double is a multiple of 2^-1074; the kernel adds the significands into a fixed-point number of 68 digits
 *   of 32 bits held in 64-bit limbs (a lane's window of four limbs in registers, a wave's limbs in LDS, one record per
 *   workgroup), and the host adds the records, propagates the carry once and rounds.
 * icnv_matrix_sum_dev: x is a DEVICE matrix; synchronises the stream and writes the sum into the HOST double *sum.
 * icnv_matrix_sum: the same for a HOST matrix (recognised when resident, else uploaded).
 * ICNV_ERR_ARG before any launch: a null matrix or result, dimensions outside 1 .. 2^31 - 1, ld < G.  Timer name: "matrix_sum". */
int icnv_matrix_sum_dev(const double *x, int64_t ld, int64_t G, int64_t C, double *sum, void *stream);
int icnv_matrix_sum(const double *x, int64_t ld, int64_t G, int64_t C, double *sum);

/* ---- sparse count matrices (K22) ----------------------------------------------------------------------------------------------
 * The count matrix as it arrives at production size -- a MatrixMarket coordinate file (10x: matrix.mtx) or a sparse matrix in
 * memory -- becomes an icnv_counts in CSC form on the device and stays sparse through .order_reduce and the cell filter of
 * CreateInfercnvObject (R/inferCNV.R:133-337 keeps a dgCMatrix sparse likewise).  DESIGN.md section 4 K22, restated in
 * tests/sparse_counts_restate.py.  Device entries only; not bound in the R shim.  The triplet grammar is the MatrixMarket
 * specification's; there is no R here, so no byte of Matrix::writeMM or Seurat::Read10X was compared: scipy's reader is the
 * independent check.  All arithmetic is integer; every result is the same on every run and for every launch shape.
 *
 * icnv_parse_triplets_dev: a chunk of the BODY of a coordinate file (the caller reads the banner, the % comments and the size
 * line) to three int32 arrays.  text_dev is the DEVICE copy (16-byte aligned), text_host the HOST copy of the same n_bytes
 * (1 .. 2^31 - 2) of whole lines; the host copy is read only to word a refusal.
 * text_host may be NULL: a refused chunk is then fetched from text_dev for that wording (icnv_parse_triplets_cols_dev too).
 * Grammar -- everything else is refused, nothing is quietly misparsed:
 *   lines     end in "\n" or "\r\n"; the last line may lack the terminator.  A line that is empty, a lone "\r" or only blanks
 *             (space, tab) is skipped.  Every other line is an entry; the k-th of the chunk goes to slot k of the arrays.
 *   entry     `i j v`, with field = ICNV_MM_PATTERN `i j` and v = 1.  The fields are separated by one or more blanks; blanks
 *             before the first and after the last field are allowed.  Another number of fields is refused, and so is a line
 *             whose first field begins with `%`.
 *   i, j      plain unsigned decimals of at most 10 digits, 1-based, in 1 .. n_rows and 1 .. n_cols; stored 0-based.  A sign,
 *             another byte or a value outside the range is refused.
 *   v         (ICNV_MM_INTEGER and ICNV_MM_REAL alike) a field of at most 40 bytes in the number grammar of "count matrices from
 *             text" above, accepted when the double nearest to it is an integer in 0 .. 2^31 - 1: 3, +3, 3.0, 3e0 and
 *             3.000000000000000e+00 are 3, and an explicit 0 is kept as a stored zero.  A field whose exact value is such an
 *             integer is taken by integer arithmetic, whatever its spelling; any other field is converted as there
 *             (csrc/table_parse_num.h), so 2147483646.999999999 is 2147483647.  Refused: a negative value (-0 included), a
 *             fraction, 2147483648 and above, NA, the empty field, NaN, Inf, more than 19 significant digits, and a field
 *             that is no integer and whose rounding cannot be certified (an underflow; no such field of at most 19 digits
 *             rounds to an integer).  No host fallback.
 * Output: row_dev / col_dev / val_dev (DEVICE, `capacity` elements each) receive the entries in file order; *n_entries (HOST)
 *   their number (0 for a chunk of blank lines).
 * ICNV_ERR_ARG before any launch: a null pointer; n_bytes out of range; a device text that is not 16-byte aligned; an unknown
 *   field; n_rows or n_cols outside 1 .. 2^31 - 1; line0 < 1; capacity < 0.  ICNV_ERR_ARG after the passes: more entries than
 *   capacity (nothing is written past the end), or a refusal, whose message reads
 *   "parse_triplets: line L, field K: <what>: '<bytes>'" with L the 1-based file line (line0 is the file line of the chunk's
 *   first line; blank lines count), K the 1-based field and <bytes> at most 60 bytes of it.  A wrong number of fields and a
 *   comment line are reported at the line's first byte with the line's bytes, K being the number of fields (1 for a comment).
 *   Of several refusals the one at the smallest byte offset is reported.  On any error the three arrays and *n_entries are
 *   left as they were: the entries are staged and copied only when the whole chunk is known.  Synchronises.
 * Method: a structure pass marks the first byte of every line that is not blank, 16 positions per lane, counts them per
 *   4096-byte segment and scans the counts; an index pass lists them; a parse pass runs one lane per entry.  The one atomic is
 *   the 64-bit atomicMin on the error word.  A line that begins with a blank is walked to its first other byte by the lane
 *   that owns its first byte.  Timer names: "triplets_structure", "triplets_index", "triplets_parse". */
#define ICNV_MM_INTEGER 0
#define ICNV_MM_REAL 1
#define ICNV_MM_PATTERN 2
int icnv_parse_triplets_dev(const uint8_t *text_dev, const uint8_t *text_host, int64_t n_bytes, int32_t field, int64_t n_rows,
                            int64_t n_cols, int64_t line0, int32_t *row_dev, int32_t *col_dev, int32_t *val_dev, int64_t capacity,
                            int64_t *n_entries, void *stream);
/* The column pointers of triplets that are sorted: row_dev / col_dev [nnz] (DEVICE, 0-based, nnz >= 0) must have strictly
 * ascending 64-bit keys col * G + row -- column-major order, what 10x, Matrix::writeMM and scipy.io.mmwrite of a CSC matrix
 * write (believed of the first two, not verified here).  Then row and the values ARE the CSC's rowidx and vals, without a copy,
 * and colptr_dev [C + 1] (DEVICE, int64) is written by boundary detection: entry k stores k into
 * colptr[col[k - 1] + 1 .. col[k]] (col[-1] = -1), the last entry also nnz into colptr[col + 1 .. C].  No histogram and no
 * atomics; empty columns at the start, in the middle and at the end come out right.  nnz = 0 gives the all-zero colptr without
 * a launch.
 *   *first_violation (HOST)  the smallest k with key[k] <= key[k - 1], or -1
 *   *violation_kind (HOST)   ICNV_CSC_SORTED; ICNV_CSC_DUPLICATE: the keys of k - 1 and k are equal, a (gene, cell) pair stored
 *                            twice -- an error for the caller, since icnv_counts does not detect duplicates downstream;
 *                            ICNV_CSC_DESCENT: unsorted input, to be sorted by the caller and handed in again.
 * With a violation the call returns ICNV_OK and colptr_dev is left untouched.  ICNV_ERR_ARG: a null pointer, G or C outside
 * 1 .. 2^31 - 1, nnz < 0, an entry whose row or column lies outside the matrix (checked on the device before anything else;
 * colptr_dev untouched).  Synchronises.  Timer names: "csc_build_check", "csc_build_colptr". */
#define ICNV_CSC_SORTED 0
#define ICNV_CSC_DUPLICATE 1
#define ICNV_CSC_DESCENT 2
int icnv_csc_from_sorted_triplets_dev(const int32_t *row_dev, const int32_t *col_dev, int64_t nnz, int64_t G, int64_t C,
                                      int64_t *colptr_dev, int64_t *first_violation, int32_t *violation_kind, void *stream);
/* .order_reduce (R/inferCNV.R:352-428) and the cell filter (:236-288) on a CSC matrix: cnt (CSC form, DEVICE pointers, G x C),
 * gene_map_dev [G] the new row of each gene or -1 to drop it, cells_dev [n_cells] the source columns, in any order, repeats
 * allowed.  Output column j holds the entries of source column cells[j] whose gene is kept, IN SOURCE ORDER, with the rows
 * mapped -- a stable compaction, so the rows of an output column are in whatever order gene_map leaves them, which icnv_counts
 * allows ("any order inside a column").  Values are copied, stored zeros included.
 * Two calls: with rowidx_out == NULL the call fills colptr_out [n_cells + 1] (DEVICE, int64: the exclusive scan of the kept
 * entries per output column) and *nnz_out (HOST); with rowidx_out / vals_out (DEVICE, `capacity` elements each) it fills
 * those as well.  Neither call keeps state: the second counts again.
 * ICNV_ERR_ARG: a null pointer; a dense icnv_counts; G, C or n_cells outside 1 .. 2^31 - 1; n_genes_out outside 0 .. 2^31 - 1;
 * an entry of cells outside 0 .. C - 1 or of gene_map outside -1 .. n_genes_out - 1 (checked on the device before anything is
 * counted; the message names the first such entry); capacity smaller than the count.  On an error the outputs are untouched.
 * A colptr of cnt that leaves 0 .. nnz, or a row index outside 0 .. G - 1, reads nothing out of bounds: such a range is
 * clipped and such an entry dropped.  Synchronises.
 * Method: one wavefront per output column walks the source column 64 entries at a time -- first counting the kept ones by
 * ballot, then, after a two-level exclusive int64 scan of the counts (tiles of 2048 columns, their sums scanned by one
 * workgroup; exact for every n_cells), storing lane l's entry behind those of the kept lanes below it.
 * Timer names: "csc_select_count", "csc_select_fill". */
int icnv_csc_select_dev(const icnv_counts *cnt, int64_t G, int64_t C, const int32_t *gene_map_dev, int64_t n_genes_out,
                        const int32_t *cells_dev, int64_t n_cells, int64_t *colptr_out, int32_t *rowidx_out, int32_t *vals_out,
                        int64_t capacity, int64_t *nnz_out, void *stream);

/* ---- reading a selection of columns (K26) -------------------------------------------------------------------------------------
 * The two chunk parsers above for a caller that wants some of the file's columns only: a rank of the cell-sharded route that
 * reads its own cells, or an annotation file that names a subset.  DESIGN.md section 4 K26, restated in
 * tests/read_select_restate.py.  Device entries only; not bound in the R shim.
 *
 * The column map, in both entries: col_map_dev [n_cols] (DEVICE, int32) gives the output column of every numeric file column
 * (dense) or matrix column (triplets), or -1 to skip it; n_cols_out is 1 .. n_cols.  The map is checked on the device before
 * any other pass: every entry must lie in -1 .. n_cols_out - 1 and every output column must be hit exactly once.  Otherwise
 * the call returns ICNV_ERR_ARG and the message names the first offending entry: the first entry out of range; else the first
 * entry that names an output column a second time; else the first output column that no entry hits.  Timer name:
 * "col_map_check".
 *
 * icnv_parse_table_cols_dev: icnv_parse_table_dev with the map.  Row i of the chunk, file column c with col_map[c] = k >= 0
 * goes to out[k * ld + row0 + i]; `out` has n_cols_out columns.  n_cols stays the FILE's column count.
 *   What sees the whole chunk: the structure pass, the rows' starts and the rows' checks.  A ragged row (counted against
 *   n_cols + 1), a bad label or a bad separator is refused exactly as icnv_parse_table_dev refuses it, with the same message,
 *   line and field number, whatever is selected.
 *   What sees the selected columns only: everything else.  FIELDS OF SKIPPED COLUMNS ARE NOT EXAMINED: no lane converts them,
 *   they never reach the host's strtod, they do not count in icnv_table_parse_stats slots 2 and 3 (slot 2 grows by rows *
 *   n_cols_out), and a byte outside the number grammar in a skipped column is NOT reported by this call.  Over a deal in which
 *   every column has exactly one owner, every field of the file is still examined once.
 *   A refusal in a selected column reads exactly as the plain entry's: the file's line and the file's field number (not the
 *   output column), under the prefix "parse_table: ".
 *   The staged positions and values, the uncertified-field rounds and the transpose are n_cols_out wide: no device allocation
 *   of the call grows with n_cols * rows (there is no list of all field starts; the per-segment counts grow with the bytes
 *   / 4096, the rows' arrays with the rows, the map's inverse with n_cols_out).
 *   Every other rule is icnv_parse_table_dev's: the grammar, the values (strtod, bit for bit), label_ranges, *n_rows, the
 *   ICNV_ERR_ARG cases before any launch, and on any error out, label_ranges and *n_rows are left as they were.  The identity
 *   map gives icnv_parse_table_dev's output bit for bit.  Synchronises.
 *   Timer names: "table_parse_structure", "table_cols_index" (rows' starts, selected field starts), "table_cols_rows" (the
 *   rows' checks), "table_cols_fields", "table_cols_collect", "table_parse_transpose". */
int icnv_parse_table_cols_dev(const uint8_t *text_dev, const uint8_t *text_host, int64_t n_bytes, const char *sep, int64_t n_cols,
                              int64_t line0, double *out, int64_t ld, int64_t row0, int64_t max_rows, int64_t *label_ranges,
                              int64_t *n_rows, const int32_t *col_map_dev, int64_t n_cols_out, void *stream);
/* icnv_parse_triplets_cols_dev: icnv_parse_triplets_dev with the map.  EVERY entry of the chunk is parsed and validated in
 * full, as there: its fields have to be read to learn its column, the value grammar is integer-only and there is no host
 * fallback -- so a refusal anywhere, in a skipped column too, reads the same on every rank ("parse_triplets: line L, field
 * K: ...").  Then the entries whose column maps to -1 are dropped and the kept ones are stored in FILE ORDER -- a stable
 * compaction -- with the column replaced by col_map[col].
 *   *n_entries (HOST)  the kept entries;  *n_seen (HOST)  the entries of the chunk (what icnv_parse_triplets_dev counts).
 *   capacity bounds the KEPT entries: with more, ICNV_ERR_ARG "parse_triplets_cols: N entries are kept, capacity is M" and
 *   nothing is written (the caller may grow its arrays to N and call again).  An output column need not receive an entry.
 *   On any error the three arrays, *n_entries and *n_seen are left as they were.  Synchronises.
 * Method: K22's structure, index and parse passes into staged arrays; then the kept entries of every tile of 2048 staged
 *   entries are counted by ballot, the counts scanned by one workgroup, and entry k is stored behind the kept entries of the
 *   tiles before its tile and of the steps, wavefronts and lanes before it inside the tile.  No atomics besides K22's error word; the result does not depend on the launch
 *   shape.  Timer names: "triplets_structure", "triplets_index", "triplets_parse", "triplets_keep_count", "triplets_keep_fill". */
int icnv_parse_triplets_cols_dev(const uint8_t *text_dev, const uint8_t *text_host, int64_t n_bytes, int32_t field, int64_t n_rows,
                                 int64_t n_cols, int64_t line0, int32_t *row_dev, int32_t *col_dev, int32_t *val_dev, int64_t capacity,
                                 int64_t *n_entries, const int32_t *col_map_dev, int64_t n_cols_out, int64_t *n_seen, void *stream);

/* ---- CNV region reports (K24) -----------------------------------------------------------------------------------------------
 * The bodies of `<prefix>.pred_cnv_genes.dat` and `<prefix>.pred_cnv_regions.dat`, which generate_cnv_region_reports writes
 * with write.table(quote = FALSE, sep = "\t") (R/inferCNV_HMM.R:790-869).  The byte-level yardstick is the host writer kept in
 * infercnv_amd/cnv_regions.py; DESIGN.md section 4 K24, restated in tests/cnv_reports_restate.py.  The header lines stay with
 * the caller.  Not yet bound in the R shim.
 *
 * A plan describes one file.  icnv_cnv_report_begin[_dev] takes
 *   records    the six int32 arrays of icnv_cnv_runs_dev, records[f * capacity + r] for r < n_records: f = 0 list position,
 *              1 chromosome index, 2 first gene, 3 last gene (inclusive), 4 state, 5 ordinal.  They are already filtered by
 *              `neutral` and ordered by (list position, gene).  DEVICE in the _dev flavour, where the plan keeps the pointer:
 *              the arrays stay valid and unchanged until icnv_cnv_report_end.  HOST otherwise (the plan uploads a copy).
 *   three string tables, HOST, each as bytes plus int64 offsets [n + 1] (entry i is bytes[off[i] .. off[i + 1]), copied as
 *              bytes; bytes may be null when every entry is empty): the cell-group names by list position, the chromosome names
 *              by chromosome index, the gene names in the gathered gene order of chr_layout() -- the order the records count in.
 *   gene_start, gene_end   HOST int64 [G], in the same gathered order.
 *   totals     HOST, nullable, 3 entries: bytes of the whole body, lines of the whole body, bytes of the largest record.
 * begin uploads the tables once, computes the byte offset of every record and keeps it on both sides; it synchronises.
 * n_records = 0 gives a valid plan of an empty body.  icnv_cnv_report_end frees the plan (null is fine).
 *
 * ICNV_REPORT_GENES: one line for every gene g in gene_first .. gene_last of every record, in record order, then gene order:
 *   <group>\t<chr>-region_<ordinal>\t<state>\t<gene name g>\t<chr>\t<start[g]>\t<end[g]>\n
 * ICNV_REPORT_REGIONS: one line per record:
 *   <group>\t<chr>-region_<ordinal>\t<state>\t<chr>\t<min start over the run>\t<max end over the run>\n
 * Integers are plain decimal, `-` in front of a negative one, no padding.  State 255 -- the library's invalid state -- is
 * written as -1, every other state byte as its decimal value.  There is no limit on the length of a name or of a line.
 *
 * icnv_cnv_report_format[_dev] formats the records rec0 .. into `out` (capacity bytes; DEVICE in the _dev flavour, any
 * alignment) and stops before the first record that does not fit: *recs_done records (>= 1) take *n_bytes bytes, record
 * rec0 + i of them at rec_offsets[i] .. rec_offsets[i + 1] (HOST, nullable, room for n_records - rec0 + 1 entries; entries
 * 0 .. *recs_done are written).  A caller streams a file in chunks of whole records by calling again with rec0 + *recs_done.
 * Offsets within the file are int64 throughout.
 * ICNV_ERR_ARG, before any launch: a null plan pointer, records, offsets, positions, out, recs_done or n_bytes; an unknown
 *   kind; capacity (of the records) < n_records; a table of no entry; offsets that do not start at 0 or descend, or bytes
 *   missing for them; a record whose list position, chromosome or gene range leaves its table, with gene_first > gene_last,
 *   or with a state outside 0 .. 255 (the device records are copied to the host for this check); rec0 outside
 *   0 .. n_records - 1; a capacity below the first record.  ICNV_ERR_UNSUPPORTED: a capacity above 2^31 - 1.
 *   On an error the outputs are left as they were; `out` is written only by a call that succeeds, and never outside
 *   out[0 .. *n_bytes).  The calls synchronise the stream.
 * Method: no pass over the lines.  P = int64 prefix sum over the genes of len(name) + digits(start) + digits(end); the fixed
 *   part of a record's lines is F = len(group) + 2 len(chr) + 8 + digits(ordinal) + len(state text) + 7; a GENES record of n
 *   genes takes n F + P[last + 1] - P[first] bytes and its line i starts at i F + P[first + i] - P[first]; a REGIONS record
 *   takes F - 1 + digits(min) + digits(max) after a min / max reduction over its genes.  One scan gives the record offsets.
 *   The emit pass gives each workgroup 16 KiB of the output: it finds the lines that overlap them from the offsets, assembles
 *   the bytes in LDS and stores aligned 16-byte words (the ragged ends of the chunk byte by byte).
 *   Timer names: "cnv_report_prefix", "cnv_report_lengths", "cnv_report_scan", "cnv_report_emit". */
#define ICNV_REPORT_GENES 0
#define ICNV_REPORT_REGIONS 1
typedef struct icnv_cnv_report icnv_cnv_report_t;
int icnv_cnv_report_begin_dev(icnv_cnv_report_t **plan, int32_t kind, const int32_t *records, int64_t capacity, int64_t n_records,
                              const uint8_t *group_bytes, const int64_t *group_off, int64_t n_groups, const uint8_t *chr_bytes,
                              const int64_t *chr_off, int64_t n_chr, const uint8_t *gene_bytes, const int64_t *gene_off,
                              const int64_t *gene_start, const int64_t *gene_end, int64_t G, int64_t *totals, void *stream);
int icnv_cnv_report_begin(icnv_cnv_report_t **plan, int32_t kind, const int32_t *records, int64_t capacity, int64_t n_records,
                          const uint8_t *group_bytes, const int64_t *group_off, int64_t n_groups, const uint8_t *chr_bytes,
                          const int64_t *chr_off, int64_t n_chr, const uint8_t *gene_bytes, const int64_t *gene_off,
                          const int64_t *gene_start, const int64_t *gene_end, int64_t G, int64_t *totals);
int icnv_cnv_report_format_dev(icnv_cnv_report_t *plan, int64_t rec0, uint8_t *out, int64_t capacity, int64_t *rec_offsets,
                               int64_t *recs_done, int64_t *n_bytes, void *stream);
int icnv_cnv_report_format(icnv_cnv_report_t *plan, int64_t rec0, uint8_t *out, int64_t capacity, int64_t *rec_offsets, int64_t *recs_done,
                           int64_t *n_bytes);
void icnv_cnv_report_end(icnv_cnv_report_t *plan);
/* Counters since the last reset, n = int64 slots (<= 5 written); a refused call counts nowhere:
 *   out[0] format calls   out[1] records written   out[2] lines written   out[3] bytes written   out[4] wall microseconds */
int icnv_cnv_report_stats(int64_t *out, int32_t n);
void icnv_cnv_report_stats_reset(void);

/* ---- R's XDR stream of a matrix (K27) ------------------------------------------------------------------------------------------
 * saveRDS writes a numeric or integer vector as its elements in order, each big-endian (XDR); a matrix is the vector of its
 * columns, so element (r, c) of a rows x cols matrix is element e = c * rows + r of the stream.  The rest of the format -- the
 * header, the flag words, attributes, strings -- is written on the host and is set down in infercnv_amd/rds.py.
 *
 * icnv_xdr_encode_dev writes the elements [e0, e1) of that stream to dst (DEVICE, (e1 - e0) * elem_size bytes: element e at
 * dst + (e - e0) * elem_size), every element's bytes reversed.  elem_size is 8 (REALSXP) or 4 (INTSXP, LGLSXP).
 *   ICNV_XDR_COLS  src is (cols, rows) with contiguous rows, ld >= rows elements apart: the device-resident (cells, genes)
 *                  matrix, already in R's order.  A coalesced swap; 16-byte loads and stores where the segment is contiguous
 *                  in src and src's first element and dst share their position in a 16-byte word.
 *   ICNV_XDR_ROWS  src is (rows, cols) with contiguous rows, ld >= cols: an uploaded host expr_data.  A 64 x 64 tile transpose
 *                  through LDS (rows padded by one element: no bank conflicts on either side) plus the swap.
 * A vector is rows = n, cols = 1 (ICNV_XDR_COLS).  e0 and e1 need not fall on tile, row or column boundaries: a stream is cut
 * into chunks by bytes.  e0 == e1 is a valid empty call.
 * icnv_xdr_decode_dev is the inverse: src is the stream segment (DEVICE, element e at src + (e - e0) * elem_size), dst the
 * matrix in either layout; only the elements of the segment are written.
 * Index arithmetic is 64-bit throughout.  No floating-point operation touches the data: a NaN keeps its payload, NA_real_
 * (0x7FF00000000007A2) among them.  The calls do not synchronise.
 * ICNV_ERR_ARG before any launch: a null pointer; elem_size other than 8 or 4; an unknown layout; rows or cols < 1 or
 *   rows * cols > 2^59; ld below the row length; e0 < 0, e0 > e1 or e1 > rows * cols; a pointer not aligned to elem_size.
 * ICNV_ERR_UNSUPPORTED: an ICNV_XDR_ROWS segment of more than 2^31 - 1 tiles.
 * Timer names: "xdr_encode", "xdr_decode". */
#define ICNV_XDR_COLS 0
#define ICNV_XDR_ROWS 1
int icnv_xdr_encode_dev(const void *src, int32_t elem_size, int64_t rows, int64_t cols, int64_t ld, int32_t layout, int64_t e0,
                        int64_t e1, void *dst, void *stream);
int icnv_xdr_decode_dev(const void *src, int32_t elem_size, int64_t rows, int64_t cols, int64_t ld, int32_t layout, int64_t e0,
                        int64_t e1, void *dst, void *stream);

/* ---- DEFLATE in independent pieces (K28) ------------------------------------------------------------------------------------------
 * A payload-agnostic compressor: bytes on the device in, DEFLATE (RFC 1951) out.  The input is cut into pieces of piece_bytes
 * (the last one shorter); piece i compresses src[i * piece_bytes, min(n, (i + 1) * piece_bytes)) on its own, one workgroup per
 * piece, and lands at dst + i * dst_stride.  saveRDS's gzip stream is assembled from such pieces in infercnv_amd/rds.py.
 *   a piece     a sequence of complete DEFLATE blocks: no block has BFINAL set; no match distance reaches before the piece's
 *               first byte; the piece ends on a byte boundary (after a Huffman-coded block the empty stored block of zlib's
 *               Z_SYNC_FLUSH follows: 000, pad, 00 00 FF FF).  A raw inflater started fresh on a piece returns the piece's
 *               input and accepts the next piece, or a final empty block, directly behind it.
 *   its form    whichever is smaller: one stored block (5 bytes of header), or one dynamic-Huffman block (BTYPE 10) over LZ77
 *               tokens -- matches of 3..258 bytes at distance 8, distance 1 or to the latest earlier position with the same
 *               4-byte hash; code lengths <= 15 (literal/length, distance) and <= 7 (code-length alphabet), the length sequence
 *               run-length coded with 16, 17, 18.  A length limit that cannot be met stores the piece.  No fixed-Huffman block.
 *   piece_len   DEVICE int32 [pieces]: the bytes of piece i, 6 <= piece_len[i] <= icnv_deflate_bound(piece_bytes).
 *   piece_crc   DEVICE uint32 [pieces]: the CRC-32 of piece i's INPUT (zlib's: reflected 0xEDB88320, initial value and final xor
 *               0xFFFFFFFF); the stream's CRC follows by crc32_combine without a pass over the payload.
 *   bound       icnv_deflate_bound(piece_bytes) = piece_bytes + 5 * ceil(piece_bytes / 65535), or -1 outside the allowed range.
 *               No store lands outside [dst + i * dst_stride, + bound): every store's offset is tested against it.
 *   range       256 <= piece_bytes <= 16384 (the piece, its match records and its hash table live in 77 KiB of LDS).
 * The output is a function of src's bytes, n and piece_bytes only: every atomic is an integer max, sum, or or xor in LDS, no
 * workgroup looks at another, and the geometry is fixed.  src needs no alignment (4-byte aligned pieces are loaded as dwords).
 * n == 0 is a valid empty call.  The call does not synchronise.
 * icnv_deflate_pack_dev: the lengths pass plus emit pass of K20 / K24 -- a prefix sum of piece_len (each clamped to
 * [0, dst_stride]), then a copy of every piece behind the one before into out (DEVICE, out_cap bytes).  *out_len (HOST) is
 * the packed size.  The call WAITS on `stream` twice: for the size, ahead of the copy, and at its end.
 * ICNV_ERR_ARG before any launch: n < 0; piece_bytes outside the range; dst_stride below the bound; a null pointer with work
 *   to do; piece_len / piece_crc not 4-byte aligned; more than 2^31 - 1 pieces.  icnv_deflate_pack_dev: the same kind, and,
 *   after the lengths pass and before the copy, out_cap below the packed size -- nothing is written to out then.
 * Timer names: "deflate_pieces", "deflate_pack". */
int64_t icnv_deflate_bound(int64_t piece_bytes);
int icnv_deflate_pieces_dev(const uint8_t *src, int64_t n, int64_t piece_bytes, uint8_t *dst, int64_t dst_stride, int32_t *piece_len,
                            uint32_t *piece_crc, void *stream);
int icnv_deflate_pack_dev(const uint8_t *dst, int64_t dst_stride, const int32_t *piece_len, int64_t n_pieces, uint8_t *out,
                          int64_t out_cap, int64_t *out_len /* HOST */, void *stream);

/* ---- INFLATE in independent units (K29) ---------------------------------------------------------------------------------------------
 * The way back from K28's files: a raw DEFLATE stream (RFC 1951) that was written with flush points is inflated unit by unit,
 * one wavefront per unit.  The stream carries no index of its units; the caller finds them with these four calls (the chain
 * walk between them is host work on a few numbers per unit: infercnv_amd/rds.py, inflate_gzip).
 *   candidate   an offset p of src with src[p - 4, p) = 00 00 FF FF: the byte behind a flush marker.  The caller adds the
 *               stream's first byte.  A marker pattern inside compressed or stored data is a false candidate: it costs one
 *               wasted measure and is never reached by the chain.
 *   unit        starts at a candidate, on a byte boundary: the run of complete DEFLATE blocks from there up to and including
 *               the first EMPTY stored block (LEN = 0: it ends the unit on a byte boundary behind a marker, so on a candidate)
 *               or a block with BFINAL set (the unit ends on the next byte boundary).  Stored (non-empty ones are copied and
 *               do not end the unit), fixed-Huffman and dynamic-Huffman blocks in any number.  A match reaches back anywhere
 *               inside its own unit, up to 32 768 bytes; one that reaches before the unit's first output byte is NEEDS_HISTORY.
 *   chain       the first unit ends where the second starts, and so on, up to the unit that ends with BFINAL.
 *   status      DEVICE int32 per unit:
 *     ICNV_INFLATE_OK_MARKER      ended by an empty stored block without BFINAL
 *     ICNV_INFLATE_OK_FINAL       ended by a block with BFINAL
 *     ICNV_INFLATE_TRUNCATED      ran into src + n
 *     ICNV_INFLATE_TOO_LONG       needed more than max_in compressed bytes (the measure only)
 *     ICNV_INFLATE_BAD_STREAM     BTYPE 11; stored LEN != ~NLEN; HLIT > 286 or HDIST > 30 symbols; an over-subscribed set of
 *                                 code lengths, or an incomplete one -- except, for the literal/length and the distance code,
 *                                 no code at all or one single code of length one (what zlib accepts); no code for symbol 256;
 *                                 a repeat code 16 with nothing before it; lengths running past HLIT + HDIST; bits that are no
 *                                 code; literal/length symbols 286 / 287; distance symbols 30 / 31; a distance code where the
 *                                 block defines none.  The decode: any disagreement with the caller's end / out_len, an end
 *                                 that comes too early included.
 *     ICNV_INFLATE_NEEDS_HISTORY  a distance beyond the bytes the unit has produced so far
 *               A malformed stream is an ordinary input: it ends in one of these, never in a fault.  Every load is tested
 *               against [src, src + n) and every store against the unit's own output range before it is issued; every loop
 *               takes at least one bit (a stored block: four bytes) of the unit's budget per round.
 * icnv_inflate_scan_dev      cand (DEVICE int64 [cand_cap]) receives the candidates in [4, n] in ascending order, *n_cand (HOST)
 *               their number.  Two passes (count, emit) compacted by ballot and prefix sums: no atomics.  The call WAITS on
 *               `stream` for the count; when it exceeds cand_cap the call returns ICNV_ERR_ARG with *n_cand set and nothing
 *               written to cand.
 * icnv_inflate_measure_dev   parses the unit at every start[i] (DEVICE int64) without producing bytes: end[i], the offset just
 *               behind the unit; out_len[i], the bytes it inflates to (both DEVICE int64; with a status other than OK_* they
 *               hold where the parse stood); status[i].  max_in: the most compressed bytes a unit may take.
 * icnv_inflate_units_dev     decodes unit i, src[start[i], end[i]), into out[out_off[i], out_off[i] + out_len[i]).  A unit
 *               whose decode does not end exactly at end[i] with exactly out_len[i] bytes gets BAD_STREAM; its output range
 *               holds unspecified bytes then, and nothing outside it was written.  Ranges of different units must not overlap
 *               (not checked: the stores stay inside each unit's own range either way).
 * icnv_crc32_pieces_dev      crc[i] (DEVICE uint32 [ceil(n / piece_bytes)]) = the CRC-32 (zlib's) of
 *               src[i * piece_bytes, min(n, (i + 1) * piece_bytes)), any piece_bytes >= 1 -- what icnv_deflate_pieces_dev
 *               computes of its input, for a buffer that is already there.  crc32_combine folds them (device.py).
 * The outputs are functions of the inputs alone.  src needs no alignment.  n_units == 0 (n == 0 for the scan and the CRC) is a
 * valid empty call.  The measure and the decode WAIT on `stream` once, for their check kernel's word; the CRC does not wait.
 * ICNV_ERR_ARG before the kernel that does the work: a negative size; a null pointer with work to do; int64 arrays not aligned
 *   to 8 bytes, int32 / uint32 arrays not to 4; piece_bytes < 1; and, by a small check kernel over the units, a start[i]
 *   outside [0, n), and for the decode an end[i] outside [start[i], n] or an output range outside [0, out_cap].
 * Timer names: "inflate_scan", "inflate_measure", "inflate_units", "crc32_pieces". */
#define ICNV_INFLATE_OK_MARKER 0
#define ICNV_INFLATE_OK_FINAL 1
#define ICNV_INFLATE_TRUNCATED 2
#define ICNV_INFLATE_TOO_LONG 3
#define ICNV_INFLATE_BAD_STREAM 4
#define ICNV_INFLATE_NEEDS_HISTORY 5
int icnv_inflate_scan_dev(const uint8_t *src, int64_t n, int64_t *cand, int64_t cand_cap, int64_t *n_cand /* HOST */, void *stream);
int icnv_inflate_measure_dev(const uint8_t *src, int64_t n, const int64_t *start, int64_t n_units, int64_t max_in, int64_t *end,
                             int64_t *out_len, int32_t *status, void *stream);
int icnv_inflate_units_dev(const uint8_t *src, int64_t n, const int64_t *start, const int64_t *end, const int64_t *out_off,
                           const int64_t *out_len, int64_t n_units, uint8_t *out, int64_t out_cap, int32_t *status, void *stream);
int icnv_crc32_pieces_dev(const uint8_t *src, int64_t n, int64_t piece_bytes, uint32_t *crc, void *stream);

/* ---- INFLATE with unknown history (K30) ---------------------------------------------------------------------------------------------
 * Any raw DEFLATE stream, written by any deflater without flush points (R's gzfile, Python's GzipFile, gzip, 10x), inflated in
 * parallel: a second route, tried where K29's gives up.  The stream is src[0, n): the bytes between the gzip header and the
 * 8-byte trailer.  Bit b of the stream is bit b & 7 of byte b >> 3.  W = 32 768.
 *   candidate   a bit offset b where the bits read BFINAL = 0, BTYPE = 10 and the dynamic header behind them is accepted by the
 *               rules K29 lists under BAD_STREAM, entirely inside the stream.  Fixed and stored blocks cannot be recognised:
 *               they are no candidates and are decoded by the unit that runs into them.  A false candidate (the pattern inside
 *               compressed or stored data) costs one wasted measure and is never reached by the chain.
 *   unit        starts at bit s -- bit 0, or a candidate -- and decodes block after block.  It ends with
 *     ICNV_GUNZIP_OK_BOUNDARY   ahead of a block header (not its own first) it stands on a bit offset that is in the candidate
 *                               list handed to the call (a binary search: the list must ascend); end = that offset
 *     ICNV_GUNZIP_OK_FINAL      behind a block with BFINAL; end = the bit offset rounded up to a whole byte
 *     ICNV_GUNZIP_TRUNCATED     ran into src + n
 *     ICNV_GUNZIP_TOO_LONG      needed a byte at or beyond (s >> 3) + max_in (the measure only)
 *     ICNV_GUNZIP_BAD_STREAM    K29's causes; a distance beyond q + W (below); for the symbols call any disagreement with the
 *                               caller's end / out_len.
 *               There is no NEEDS_HISTORY.  The host walks end -> start from bit 0 (infercnv_amd/gunzip.py).
 *   symbols     a unit produces out_len symbols of 16 bits.  A value below 256 is that byte.  0x8000 | w, w in [0, W), is "the
 *               byte at position w of the W bytes in front of this unit's output" (w = W - 1: the byte just before it).  A
 *               match of distance d that starts at unit position q produces for k = 0 .. len - 1 the symbol at unit position
 *               q + k - d: when that is >= 0 the stored symbol, which may itself be a marker (an overlapping match over markers
 *               repeats them), else the marker 0x8000 | (W + q + k - d).  d > q + W is BAD_STREAM.
 *   places      unit i's symbols lie at sym[out_off[i], out_off[i] + out_len[i]) and its bytes at the same indices of out;
 *               out_off are the prefix sums of out_len, from 0 (checked).
 *   tails       goes through the units IN ORDER and resolves the last min(W, out_len[i]) symbols of unit i into out; a marker
 *               reads out[out_off[i] - W + w].  By induction those bytes are final: the tails of the units before cover the W
 *               bytes in front of a unit however short those units are.  A marker that points in front of byte 0 sets *bad and
 *               writes nothing.  The only sequential step: one workgroup, at most W symbols per unit.
 *   resolve     everything in front of the tails, all units in parallel, by the same rule into the same out.  Afterwards out
 *               is the inflated stream (icnv_crc32_pieces_dev checks it).
 *               A malformed stream is an ordinary input, as in K29: every load is tested against the stream's limit, every
 *               store against the unit's own range of sym / out, and every loop takes at least one bit (a stored block: four
 *               bytes) per round.
 * icnv_gunzip_find_dev      cand (DEVICE int64 [cand_cap]) receives EVERY candidate in ascending order, *n_cand (HOST) their
 *               number.  A lane per bit offset; count, prefix, emit: no atomics.  WAITS on `stream` for the count; when it
 *               exceeds cand_cap the call returns ICNV_ERR_ARG with *n_cand set and nothing written to cand.
 * icnv_gunzip_measure_dev   parses the unit at every start[i] (DEVICE int64, bits) without producing symbols: end[i] (bits),
 *               out_len[i], status[i].  cand / n_cand: the stops.  max_in: the most compressed bytes a unit may take.
 * icnv_gunzip_symbols_dev   decodes unit i into sym[out_off[i], out_off[i] + out_len[i]).  A unit whose decode does not end
 *               exactly at end[i] with exactly out_len[i] symbols gets BAD_STREAM; nothing outside its range was written.
 * icnv_gunzip_tails_dev     *bad (DEVICE int32) is set to 1 or left alone (the caller zeroes it); *markers (DEVICE int64)
 *               receives the number of markers among the tails' symbols.
 * icnv_gunzip_resolve_dev   *bad as above.
 * The outputs are functions of the inputs alone.  src needs no alignment.  n_units == 0 is a valid empty call (n < 3 for the
 * finder).  Every call but the finder WAITS on `stream` once, for its check kernel's word.
 * ICNV_ERR_ARG before the kernel that does the work: a negative size; n beyond 2^40 (the finder: 2^32); a null pointer with work to do; int64
 *   arrays not aligned to 8 bytes, int32 to 4, sym to 2; and, by a small check kernel over the units, a start[i] outside
 *   [0, 8 n), an end[i] outside [start[i], 8 n], places that are not the prefix sums of out_len inside [0, sym_cap / out_cap].
 * Timer names: "gunzip_find", "gunzip_measure", "gunzip_symbols", "gunzip_tails", "gunzip_resolve". */
#define ICNV_GUNZIP_OK_BOUNDARY 0
#define ICNV_GUNZIP_OK_FINAL 1
#define ICNV_GUNZIP_TRUNCATED 2
#define ICNV_GUNZIP_TOO_LONG 3
#define ICNV_GUNZIP_BAD_STREAM 4
int icnv_gunzip_find_dev(const uint8_t *src, int64_t n, int64_t *cand, int64_t cand_cap, int64_t *n_cand /* HOST */, void *stream);
int icnv_gunzip_measure_dev(const uint8_t *src, int64_t n, const int64_t *cand, int64_t n_cand, const int64_t *start, int64_t n_units,
                            int64_t max_in, int64_t *end, int64_t *out_len, int32_t *status, void *stream);
int icnv_gunzip_symbols_dev(const uint8_t *src, int64_t n, const int64_t *cand, int64_t n_cand, const int64_t *start, const int64_t *end,
                            const int64_t *out_off, const int64_t *out_len, int64_t n_units, uint16_t *sym, int64_t sym_cap, int32_t *status,
                            void *stream);
int icnv_gunzip_tails_dev(const uint16_t *sym, const int64_t *out_off, const int64_t *out_len, int64_t n_units, uint8_t *out, int64_t out_cap,
                          int32_t *bad, int64_t *markers, void *stream);
int icnv_gunzip_resolve_dev(const uint16_t *sym, const int64_t *out_off, const int64_t *out_len, int64_t n_units, uint8_t *out, int64_t out_cap,
                            int32_t *bad, void *stream);

/* ---- 2-D median denoise -------------------------------------------------- */
/* apply_median_filtering / .median_filter (R/noise_reduction.R:43-113): for
 * every (tile, chromosome) block -- tile = one tumour subcluster or one whole
 * reference group, cells in stored order -- out[p,q] = median over the clamped
 * (window_size+2)^2 neighbourhood.  Cells in no tile are copied through.
 * A NaN is not looked for: a window that holds one gets a value that depends on
 * the kernel that served it.  icnv_median_filter_na[_dev] below honours R's NA. */
int icnv_median_filter(const double *expr_in, double *expr_out, int64_t G, int64_t C,
                       const int32_t *chr_start, int32_t n_chr, const int32_t *tile_idx,
                       const int32_t *tile_off, int32_t n_tiles, int32_t window_size);
int icnv_median_filter_dev(const double *expr_in, double *expr_out, int64_t G, int64_t C,
                           const int32_t *chr_start, int32_t n_chr, const int32_t *tile_idx,
                           const int32_t *tile_off, int32_t n_tiles, int32_t window_size,
                           void *stream);
/* The same filter with R's NA result (K19, csrc/median_na_kernels.hip): median() returns NA as soon as its argument holds
 * one NA or NaN (R/noise_reduction.R:107), so an output is NA exactly when its window holds one.  Opt-in, like
 * ICNV_ST_NA_AWARE for the chain; icnv_median_filter[_dev] keep their contract and their code path.
 *   NA        an element whose bits satisfy (bits & 0x7FFFFFFFFFFFFFFF) > 0x7FF0000000000000: any NaN, R's NA_real_
 *             included (the bits are tested, never x != x).  +-Inf is a number, as in the plain entry.
 *   blocks    as icnv_median_filter: one block per (tile, chromosome) pair, a tile's cells in the order of its index list.
 *   window    of output (p, q) of an n x m block, 1-based: [max(1, p - h), min(n, p + h)] x [max(1, q - h), min(m, q + h)]
 *             with h = (window_size - 1) / 2 + 1.  The reference's ifelse pairs (:102-106) reduce to exactly this clamp:
 *             `p <= h ? 1 : p - h` is max(1, p - h), and `p >= n - h ? n : p + h` is min(n, p + h).
 *   tiled     out[p, q] = NA_real_ (bits 0x7FF00000000007A2) if the window holds at least one NA; otherwise bit for bit
 *             what icnv_median_filter returns for that output on the same input -- whatever the NAs elsewhere hold.
 *   untiled   cells in no tile are copied through bit for bit, NaN payloads included; they poison nothing.
 *   n_na_out  HOST, nullable: the number of NA elements of the matrix, tiled or not.
 * Refusals, window_size limits and the aliasing rule are icnv_median_filter's, checked before any launch.  A cell listed in
 * several tiles is NA if one of its windows holds an NA and otherwise as the plain entry leaves it.  The entry reads the
 * matrix once to look for NAs (a bit mask of G * C / 8 bytes of pool scratch), WAITS for the count on `stream` -- the one
 * host wait, so it cannot be captured into a graph -- and without an NA launches the plain filter on the caller's input.
 * With NAs it filters a cleaned copy (G * C doubles of pool scratch) and stores the NAs of the dilated mask afterwards.
 * The host-buffer entry deals whole tiles to the devices of icnv_set_devices as icnv_median_filter does.
 * Timer names: "median_na_scan", "median_na_clean", "median_na_fixup" (and the plain filter's "median_filter"). */
int icnv_median_filter_na(const double *expr_in, double *expr_out, int64_t G, int64_t C,
                          const int32_t *chr_start, int32_t n_chr, const int32_t *tile_idx,
                          const int32_t *tile_off, int32_t n_tiles, int32_t window_size,
                          int64_t *n_na_out);
int icnv_median_filter_na_dev(const double *expr_in, double *expr_out, int64_t G, int64_t C,
                              const int32_t *chr_start, int32_t n_chr, const int32_t *tile_idx,
                              const int32_t *tile_off, int32_t n_tiles, int32_t window_size,
                              int64_t *n_na_out /* HOST, nullable */, void *stream);

/* ---- reference z-score gene filter (K32) ---------------------------------------------------------------------------------------
 * The statistics of the gene filter of define_signif_tumor_subclusters (R/inferCNV_tumor_subclusters.R:45-71) on a resident
 * matrix: over the N = n_ref * G values v of the listed reference cells of a (C, G) DEVICE matrix whose rows lie ld >= G apart,
 *   mean       sum(v) / N
 *   sd         sqrt(sum((v - mean)^2) / (N - 1)), around the ROUNDED mean (R's two-pass sd); NaN when N < 2, as R's
 *   row_mean   per gene g: sum over the listed cells of |(v - mean) / sd| / n_ref, each term two fp64 operations as R evaluates
 *              (ref - mean) / sd, with the rounded mean and sd
 * The three sums are accumulated in double-double (about 104 bits) and rounded to double once at the end, so every result is
 * the correctly rounded value of its exact expression whenever that value lies further from a rounding boundary than the
 * accumulation's error: N * 2^-104 of the sum of the |terms|.  That is every input the pipeline produces; it is not
 * certified, and a mean that is the small remainder of large cancelling values can miss.  tests/zscore_restate.py states the
 * exact expressions with fractions.  The squares are taken at a power-of-two scale, so values up to 2^1022 and down to the
 * subnormals keep a finite, correctly scaled sd; a non-finite value among the listed cells makes all three results NaN.
 * The `>= 0.8` decision is the caller's.  The host route (tumor_subclusters.zscore_outlier_genes) follows R's long-double
 * sums, which round more than once: its mean, sd or a row mean may differ from these by an ulp.
 * The order of every sum depends on (G, n_ref) and the order of the list alone: no atomics, the same bits on every run.  A cell
 * listed twice counts twice.  ref_cells: HOST list, 0-based, any order.  mean_sd: HOST [2].  row_mean: DEVICE [G].
 * ICNV_ERR_ARG before any launch, with the outputs untouched: a null pointer, dimensions outside 1 .. 2^31 - 1, ld < G,
 * n_ref < 1, an entry that is not a cell.  Synchronises.  Timer names: "zscore_filter_pass", "zscore_filter_finish". */
int icnv_zscore_gene_filter_dev(const double *x, int64_t ld, int64_t G, int64_t C, const int32_t *ref_cells, int64_t n_ref, double *mean_sd,
                                double *row_mean, void *stream);

/* ---- K34: count matrices out of R's serialisation stream (.rds / .rda) ----------------------------------------------------------
 * What readRDS hands CreateInfercnvObject (R/inferCNV.R:151-162) -- a matrix, a data.frame or a dgCMatrix -- decoded from the
 * serialised stream where it lies.  `stream` is the stream as a DEVICE uint8 vector of stream_bytes bytes; every payload is
 * named by its BYTE offset in it.  Neither the offsets nor `stream` itself need any alignment: the kernels load the aligned
 * 32-bit words that cover an element and shift, and a word that is not wholly inside [stream, stream + stream_bytes) is read as
 * the single bytes of it that are.  No byte outside the stream is loaded, so the stream may be a view of a larger allocation.
 * All index arithmetic is 64-bit.  Elements are big-endian (XDR).
 *
 * icnv_rds_columns_dev: dense columns.  Output row j (DEVICE doubles, rows ld >= rows apart: the (cells, genes) layout) is the
 * `rows` elements that start at byte col_off[j], of kind col_kind[j] (col_off, col_kind: DEVICE [n_out]):
 *   ICNV_RDS_REAL  8-byte elements, bytes reversed and nothing else: integer loads and stores, so a NaN keeps its payload
 *                  (NA_real_, 0x7FF00000000007A2, is one)
 *   ICNV_RDS_INT   4-byte elements, the exact int -> double conversion; NA_integer_ (INT_MIN) becomes NA_real_
 * For a matrix payload col_off[j] = payload + cells[j] * rows * elem_size; for a data.frame the column's own payload.  The
 * same column may be asked for twice; bytes that no requested column covers are not read; the padding between rows - 1 and ld
 * is not written.  ICNV_ERR_ARG before any launch (col_off and col_kind are fetched for it): a null pointer, n_out, rows < 1,
 * ld < rows, stream_bytes < 0, a kind that is neither, a column that does not lie inside the stream.  The call waits for the
 * stream once, for that fetch, and NOT after its launch: it returns with the kernel queued on hip_stream, and the kernel reads
 * col_off and col_kind -- keep both, the stream and out alive until hip_stream has been synchronised.  Timer: "rds_columns".
 *
 * icnv_rds_csc_check_dev / icnv_rds_csc_fill_dev: a dgCMatrix (slots i, p, x at their byte offsets; G rows, C columns, nnz
 * entries) to the CSC arrays of icnv_counts.  cells: DEVICE list of n_out file columns (0-based, any order) or null with
 * n_out = C: every column in order.  Output column k is file column cells[k], its entries in stream order.
 * The check validates the WHOLE of p -- p[0] == 0 (ICNV_RDS_P_FIRST), p[j] <= p[j + 1] (ICNV_RDS_P_DESCENT, at index j + 1),
 * p[C] == nnz (ICNV_RDS_P_LAST, at index C) -- and every entry e of the SELECTED columns: 0 <= i[e] < G (ICNV_RDS_ROW_RANGE),
 * i strictly increasing within a column (ICNV_RDS_ROW_ORDER, Matrix's own validity rule: it catches a pair stored twice; equal
 * rows on both sides of a column boundary are valid), x[e] an integer value in 0 .. 2^31 - 1 (ICNV_RDS_VALUE: a fraction, a
 * negative value, 2^31, an infinity, a NaN; -0 counts as 0; tested on the bits, no floating-point operation).  Entries of
 * columns that are not selected are not examined (K26's rule: over a deal where every column has one owner every entry is
 * still examined once).  status (HOST [3]) receives {code, file column, index}: ICNV_RDS_OK, or the violation with the smallest
 * index -- p violations (index: into p; column: min(index, C - 1)) before entry violations (index: the entry's in the stream;
 * column: the file column that holds it); among codes at one index the smallest.  The choice is an integer atomic minimum on a
 * 64-bit key and does not depend on launch order.  On ICNV_RDS_OK colptr (DEVICE int64 [n_out + 1]) is written by a scan and
 * *nnz_out (HOST) is colptr[n_out]; on a violation nothing is written but status.  Returns ICNV_OK in both cases.
 * The fill writes rowidx and vals (DEVICE int32 [out_nnz], out_nnz = the check's *nnz_out) for the same arguments and the
 * check's colptr.  It must follow a check that found no violation; after anything else what it writes is unspecified, but
 * every access stays inside the stream and the outputs.
 * ICNV_ERR_ARG before any launch (cells is fetched for it): a null pointer, G, C < 1 or beyond 2^31 - 1, nnz < 0 or beyond
 * 2^31 - 1, a payload that does not lie inside the stream, n_out < 1, a cells entry that is no column, out_nnz < 0.
 * The check and the fill synchronise before they return.  Timers: "rds_csc_check", "rds_csc_fill".
 * icnv_rds_counts_stats: {calls of columns, columns, elements, calls of check, entries examined, refused checks, calls of fill,
 * entries written} since the last reset (the first n of them). */
#define ICNV_RDS_INT 13
#define ICNV_RDS_REAL 14
#define ICNV_RDS_OK 0
#define ICNV_RDS_P_FIRST 1
#define ICNV_RDS_P_DESCENT 2
#define ICNV_RDS_P_LAST 3
#define ICNV_RDS_ROW_RANGE 4
#define ICNV_RDS_ROW_ORDER 5
#define ICNV_RDS_VALUE 6
int icnv_rds_columns_dev(const uint8_t *stream, int64_t stream_bytes, const int64_t *col_off, const int32_t *col_kind, int64_t n_out,
                         int64_t rows, double *out, int64_t ld, void *hip_stream);
int icnv_rds_csc_check_dev(const uint8_t *stream, int64_t stream_bytes, int64_t i_off, int64_t p_off, int64_t x_off, int64_t G, int64_t C,
                           int64_t nnz, const int32_t *cells, int64_t n_out, int64_t *colptr, int64_t *status, int64_t *nnz_out,
                           void *hip_stream);
int icnv_rds_csc_fill_dev(const uint8_t *stream, int64_t stream_bytes, int64_t i_off, int64_t p_off, int64_t x_off, int64_t G, int64_t C,
                          int64_t nnz, const int32_t *cells, int64_t n_out, const int64_t *colptr, int32_t *rowidx, int32_t *vals,
                          int64_t out_nnz, void *hip_stream);
int icnv_rds_counts_stats(int64_t *out, int32_t n);
void icnv_rds_counts_stats_reset(void);

/* ---- profiling hooks (used by bench.py) --------------------------------- */
/* When enabled, every kernel launch is bracketed by hipEvents recorded on the
 * launch stream; icnv_timing_get() synchronises those events and returns the
 * accumulated milliseconds and launch count of one kernel family:
 * "chain_apply", "chain_gene_sums", "chain_cell_stats", "viterbi",
 * "group_means", "broadcast_states", "median_filter", ...
 * on = 1: every kernel family; on = 2: only "chain_apply" and "viterbi" (an event pair costs a few microseconds of
 * stream time: fourteen pairs per bench step are 2.5 % of it, two pairs are not); on = 0: off. */
void icnv_timing_enable(int on);
void icnv_timing_reset(void);
int icnv_timing_get(const char *kernel, double *total_ms, int64_t *launches);

#ifdef __cplusplus
}
#endif
#endif /* ICNV_H */
