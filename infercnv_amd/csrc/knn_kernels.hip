// Exact k-nearest neighbours among the cells of a problem: RANN::nn2(t(expr_data), k = k_nn)$nn.idx as the reference's
// Leiden subclustering calls it (R/inferCNV_tumor_subclusters.R:726, .leiden_simple_snn; per chromosome x group at
// :646-697).  DESIGN.md section 4 K8.  Launches of one row block (all problems of a batch in every launch):
//
//   knn_mean_kernel     per (problem, gene) shift: the mean of the gene over the problem's first <= 256 cells
//   knn_gather_kernel   Y_p = x[genes_p, cells_p] - shift, compact (one row of ld_p doubles per cell), and ||y_i||^2
//   knn_screen_kernel   d~2 = ||y_i||^2 + ||y_j||^2 - 2 y_i.y_j on the matrix cores (gram::tile_product),
//                       stored as the upper 32 bits of the order keys of d~2 + e_ij and d~2 - e_ij (e_ij: DESIGN K8)
//   knn_select_kernel   per query row: b = the k-th smallest upper key (radix select), candidates = {j : lower key <= b}
//   knn_refine_kernel   per query row: d2 of every candidate exactly as the contract defines it, ranked by (d2, j)
//   knn_exact_kernel    rows whose candidates overflowed (or every row, ICNV_KNN_EXHAUSTIVE): d2 of all n_p cells ...
//   knn_exact_select_kernel   ... and the k smallest by (d2, j)
//
// This file is compiled with -ffp-contract=off (Makefile): the exact d2 is a sequential sum of rounded squares of
// rounded differences, s = s + t * t, and must not become an FMA.
#include "icnv_internal.h"
#include "gram_mfma.h"
#include "knn_internal.h"

namespace icnv {

namespace {

using gram::dbl4_t;

__device__ __forceinline__ uint64_t order_key(double v) {   // monotone map of doubles onto unsigned integers
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// problem of a global query row / of a piece: the last p with off[p] <= v
__device__ __forceinline__ int find_segment(const int64_t *__restrict__ off, int n, int64_t v) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ void knn_mean_kernel(KnnArgs a) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.total_genes) return;
    const int p = find_segment(a.gene_off, a.n_prob, t);
    const int32_t g = a.gene_idx[t];
    const int64_t c0 = a.cell_off[p];
    const int n = (int)(a.cell_off[p + 1] - c0);
    const int m = n < KNN_SHIFT_CELLS ? n : KNN_SHIFT_CELLS;
    double s = 0.0;
    for (int c = 0; c < m; ++c) s += a.x[g + (int64_t)a.G * a.cell_idx[c0 + c]];
    a.shift[t] = s / m;
}

// one workgroup per (problem, cell): y = x - shift over the problem's genes, zero padding up to ld_p, norm = sum y^2
__global__ void __launch_bounds__(256) knn_gather_kernel(KnnArgs a) {
    const int64_t row = blockIdx.x;   // global query row
    const int p = find_segment(a.cell_off, a.n_prob, row);
    const int64_t g0 = a.gene_off[p];
    const int Gp = (int)(a.gene_off[p + 1] - g0);
    const int ld = a.ld[p];
    const double *xc = a.x + (int64_t)a.G * a.cell_idx[row];
    double *y = a.Y + a.y_off[p] + (row - a.cell_off[p]) * ld;
    double s = 0.0;
    for (int g = threadIdx.x; g < ld; g += 256) {
        double v = 0.0;
        if (g < Gp) v = xc[a.gene_idx[g0 + g]] - a.shift[g0 + g];
        y[g] = v;
        s += v * v;
    }
    __shared__ double red[256];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.norm[row] = red[0];
}

// The screen's bound (DESIGN K8): |d2_seq - d~2| <= e_ij for every pair.
__device__ __forceinline__ double screen_bound(double d, double ni, double nj, int Gp) {
    const double u = 0x1p-53;
    return (((4.0 * Gp + 16.0) * (ni + nj) + 4.0 * fabs(d)) * u + (8.0 * Gp + 32.0) * 0x1p-1022) * (1.0 + 0x1p-10);
}

// One workgroup per DT x DT tile of a piece (rows [r0, r0 + nr) of problem p against all its n_p cells).
template <int WM>
__global__ void __launch_bounds__(256, (WM == 4 ? 2 : 4)) knn_screen_kernel(KnnArgs a, KnnBlock b) {
    constexpr int DT = 32 * WM;
    constexpr int RPT = DT / 64;
    extern __shared__ __attribute__((aligned(16))) double smem_d[];
    const int pc = find_segment(b.tile_off, b.n_pieces, blockIdx.x);
    const int p = b.piece_prob[pc];
    const int64_t lt = blockIdx.x - b.tile_off[pc];
    const int np = (int)(a.cell_off[p + 1] - a.cell_off[p]);
    const int ntj = (np + DT - 1) / DT;
    const int ti = (int)(lt / ntj), tj = (int)(lt - (int64_t)ti * ntj);
    const int r0 = b.piece_r0[pc], nr = b.piece_nr[pc];
    const int ld = a.ld[p];
    const double *Yp = a.Y + a.y_off[p];

    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wr = w >> 1, wc = w & 1;
    const int lrow = t >> 2;
    const double *pa[RPT], *pb[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const int ra = ti * DT + lrow + 64 * r, rb = tj * DT + lrow + 64 * r;   // ra: within the piece, rb: within the problem
        pa[r] = ra < nr ? Yp + (int64_t)(r0 + ra) * ld : nullptr;
        pb[r] = rb < np ? Yp + (int64_t)rb * ld : nullptr;
    }
    dbl4_t acc[WM][WM];
    gram::tile_product<WM>(pa, pb, ld, smem_d, acc);

    const int Gp = (int)(a.gene_off[p + 1] - a.gene_off[p]);
    const double *nrm = a.norm + a.cell_off[p];
    uint32_t *scr = b.screen + 2 * b.piece_scr[pc];   // row ra: upper keys at [2 np ra, +np), lower keys at [2 np ra + np, +np)
#pragma unroll
    for (int aa = 0; aa < WM; ++aa)
#pragma unroll
        for (int bb = 0; bb < WM; ++bb)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int ra = ti * DT + wr * 16 * WM + aa * 16 + (lane >> 4) + 4 * reg;
                const int col = tj * DT + wc * 16 * WM + bb * 16 + (lane & 15);
                if (ra < nr && col < np) {
                    const double ni = nrm[r0 + ra], nj = nrm[col];
                    const double d = (ni + nj) - 2.0 * acc[aa][bb][reg];
                    const double e = screen_bound(d, ni, nj, Gp);
                    uint32_t *row = scr + (int64_t)2 * np * ra;
                    row[col] = (uint32_t)(order_key(d + e) >> 32);
                    row[np + col] = (uint32_t)(order_key(d - e) >> 32);
                }
            }
}

// ---------------------------------------------------------------- one wavefront per query row
struct RowRef {
    int p;        // problem
    int pc;       // piece
    int lr;       // row within the piece
    int r0;       // the piece's first row within the problem
    int64_t row;  // global query row
    int np;
};
__device__ __forceinline__ RowRef row_of_block(const KnnArgs &a, const KnnBlock &b, int64_t brow) {
    RowRef r;
    const int pc = find_segment(b.row_off, b.n_pieces, brow);
    r.p = b.piece_prob[pc];
    r.pc = pc;
    r.lr = (int)(brow - b.row_off[pc]);
    r.r0 = b.piece_r0[pc];
    r.row = a.cell_off[r.p] + r.r0 + r.lr;
    r.np = (int)(a.cell_off[r.p + 1] - a.cell_off[r.p]);
    return r;
}
__device__ __forceinline__ uint64_t lanes_below() { return (1ull << (threadIdx.x & 63)) - 1ull; }

// Radix step over one digit: hist[256] (LDS, this wavefront) holds the counts of the digit among the keys that match the
// prefix; returns the digit of the `need`-th smallest (1-based) and lowers `need` by the count of the smaller digits.
__device__ __forceinline__ int radix_pick(const uint32_t *hist, uint32_t &need) {
    const int lane = threadIdx.x & 63;
    const uint32_t h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
    const uint32_t mine = h0 + h1 + h2 + h3;
    uint32_t incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    const uint32_t excl = incl - mine;
    const uint64_t hit = __ballot(excl < need && need <= incl);
    const int src = __ffsll((unsigned long long)hit) - 1;
    uint32_t before = __shfl(excl, src, 64);
    uint32_t c[4] = {__shfl(h0, src, 64), __shfl(h1, src, 64), __shfl(h2, src, 64), __shfl(h3, src, 64)};
    int d = 0;
    while (d < 3 && before + c[d] < need) { before += c[d]; ++d; }
    need -= before;
    return 4 * src + d;
}

// add one to hist[digit] for every active lane; a wavefront whose active lanes share the digit adds once
__device__ __forceinline__ void hist_add(uint32_t *hist, bool active, uint32_t digit) {
    const uint64_t act = __ballot(active);
    if (!act) return;
    const int first = __ffsll((unsigned long long)act) - 1;
    const uint32_t d0 = __shfl(digit, first, 64);
    const uint64_t same = __ballot(active && digit == d0);
    if (same == act) {
        if ((int)(threadIdx.x & 63) == first) atomicAdd(&hist[d0], (uint32_t)__popcll(act));
    } else if (active) {
        atomicAdd(&hist[digit], 1u);
    }
}

// knn_select_kernel: 64 threads = one query row of the block.  Candidates (ascending j) go to cand[brow * cap ..], their count
// (possibly > cap: the row then takes the exhaustive pass) to ncand[brow].
__global__ void __launch_bounds__(64) knn_select_kernel(KnnArgs a, KnnBlock b) {
    const int64_t brow = blockIdx.x;
    const RowRef r = row_of_block(a, b, brow);
    const int pc = r.pc;
    const uint32_t *up = b.screen + 2 * (b.piece_scr[pc] + (int64_t)r.np * r.lr);
    const uint32_t *lo = up + r.np;
    const int lane = threadIdx.x;
    __shared__ uint32_t hist[256];
    uint32_t need = (uint32_t)a.k, prefix = 0;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        for (int i = lane; i < 256; i += 64) hist[i] = 0;
        __syncthreads();
        const uint32_t mask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
        for (int j0 = 0; j0 < r.np; j0 += 64) {
            const int j = j0 + lane;
            const uint32_t key = j < r.np ? up[j] : 0u;
            hist_add(hist, j < r.np && (key & mask) == prefix, (key >> shift) & 255u);
        }
        __syncthreads();
        prefix |= (uint32_t)radix_pick(hist, need) << shift;
        __syncthreads();
    }
    // candidates: lower key <= prefix (the upper 32 bits of the k-th smallest upper bound's key)
    int32_t *cand = b.cand + brow * b.cap;
    int count = 0;
    for (int j0 = 0; j0 < r.np; j0 += 64) {
        const int j = j0 + lane;
        const bool take = j < r.np && lo[j] <= prefix;
        const uint64_t m = __ballot(take);
        const int pos = count + __popcll(m & lanes_below());
        if (take && pos < b.cap) cand[pos] = j;
        count += __popcll(m);
    }
    if (lane == 0) {
        b.ncand[brow] = count;
        if (count > b.cap || count < a.k) atomicAdd((unsigned long long *)&a.stats[KNN_STAT_OVERFLOW_ROWS], 1ull);
        else atomicAdd((unsigned long long *)&a.stats[KNN_STAT_CANDIDATES], (unsigned long long)count);
    }
}

// Exact d2 (the contract's sequential sum over genes_p, in list order) of query cell `qi` against the cells of 64 lanes (cj < 0:
// no cell); one wavefront, the candidate columns staged through LDS KNN_GC genes at a time.  Called by every lane.
__device__ __forceinline__ double exact_d2_wave(const KnnArgs &a, int p, int32_t qi, int32_t cj, double *tile /* 64 x (GC + 1) */,
                                                double *q /* GC */, int32_t *cells /* 64 */) {
    const int lane = threadIdx.x & 63;
    const int64_t g0p = a.gene_off[p];
    const int Gp = (int)(a.gene_off[p + 1] - g0p);
    constexpr int GC = KNN_GC, LD = KNN_GC + 1;
    __syncthreads();
    cells[lane] = cj;
    __syncthreads();
    double s = 0.0;
    const double *xq = a.x + (int64_t)a.G * qi;
    for (int gb = 0; gb < Gp; gb += GC) {
        const int gl = lane & (GC - 1);
        const int g = gb + gl;
        const int32_t gi = g < Gp ? a.gene_idx[g0p + g] : 0;
        if (lane < GC) q[gl] = g < Gp ? xq[gi] : 0.0;
        for (int cc = lane / GC; cc < 64; cc += 64 / GC) {
            const int32_t c = cells[cc];
            tile[cc * LD + gl] = (c >= 0 && g < Gp) ? a.x[gi + (int64_t)a.G * c] : 0.0;
        }
        __syncthreads();
        const int ge = Gp - gb < GC ? Gp - gb : GC;
        for (int u = 0; u < ge; ++u) {
            const double t = __dsub_rn(q[u], tile[lane * LD + u]);
            s = __dadd_rn(s, __dmul_rn(t, t));
        }
        __syncthreads();
    }
    return s;
}

// (d, j) < (d', j') for the contract's order
__device__ __forceinline__ bool key_less(double d, int32_t j, double d2, int32_t j2) { return d < d2 || (d == d2 && j < j2); }

// Writes the k smallest of n (d2, j) pairs held in LDS (n >= k; distinct j) to the output row, in (d2, j) order.
__device__ __forceinline__ void rank_and_write(const KnnArgs &a, int64_t row, const double *d, const int32_t *j, int n) {
    const int lane = threadIdx.x & 63;
    int32_t *oi = a.nn_idx + row * a.k;
    double *od = a.nn_dist + row * a.k;
    for (int c = lane; c < n; c += 64) {
        int rank = 0;
        for (int c2 = 0; c2 < n; ++c2) rank += key_less(d[c2], j[c2], d[c], j[c]) ? 1 : 0;
        if (rank < a.k) {
            oi[rank] = j[c];
            od[rank] = __dsqrt_rn(d[c]);
        }
    }
}

__global__ void __launch_bounds__(64) knn_refine_kernel(KnnArgs a, KnnBlock b) {
    const int64_t brow = blockIdx.x;
    const int count = b.ncand[brow];
    if (count > b.cap || count < a.k) return;      // the exhaustive pass takes this row
    const RowRef r = row_of_block(a, b, brow);
    extern __shared__ __attribute__((aligned(16))) double smem_d[];
    double *tile = smem_d;                          // 64 x (GC + 1)
    double *q = tile + 64 * (KNN_GC + 1);           // GC
    double *dd = q + KNN_GC;                        // cap
    int32_t *jj = reinterpret_cast<int32_t *>(dd + b.cap);   // cap
    int32_t *cells = jj + b.cap;                    // 64
    const int32_t *cand = b.cand + brow * b.cap;
    const int32_t *cidx = a.cell_idx + a.cell_off[r.p];
    const int32_t qi = cidx[r.r0 + r.lr];
    const int lane = threadIdx.x;
    for (int c0 = 0; c0 < count; c0 += 64) {
        const int c = c0 + lane;
        const int32_t j = c < count ? cand[c] : -1;
        const double s = exact_d2_wave(a, r.p, qi, j >= 0 ? cidx[j] : -1, tile, q, cells);
        if (c < count) { dd[c] = s; jj[c] = j; }
    }
    __syncthreads();
    rank_and_write(a, r.row, dd, jj, count);
}

// Exhaustive pass, part 1: one wavefront per flagged row writes the exact d2 of all n_p cells over the row's screen entries
// (8 bytes per pair, as the two keys took).
__global__ void __launch_bounds__(64) knn_exact_kernel(KnnArgs a, KnnBlock b) {
    const int64_t brow = blockIdx.x;
    if (!b.all_exact) {
        const int count = b.ncand[brow];
        if (count <= b.cap && count >= a.k) return;
    }
    const RowRef r = row_of_block(a, b, brow);
    const int pc = r.pc;
    double *drow = reinterpret_cast<double *>(b.screen) + b.piece_scr[pc] + (int64_t)r.np * r.lr;
    __shared__ double tile[64 * (KNN_GC + 1)], q[KNN_GC];
    __shared__ int32_t cells[64];
    const int32_t *cidx = a.cell_idx + a.cell_off[r.p];
    const int32_t qi = cidx[r.r0 + r.lr];
    for (int j0 = 0; j0 < r.np; j0 += 64) {
        const int j = j0 + threadIdx.x;
        const double s = exact_d2_wave(a, r.p, qi, j < r.np ? cidx[j] : -1, tile, q, cells);
        if (j < r.np) drow[j] = s;
    }
}

// Exhaustive pass, part 2: the k-th smallest exact d2 (radix select on 64-bit keys), then the cells below it and the first
// (lowest position) cells equal to it, ranked by (d2, j).
__global__ void __launch_bounds__(64) knn_exact_select_kernel(KnnArgs a, KnnBlock b) {
    const int64_t brow = blockIdx.x;
    if (!b.all_exact) {
        const int count = b.ncand[brow];
        if (count <= b.cap && count >= a.k) return;
    }
    const RowRef r = row_of_block(a, b, brow);
    const int pc = r.pc;
    const double *drow = reinterpret_cast<const double *>(b.screen) + b.piece_scr[pc] + (int64_t)r.np * r.lr;
    const int lane = threadIdx.x;
    __shared__ uint32_t hist[256];
    __shared__ double dd[KNN_MAX_K];
    __shared__ int32_t jj[KNN_MAX_K];
    uint32_t need = (uint32_t)a.k;
    uint64_t prefix = 0;
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        for (int i = lane; i < 256; i += 64) hist[i] = 0;
        __syncthreads();
        const uint64_t mask = pass == 0 ? 0ull : (~0ull << (shift + 8));
        for (int j0 = 0; j0 < r.np; j0 += 64) {
            const int j = j0 + lane;
            const uint64_t key = j < r.np ? order_key(drow[j]) : 0ull;
            hist_add(hist, j < r.np && (key & mask) == prefix, (uint32_t)(key >> shift) & 255u);
        }
        __syncthreads();
        prefix |= (uint64_t)radix_pick(hist, need) << shift;
        __syncthreads();
    }
    // `need` is now the number of cells equal to the k-th value that belong to the k nearest
    const int n_less = a.k - (int)need;
    int nl = 0, ne = 0;
    for (int j0 = 0; j0 < r.np; j0 += 64) {
        const int j = j0 + lane;
        const uint64_t key = j < r.np ? order_key(drow[j]) : ~0ull;
        const bool less = j < r.np && key < prefix, eq = j < r.np && key == prefix;
        const uint64_t ml = __ballot(less), me = __ballot(eq);
        const int pl = nl + __popcll(ml & lanes_below()), pe = ne + __popcll(me & lanes_below());
        if (less) { dd[pl] = drow[j]; jj[pl] = j; }
        if (eq && pe < (int)need) { dd[n_less + pe] = drow[j]; jj[n_less + pe] = j; }
        nl += __popcll(ml);
        ne += __popcll(me);
    }
    __syncthreads();
    rank_and_write(a, r.row, dd, jj, a.k);
    if (lane == 0) atomicAdd((unsigned long long *)&a.stats[KNN_STAT_EXACT_ROWS], 1ull);
}

}  // namespace

size_t knn_refine_lds_bytes(int cap) {
    return (size_t)(64 * (KNN_GC + 1) + KNN_GC + cap) * sizeof(double) + (size_t)(cap + 64) * sizeof(int32_t);
}

int launch_knn_prepare(const KnnArgs &a, hipStream_t s) {
    {
        KernelTimer kt("knn_gather", s);
        hipLaunchKernelGGL(knn_mean_kernel, dim3((unsigned)((a.total_genes + 255) / 256)), dim3(256), 0, s, a);
        hipLaunchKernelGGL(knn_gather_kernel, dim3((unsigned)a.total_rows), dim3(256), 0, s, a);
    }
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_knn_block(const KnnArgs &a, const KnnBlock &b, int wm, hipStream_t s) {
    if (!b.all_exact) {
        {
            KernelTimer kt("knn_screen", s);
            if (wm == 4) {
                static DeviceOnce once;
                if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(knn_screen_kernel<4>), (int)gram::lds_bytes(4), once)) return rc;
                hipLaunchKernelGGL(knn_screen_kernel<4>, dim3((unsigned)b.n_tiles), dim3(256), gram::lds_bytes(4), s, a, b);
            } else {
                hipLaunchKernelGGL(knn_screen_kernel<2>, dim3((unsigned)b.n_tiles), dim3(256), gram::lds_bytes(2), s, a, b);
            }
        }
        {
            KernelTimer kt("knn_select", s);
            hipLaunchKernelGGL(knn_select_kernel, dim3((unsigned)b.n_rows), dim3(64), 0, s, a, b);
        }
        {
            KernelTimer kt("knn_refine", s);
            hipLaunchKernelGGL(knn_refine_kernel, dim3((unsigned)b.n_rows), dim3(64), knn_refine_lds_bytes(b.cap), s, a, b);   // <= 30 KB
        }
    }
    {
        KernelTimer kt("knn_exhaustive", s);
        hipLaunchKernelGGL(knn_exact_kernel, dim3((unsigned)b.n_rows), dim3(64), 0, s, a, b);
        hipLaunchKernelGGL(knn_exact_select_kernel, dim3((unsigned)b.n_rows), dim3(64), 0, s, a, b);
    }
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

}  // namespace icnv
