// K14: the per-(column, chromosome) CNV counts of add_to_seurat (.get_features, R/seurat_interaction.R:244-353) and the
// run-length segmentation of state columns into CNV regions (.define_cnv_gene_regions, R/inferCNV_HMM.R:1005-1057).
// Contract: include/icnv.h; design and measurements: DESIGN.md section 4 K14, docs/KERNEL_LOG.md.
//
// Both passes use one shape: a wavefront stages a tile of 64 columns x 128 genes through LDS with 16-byte loads (8 lanes
// cover the 128 contiguous bytes of one column), then ONE LANE PER COLUMN walks the genes, four states per LDS word.  A
// chromosome border is the same gene for every lane, so the flush of a chromosome is a scalar branch; the words a border
// cuts are walked with a byte mask (the masked-out bytes count as the neutral state, which adds nothing).  The row pitch
// of 33 words keeps the 64 lanes on 64 different LDS banks.
#include "cnv_summary_internal.h"

namespace icnv {
namespace {

constexpr int TG = CNVSUM_TILE_GENES;
constexpr int PITCH = TG / 4 + 1;
constexpr uint32_t B80 = 0x80808080u, B01 = 0x01010101u;

__device__ __forceinline__ uint32_t nz_bytes(uint32_t x) {   // bit 7 of every byte of x that is not zero
    return (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & B80;
}
__device__ __forceinline__ uint32_t byte_mask(int lo, int hi) {   // 0xFF in the bytes lo .. hi - 1 (0 <= lo < hi <= 4)
    return (hi == 4 ? 0xFFFFFFFFu : (1u << (8 * hi)) - 1u) & ~((1u << (8 * lo)) - 1u);
}

// genes [t0, t0 + TG) of the list positions [pos0, pos0 + 64) -> lds[row * PITCH + word]; bytes beyond G and rows beyond
// n_pos are zero.  A 16-byte load never reaches past gene G - 1 of its column.
__device__ __forceinline__ void stage_tile(const uint8_t *__restrict__ st, int64_t ld, int32_t G, int64_t n_pos, int64_t pos0,
                                           const int32_t *__restrict__ col_idx, int32_t t0, uint32_t *lds, bool aligned) {
    constexpr int LPR = TG / 16;                       // lanes per row: 16 bytes each
    const int sub = threadIdx.x % LPR, rsub = threadIdx.x / LPR;
    const int32_t g = t0 + sub * 16;
#pragma unroll 4
    for (int i = 0; i < LPR; ++i) {
        const int row = i * (64 / LPR) + rsub;
        const int64_t pos = pos0 + row;
        uint4 q = make_uint4(0u, 0u, 0u, 0u);
        if (pos < n_pos && g < G) {
            const int64_t col = col_idx ? (int64_t)col_idx[pos] : pos;
            const uint8_t *p = st + col * ld + g;
            if (g + 16 <= G) {
                if (aligned) q = *reinterpret_cast<const uint4 *>(p);
                else __builtin_memcpy(&q, p, 16);
            } else {
                const int n = G - g;
                uint32_t v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    uint32_t x = 0;
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (4 * j + k < n) x |= (uint32_t)p[4 * j + k] << (8 * k);
                    v[j] = x;
                }
                q = make_uint4(v[0], v[1], v[2], v[3]);
            }
        }
        uint32_t *dst = lds + row * PITCH + sub * 4;
        dst[0] = q.x; dst[1] = q.y; dst[2] = q.z; dst[3] = q.w;
    }
}

// The counting pass.  Workgroup = one wavefront = 64 columns x the genes [g0, g1) of one chunk.  Per lane and chromosome:
// sad = sum |s - s0|, sum = sum s, nle = #{s <= s0}, nlt = #{s < s0} over 4 * ndw bytes (masked-out bytes are s0), so
// n_loss = nlt, n_gain = 4 ndw - nle, d_gain - d_loss = sum - 4 ndw s0, d_gain + d_loss = sad.  A chromosome that lies
// inside the chunk is stored, one that a chunk border cuts is added (the launch zeroes the output).
template <bool FEAT>
__global__ __launch_bounds__(64) void cnvsum_count_kernel(CnvSumArgs a, int aligned) {
    __shared__ uint32_t lds[64 * PITCH];
    const int lane = threadIdx.x;
    const int64_t col0 = (int64_t)blockIdx.x * 64, col = col0 + lane;
    const bool live = col < a.C;
    const int32_t G = a.G;
    const int32_t g0 = (int32_t)blockIdx.y * CNVSUM_CHUNK_GENES;
    const int32_t g1 = g0 + CNVSUM_CHUNK_GENES < G ? g0 + CNVSUM_CHUNK_GENES : G;
    const int32_t *__restrict__ cs = a.chr_start;
    const uint32_t s0 = (uint32_t)a.neutral, S0 = s0 * B01, S0M1 = (s0 ? s0 - 1u : 0u) * B01;
    const uint32_t FILL = s0 ? S0 : B01;               // what a masked-out byte counts as: the neutral state, or (neutral = 0) any valid one
    const uint32_t CK = (uint32_t)(0x80 - a.K) * B01;
    const bool validate = a.K > 0;

    int c = 0;
    while (cs[c + 1] <= g0) ++c;                       // g0 < G = cs[n_chr]
    uint32_t prev = 0;
    if (live && g0 > cs[c]) prev = a.st[col * a.ld + g0 - 1];
    uint32_t sad = 0, sum = 0, nle = 0, nlt = 0, bad = 0, runs_all = 0, runs_nn = 0;
    int32_t ndw = 0;

    auto step = [&](uint32_t w, uint32_t m, uint32_t force) {
        const uint32_t pw = (w << 8) | prev;
        prev = w >> 24;
        const uint32_t chg = (nz_bytes(w ^ pw) | force) & m & B80;
        const uint32_t wm = (w & m) | (FILL & ~m);
        if (validate) {
            const uint32_t t = wm - B01;               // a zero byte becomes 0xFF (a borrow only ever follows one)
            bad |= (t & 0xF8F8F8F8u) | ((t + CK) & B80);
        }
        if (FEAT) {
            sad = __builtin_amdgcn_sad_u8(wm, S0, sad);
            sum = __builtin_amdgcn_sad_u8(wm, 0u, sum);
            nle += __builtin_popcount(((S0 | B80) - wm) & B80);
            nlt += __builtin_popcount(((S0M1 | B80) - wm) & B80);          // s0 >= 1 here: #{s <= s0 - 1}
        }
        runs_all += __builtin_popcount(chg);
        runs_nn += __builtin_popcount(chg & nz_bytes(wm ^ S0));
        ++ndw;
    };
    auto flush = [&](int chr, bool whole) {
        if (FEAT && ndw > 0) {
            const int32_t n = 4 * ndw, diff = (int32_t)sum - n * (int32_t)s0;
            const int32_t nl = (int32_t)nlt, ng = n - (int32_t)nle;
            const int32_t dg = ((int32_t)sad + diff) / 2, dl = ((int32_t)sad - diff) / 2;
            if (live && (nl | ng)) {
                int32_t *o = a.counts + ((int64_t)chr * a.C + col) * 4;
                if (whole) {
                    *reinterpret_cast<int4 *>(o) = make_int4(nl, ng, dl, dg);
                } else {
                    if (nl) { atomicAdd(o + 0, nl); atomicAdd(o + 2, dl); }
                    if (ng) { atomicAdd(o + 1, ng); atomicAdd(o + 3, dg); }
                }
            }
        }
        sad = sum = nle = nlt = 0;
        ndw = 0;
    };

    for (int32_t t0 = g0; t0 < g1; t0 += TG) {
        __syncthreads();
        stage_tile(a.st, a.ld, G, a.C, col0, nullptr, t0, lds, aligned != 0);
        __syncthreads();
        const uint32_t *row = lds + lane * PITCH;
        const int32_t t1 = t0 + TG < g1 ? t0 + TG : g1;
        int32_t p = t0;
        while (p < t1) {
            while (cs[c + 1] <= p) ++c;                // also steps over empty chromosomes
            const int32_t e = cs[c + 1] < t1 ? cs[c + 1] : t1;
            if (cs[c + 1] - cs[c] < 2) {               // a one-gene chromosome is never reported: validated, not counted
                if (validate) {
                    const uint32_t b = (row[(p - t0) >> 2] >> (8 * ((p - t0) & 3))) & 0xFFu;
                    bad |= (b - 1u >= (uint32_t)a.K) ? 1u : 0u;
                }
            } else {
                const int d_first = (p - t0) >> 2, d_last = (e - 1 - t0) >> 2;
                int d = d_first;
                {   // the first word: the segment may begin inside it, and a chromosome's first gene always begins a run
                    const int lo = (p - t0) & 3;
                    const int hi = d == d_last ? e - t0 - 4 * d : 4;
                    step(row[d], byte_mask(lo, hi), p == cs[c] ? 0x80u << (8 * lo) : 0u);
                    ++d;
                }
                const int d_full = ((e - t0) & 3) ? d_last : d_last + 1;   // words d .. d_full - 1 are whole
                for (; d < d_full; ++d) step(row[d], 0xFFFFFFFFu, 0u);
                if (d <= d_last) step(row[d], byte_mask(0, e - t0 - 4 * d), 0u);
            }
            p = e;
            if (e == cs[c + 1]) flush(c, cs[c] >= g0);
        }
    }
    if (ndw > 0) flush(c, false);                      // the chunk ends inside chromosome c
    if (live) {
        if (a.neutral == 0) runs_nn = runs_all;
        if (runs_all) atomicAdd(a.run_counts + col * 2, (int32_t)runs_all);
        if (runs_nn) atomicAdd(a.run_counts + col * 2 + 1, (int32_t)runs_nn);
        if (bad) atomicOr(a.bad, 1);
    }
}

// One workgroup of 1024 threads: thread t sums its slice of the list, thread 0 scans the 1024 sums, every thread writes its slice.
__global__ __launch_bounds__(1024) void cnvsum_scan_kernel(const int32_t *__restrict__ run_counts, const int32_t *__restrict__ col_idx,
                                                           int64_t n, int64_t *__restrict__ rec_off, int64_t *__restrict__ ord_off,
                                                           int64_t *__restrict__ totals) {
    __shared__ int64_t part[2][1024];
    const int t = threadIdx.x;
    const int64_t per = (n + 1023) / 1024;
    const int64_t lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    int64_t sa = 0, sn = 0;
    for (int64_t i = lo; i < hi; ++i) {
        const int64_t col = col_idx ? (int64_t)col_idx[i] : i;
        sa += run_counts[col * 2];
        sn += run_counts[col * 2 + 1];
    }
    part[0][t] = sa;
    part[1][t] = sn;
    __syncthreads();
    if (t == 0) {
        int64_t ra = 0, rn = 0;
        for (int k = 0; k < 1024; ++k) {
            const int64_t va = part[0][k], vn = part[1][k];
            part[0][k] = ra;
            part[1][k] = rn;
            ra += va;
            rn += vn;
        }
        totals[0] = rn;
        totals[1] = ra;
    }
    __syncthreads();
    sa = part[0][t];
    sn = part[1][t];
    for (int64_t i = lo; i < hi; ++i) {
        const int64_t col = col_idx ? (int64_t)col_idx[i] : i;
        ord_off[i] = sa;
        rec_off[i] = sn;
        sa += run_counts[col * 2];
        sn += run_counts[col * 2 + 1];
    }
}

// The segmentation pass.  Workgroup = one wavefront = 64 list positions x every gene; a lane writes the records of its column
// from rec_off on.  Words without a change of state (nearly all of them) cost the compare alone.  Unlike the counting pass
// it is not chunked in genes (columns / 64 wavefronts in all): a chunk's record offset would need run counts per (column,
// chunk), which the scan does not produce -- DESIGN.md section 4 K14.
__global__ __launch_bounds__(64) void cnvsum_runs_kernel(CnvRunsArgs a, int aligned) {
    __shared__ uint32_t lds[64 * PITCH];
    const int lane = threadIdx.x;
    const int64_t pos0 = (int64_t)blockIdx.x * 64, pos = pos0 + lane;
    const bool live = pos < a.n_cols;
    const int32_t G = a.G;
    const int32_t *__restrict__ cs = a.chr_start;
    int64_t r = live ? a.rec_off[pos] : 0, ord = live ? a.ord_off[pos] : 0, open = -1;
    const int64_t cap = a.capacity;
    int32_t *const f_col = a.rec, *const f_chr = a.rec + cap, *const f_first = a.rec + 2 * cap, *const f_last = a.rec + 3 * cap,
                  *const f_state = a.rec + 4 * cap, *const f_ord = a.rec + 5 * cap;
    uint32_t prev = 0;
    int c = 0;
    for (int32_t t0 = 0; t0 < G; t0 += TG) {
        __syncthreads();
        stage_tile(a.st, a.ld, G, a.n_cols, pos0, a.col_idx, t0, lds, aligned != 0);
        __syncthreads();
        const uint32_t *row = lds + lane * PITCH;
        const int32_t t1 = t0 + TG < G ? t0 + TG : G;
        int32_t p = t0;
        while (p < t1) {
            while (cs[c + 1] <= p) ++c;
            const int32_t e = cs[c + 1] < t1 ? cs[c + 1] : t1;
            if (cs[c + 1] - cs[c] >= 2) {
                const int d_last = (e - 1 - t0) >> 2;
                for (int d = (p - t0) >> 2; d <= d_last; ++d) {
                    const int32_t gw = t0 + 4 * d;                 // gene of the word's first byte
                    const int lo = p > gw ? p - gw : 0, hi = e - gw < 4 ? e - gw : 4;
                    const uint32_t w = row[d];
                    const uint32_t pw = (w << 8) | prev;
                    prev = w >> 24;
                    const uint32_t force = (gw + lo == cs[c]) ? 0x80u << (8 * lo) : 0u;
                    const uint32_t chg = (nz_bytes(w ^ pw) | force) & byte_mask(lo, hi) & B80;
                    if (chg && live) {
                        for (int k = lo; k < hi; ++k) {
                            if (!((chg >> (8 * k + 7)) & 1u)) continue;
                            const int32_t g = gw + k;
                            const int32_t b = (int32_t)((w >> (8 * k)) & 0xFFu);
                            if (open >= 0) f_last[open] = g - 1;
                            open = -1;
                            ++ord;
                            if (a.neutral == 0 || b != a.neutral) {
                                if (r < cap) {
                                    f_col[r] = (int32_t)pos;
                                    f_chr[r] = c;
                                    f_first[r] = g;
                                    f_state[r] = b;
                                    f_ord[r] = (int32_t)ord;
                                    open = r;
                                }
                                ++r;
                            }
                        }
                    }
                }
            }
            p = e;
            if (e == cs[c + 1]) {
                if (open >= 0) f_last[open] = e - 1;
                open = -1;
            }
        }
    }
}

bool aligned16(const uint8_t *st, int64_t ld) { return (reinterpret_cast<uintptr_t>(st) & 15u) == 0 && (ld & 15) == 0; }

}  // namespace

int launch_cnvsum_count(const CnvSumArgs &a, hipStream_t stream) {
    if (a.C <= 0) return ICNV_OK;
    ICNV_HIP(hipMemsetAsync(a.run_counts, 0, (size_t)a.C * 2 * sizeof(int32_t), stream));
    ICNV_HIP(hipMemsetAsync(a.bad, 0, sizeof(int32_t), stream));
    if (a.counts) ICNV_HIP(hipMemsetAsync(a.counts, 0, (size_t)a.n_chr * (size_t)a.C * 4 * sizeof(int32_t), stream));
    const int64_t bx = (a.C + 63) / 64;
    const int by = (a.G + CNVSUM_CHUNK_GENES - 1) / CNVSUM_CHUNK_GENES;
    if (bx > 0x7fffffff || by > 65535) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "cnv_features: matrix too large for one launch");
    const int al = aligned16(a.st, a.ld) ? 1 : 0;
    if (a.counts) {
        KernelTimer kt("cnvsum_features", stream);
        hipLaunchKernelGGL(cnvsum_count_kernel<true>, dim3((unsigned)bx, (unsigned)by), dim3(64), 0, stream, a, al);
    } else {
        KernelTimer kt("cnvsum_run_counts", stream);
        hipLaunchKernelGGL(cnvsum_count_kernel<false>, dim3((unsigned)bx, (unsigned)by), dim3(64), 0, stream, a, al);
    }
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_cnvsum_scan(const int32_t *run_counts, const int32_t *col_idx, int64_t n_cols, int64_t *rec_off, int64_t *ord_off,
                       int64_t *totals, hipStream_t stream) {
    KernelTimer kt("cnvsum_scan", stream);
    hipLaunchKernelGGL(cnvsum_scan_kernel, dim3(1), dim3(1024), 0, stream, run_counts, col_idx, n_cols, rec_off, ord_off, totals);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_cnvsum_runs(const CnvRunsArgs &a, hipStream_t stream) {
    if (a.n_cols <= 0) return ICNV_OK;
    const int64_t bx = (a.n_cols + 63) / 64;
    if (bx > 0x7fffffff) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "cnv_runs: too many columns for one launch");
    KernelTimer kt("cnvsum_runs", stream);
    hipLaunchKernelGGL(cnvsum_runs_kernel, dim3((unsigned)bx), dim3(64), 0, stream, a, aligned16(a.st, a.ld) ? 1 : 0);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

}  // namespace icnv
