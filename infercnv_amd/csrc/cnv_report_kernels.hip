// Kernels of K24 (include/icnv.h "CNV region reports"): the text of <prefix>.pred_cnv_genes.dat and .pred_cnv_regions.dat from
// the run records of icnv_cnv_runs_dev.  No pass runs over the lines: the length of a line is a closed form of its record and
// of a per-gene prefix sum, so a record's bytes and the first byte of each of its lines are known from three loads.
// DESIGN.md section 4 K24.
#include "cnv_report_internal.h"
#include "icnv_internal.h"

namespace icnv {
namespace {

// ---- prefix sums ----------------------------------------------------------------------------------------------------------
// One workgroup: a lane sums a contiguous piece, the pieces are scanned in LDS, the lane writes its running sums.
__device__ inline int64_t cr_block_exclusive(int64_t mine, int64_t *s_scan) {
    const int tid = threadIdx.x;
    __syncthreads();                                           // the previous use of s_scan is over
    s_scan[tid] = mine;
    __syncthreads();
    for (int d = 1; d < CR_SCAN_NT; d <<= 1) {
        const int64_t add = tid >= d ? s_scan[tid - d] : 0;
        __syncthreads();
        s_scan[tid] += add;
        __syncthreads();
    }
    return s_scan[tid] - mine;
}

__device__ inline int64_t cr_gene_bytes(const CrArgs &a, int64_t g) {
    return a.gene_off[g + 1] - a.gene_off[g] + cr_int_len(a.gstart[g]) + cr_int_len(a.gend[g]);
}

__global__ __launch_bounds__(CR_SCAN_NT) void cr_gene_prefix_kernel(CrArgs a) {
    __shared__ int64_t s_scan[CR_SCAN_NT];
    const int64_t piece = (a.G + CR_SCAN_NT - 1) / CR_SCAN_NT, lo = (int64_t)threadIdx.x * piece;
    const int64_t hi = lo + piece < a.G ? lo + piece : a.G;
    int64_t sum = 0;
    for (int64_t g = lo; g < hi; ++g) sum += cr_gene_bytes(a, g);
    int64_t run = cr_block_exclusive(sum, s_scan);
    for (int64_t g = lo; g < hi; ++g) {
        run += cr_gene_bytes(a, g);
        a.P[g + 1] = run;
    }
    if (threadIdx.x == 0) a.P[0] = 0;
}

// in place: x[0] = 0, x[i + 1] = sum of the x[1 .. i + 1] it held
__global__ __launch_bounds__(CR_SCAN_NT) void cr_scan_kernel(int64_t *x0, int64_t *x1, int64_t n) {
    __shared__ int64_t s_scan[CR_SCAN_NT];
    const int64_t piece = (n + CR_SCAN_NT - 1) / CR_SCAN_NT, lo = (int64_t)threadIdx.x * piece;
    const int64_t hi = lo + piece < n ? lo + piece : n;
    for (int k = 0; k < 2; ++k) {
        int64_t *x = k == 0 ? x0 : x1;
        if (!x) continue;                                      // uniform
        int64_t sum = 0;
        for (int64_t i = lo; i < hi; ++i) sum += x[i + 1];
        int64_t run = cr_block_exclusive(sum, s_scan);
        for (int64_t i = lo; i < hi; ++i) {
            run += x[i + 1];
            x[i + 1] = run;
        }
        if (threadIdx.x == 0) x[0] = 0;
    }
}

// ---- record lengths -------------------------------------------------------------------------------------------------------
// F_r of the contract: the bytes of a line that do not depend on the gene (GENES), all but the two positions (REGIONS)
__device__ inline int64_t cr_fixed(const CrArgs &a, int64_t r) {
    const int64_t q = a.col[r], c = a.chr[r];
    return (a.grp_off[q + 1] - a.grp_off[q]) + 2 * (a.chr_off[c + 1] - a.chr_off[c]) + 8 + cr_int_len(a.ordinal[r]) +
           cr_int_len(cr_state_value(a.state[r])) + (a.kind == CR_GENES ? 7 : 6);
}

__global__ __launch_bounds__(CR_NT) void cr_lengths_kernel(CrArgs a) {
    const int64_t r = (int64_t)blockIdx.x * CR_NT + threadIdx.x;
    if (r >= a.n_rec) return;
    const int64_t first = a.first[r], last = a.last[r], F = cr_fixed(a, r);
    if (a.kind == CR_GENES) {
        a.rec_off[r + 1] = (last - first + 1) * F + a.P[last + 1] - a.P[first];
        a.line_base[r + 1] = last - first + 1;
    } else {
        int64_t lo = a.gstart[first], hi = a.gend[first];
        for (int64_t g = first + 1; g <= last; ++g) {
            lo = a.gstart[g] < lo ? a.gstart[g] : lo;
            hi = a.gend[g] > hi ? a.gend[g] : hi;
        }
        a.rmin[r] = lo;
        a.rmax[r] = hi;
        a.rec_off[r + 1] = F + cr_int_len(lo) + cr_int_len(hi);
    }
}

// ---- emit -----------------------------------------------------------------------------------------------------------------
// A workgroup owns CR_TILE bytes of the output, cut at the 16-byte words of `out`'s address.  It finds the first and the last
// line that overlap its bytes from the record offsets, the line counts and the closed form above; a lane takes every
// CR_NT-th of those lines and writes the part of it that lies inside the tile into LDS.  The lines cover the tile without a
// gap, so every byte of the tile is written once; whole words then leave as 16-byte stores, the ragged ends of the chunk
// byte by byte.  A line may begin before the tile, end after it, or both (a line longer than a tile).
struct CrCursor {
    uint8_t *lds;         // lds[0] is the body's byte `org`
    int64_t org, lo, hi;  // the tile's bytes are [lo, hi)
    int64_t pos;          // the next byte of the line
};

__device__ inline void cr_put_bytes(CrCursor &o, const uint8_t *src, int64_t len) {
    const int64_t b0 = o.pos > o.lo ? o.pos : o.lo, b1 = o.pos + len < o.hi ? o.pos + len : o.hi;
    for (int64_t q = b0; q < b1; ++q) o.lds[q - o.org] = src[q - o.pos];
    o.pos += len;
}

__device__ inline void cr_put_char(CrCursor &o, uint8_t c) {
    if (o.pos >= o.lo && o.pos < o.hi) o.lds[o.pos - o.org] = c;
    o.pos += 1;
}

__device__ inline void cr_put_int(CrCursor &o, int64_t v) {
    const int len = cr_int_len(v);
    if (o.pos + len > o.lo && o.pos < o.hi) {
        uint64_t m = v < 0 ? 0 - (uint64_t)v : (uint64_t)v;
        const int n_digits = len - (v < 0 ? 1 : 0);
        int64_t q = o.pos + len - 1;
        for (int k = 0; k < n_digits; ++k, --q) {              // last digit first
            if (q >= o.lo && q < o.hi) o.lds[q - o.org] = (uint8_t)('0' + (int)(m % 10));
            m /= 10;
        }
        if (v < 0 && o.pos >= o.lo) o.lds[o.pos - o.org] = (uint8_t)'-';
    }
    o.pos += len;
}

__device__ inline void cr_put_name(CrCursor &o, const uint8_t *bytes, const int64_t *off, int64_t i) {
    cr_put_bytes(o, bytes + off[i], off[i + 1] - off[i]);
}

// the offset of line i of GENES record r within the record
__device__ inline int64_t cr_line_start(const CrArgs &a, int64_t first, int64_t F, int64_t i) {
    return i * F + a.P[first + i] - a.P[first];
}

// the global line that holds byte x of the body, which lies in record r
__device__ inline int64_t cr_line_at(const CrArgs &a, int64_t r, int64_t x) {
    if (a.kind != CR_GENES) return r;
    const int64_t first = a.first[r], F = cr_fixed(a, r), within = x - a.rec_off[r];
    int64_t lo = 0, hi = a.last[r] - first;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (cr_line_start(a, first, F, mid) <= within) lo = mid;
        else hi = mid - 1;
    }
    return a.line_base[r] + lo;
}

// the largest i in [lo, hi] with x[i] <= v (x ascending, x[lo] <= v)
__device__ inline int64_t cr_last_le(const int64_t *x, int64_t lo, int64_t hi, int64_t v) {
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (x[mid] <= v) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(CR_NT) void cr_emit_kernel(CrArgs a, int64_t rec0, int64_t rec1, int64_t base, int64_t n_bytes, uint8_t *out) {
    __shared__ uint4 s_txt4[CR_TILE / 16];
    __shared__ int64_t s_span[4];                              // first record, last record, first line, last line of the tile
    uint8_t *s_txt = reinterpret_cast<uint8_t *>(s_txt4);
    const int tid = threadIdx.x;
    const int64_t shift = (int64_t)(reinterpret_cast<uintptr_t>(out) & 15);
    const int64_t t0 = (int64_t)blockIdx.x * CR_TILE - shift;  // chunk position of s_txt[0]: out + t0 is 16-byte aligned
    const int64_t c_lo = t0 > 0 ? t0 : 0, c_hi = t0 + CR_TILE < n_bytes ? t0 + CR_TILE : n_bytes;
    if (c_lo >= c_hi) return;                                  // uniform
    CrCursor o{s_txt, base + t0, base + c_lo, base + c_hi, 0};
    if (tid == 0) {
        const int64_t r_lo = cr_last_le(a.rec_off, rec0, rec1 - 1, o.lo), r_hi = cr_last_le(a.rec_off, r_lo, rec1 - 1, o.hi - 1);
        s_span[0] = r_lo;
        s_span[1] = r_hi;
        s_span[2] = cr_line_at(a, r_lo, o.lo);
        s_span[3] = cr_line_at(a, r_hi, o.hi - 1);
    }
    __syncthreads();
    const int64_t r_lo = s_span[0], r_hi = s_span[1], l_hi = s_span[3];
    for (int64_t l = s_span[2] + tid; l <= l_hi; l += CR_NT) {
        const int64_t r = a.kind == CR_GENES ? cr_last_le(a.line_base, r_lo, r_hi, l) : l;
        const int64_t q = a.col[r], c = a.chr[r], first = a.first[r];
        if (a.kind == CR_GENES) {
            const int64_t i = l - a.line_base[r], g = first + i;
            o.pos = a.rec_off[r] + cr_line_start(a, first, cr_fixed(a, r), i);
            cr_put_name(o, a.grp_b, a.grp_off, q);
            cr_put_char(o, '\t');
            cr_put_name(o, a.chr_b, a.chr_off, c);
            cr_put_bytes(o, reinterpret_cast<const uint8_t *>("-region_"), 8);
            cr_put_int(o, a.ordinal[r]);
            cr_put_char(o, '\t');
            cr_put_int(o, cr_state_value(a.state[r]));
            cr_put_char(o, '\t');
            cr_put_name(o, a.gene_b, a.gene_off, g);
            cr_put_char(o, '\t');
            cr_put_name(o, a.chr_b, a.chr_off, c);
            cr_put_char(o, '\t');
            cr_put_int(o, a.gstart[g]);
            cr_put_char(o, '\t');
            cr_put_int(o, a.gend[g]);
            cr_put_char(o, '\n');
        } else {
            o.pos = a.rec_off[r];
            cr_put_name(o, a.grp_b, a.grp_off, q);
            cr_put_char(o, '\t');
            cr_put_name(o, a.chr_b, a.chr_off, c);
            cr_put_bytes(o, reinterpret_cast<const uint8_t *>("-region_"), 8);
            cr_put_int(o, a.ordinal[r]);
            cr_put_char(o, '\t');
            cr_put_int(o, cr_state_value(a.state[r]));
            cr_put_char(o, '\t');
            cr_put_name(o, a.chr_b, a.chr_off, c);
            cr_put_char(o, '\t');
            cr_put_int(o, a.rmin[r]);
            cr_put_char(o, '\t');
            cr_put_int(o, a.rmax[r]);
            cr_put_char(o, '\n');
        }
    }
    __syncthreads();
    uint8_t *word0 = out + t0;                                 // 16-byte aligned; bytes before out[c_lo] are never touched
    for (int w = tid; w < CR_TILE / 16; w += CR_NT) {
        const int64_t p0 = t0 + (int64_t)w * 16, p1 = p0 + 16;
        if (p0 >= c_lo && p1 <= c_hi) reinterpret_cast<uint4 *>(word0)[w] = s_txt4[w];
        else
            for (int64_t p = p0 > c_lo ? p0 : c_lo; p < (p1 < c_hi ? p1 : c_hi); ++p) out[p] = s_txt[p - t0];
    }
}

}  // namespace

int launch_cr_gene_prefix(const CrArgs &a, hipStream_t s) {
    KernelTimer kt("cnv_report_prefix", s);
    hipLaunchKernelGGL(cr_gene_prefix_kernel, dim3(1), dim3(CR_SCAN_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_cr_lengths(const CrArgs &a, hipStream_t s) {
    const int64_t blocks = (a.n_rec + CR_NT - 1) / CR_NT;
    if (blocks < 1 || blocks > 0x7fffffff) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "cnv_report: the records need more than 2^31 - 1 workgroups");
    {
        KernelTimer kt("cnv_report_lengths", s);
        hipLaunchKernelGGL(cr_lengths_kernel, dim3((unsigned)blocks), dim3(CR_NT), 0, s, a);
        ICNV_HIP(hipGetLastError());
    }
    KernelTimer kt("cnv_report_scan", s);
    hipLaunchKernelGGL(cr_scan_kernel, dim3(1), dim3(CR_SCAN_NT), 0, s, a.rec_off, a.kind == CR_GENES ? a.line_base : nullptr, a.n_rec);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_cr_emit(const CrArgs &a, int64_t rec0, int64_t rec1, int64_t base, int64_t n_bytes, uint8_t *out, hipStream_t s) {
    KernelTimer kt("cnv_report_emit", s);
    const int64_t shift = (int64_t)(reinterpret_cast<uintptr_t>(out) & 15), blocks = (n_bytes + shift + CR_TILE - 1) / CR_TILE;
    if (blocks < 1 || blocks > 0x7fffffff) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "cnv_report: the chunk needs more than 2^31 - 1 workgroups");
    hipLaunchKernelGGL(cr_emit_kernel, dim3((unsigned)blocks), dim3(CR_NT), 0, s, a, rec0, rec1, base, n_bytes, out);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

}  // namespace icnv
