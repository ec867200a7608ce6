// C ABI of K34 (include/icnv.h "K34: count matrices out of R's serialisation stream"): everything that can be refused is refused
// before a launch -- the device lists (col_off, col_kind, cells) are fetched for it --, then the kernels of
// rds_counts_kernels.hip.  DESIGN.md section 4 K34.
#include <atomic>

#include "icnv_internal.h"
#include "rds_counts_internal.h"

using namespace icnv;

namespace {

// calls of columns, columns, elements, calls of check, entries examined, refused checks, calls of fill, entries written
std::atomic<int64_t> g_rds_stats[8];

constexpr int64_t RC_MAX = 0x7fffffff;

// does the payload of n elements of es bytes at byte off lie inside a stream of stream_bytes bytes?
bool rc_inside(int64_t off, int64_t n, int64_t es, int64_t stream_bytes) {
    return off >= 0 && n >= 0 && off <= stream_bytes && n <= (stream_bytes - off) / es;
}

int rc_csc_args(const char *who, const uint8_t *stream, int64_t stream_bytes, int64_t i_off, int64_t p_off, int64_t x_off, int64_t G,
                int64_t C, int64_t nnz, const int32_t *cells, int64_t n_out, hipStream_t s) {
    const std::string w(who);
    if (!stream) ICNV_FAIL(ICNV_ERR_ARG, w + ": null argument");
    if (G < 1 || C < 1 || G > RC_MAX || C >= RC_MAX) ICNV_FAIL(ICNV_ERR_ARG, w + ": G and C must be 1 .. 2^31 - 1");
    if (nnz < 0 || nnz > RC_MAX) ICNV_FAIL(ICNV_ERR_ARG, w + ": nnz must be 0 .. 2^31 - 1");
    if (stream_bytes < 0 || !rc_inside(i_off, nnz, 4, stream_bytes) || !rc_inside(p_off, C + 1, 4, stream_bytes) ||
        !rc_inside(x_off, nnz, 8, stream_bytes))
        ICNV_FAIL(ICNV_ERR_ARG, w + ": a payload does not lie inside the stream");
    if (n_out < 1 || n_out >= RC_MAX || (!cells && n_out != C)) ICNV_FAIL(ICNV_ERR_ARG, w + ": n_out must be the number of listed columns, or C without a list");
    if (cells) {
        std::vector<int32_t> h((size_t)n_out);
        ICNV_HIP(hipMemcpyAsync(h.data(), cells, (size_t)n_out * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        ICNV_HIP(hipStreamSynchronize(s));
        for (int64_t k = 0; k < n_out; ++k)
            if (h[(size_t)k] < 0 || h[(size_t)k] >= C)
                ICNV_FAIL(ICNV_ERR_ARG, w + ": cells[" + std::to_string(k) + "] = " + std::to_string(h[(size_t)k]) + " is no column of " + std::to_string(C));
    }
    return ICNV_OK;
}

}  // namespace

extern "C" {

int icnv_rds_columns_dev(const uint8_t *stream, int64_t stream_bytes, const int64_t *col_off, const int32_t *col_kind, int64_t n_out,
                         int64_t rows, double *out, int64_t ld, void *hip_stream) {
    hipStream_t s = (hipStream_t)hip_stream;
    if (!stream || !col_off || !col_kind || !out) ICNV_FAIL(ICNV_ERR_ARG, "rds_columns: null argument");
    if (n_out < 1 || rows < 1 || ld < rows || stream_bytes < 0 || n_out > ((int64_t)1 << 59) / ld)
        ICNV_FAIL(ICNV_ERR_ARG, "rds_columns: n_out and rows must be at least 1, ld at least rows, and the output below 2^59 elements");
    std::vector<int64_t> h_off((size_t)n_out);
    std::vector<int32_t> h_kind((size_t)n_out);
    ICNV_HIP(hipMemcpyAsync(h_off.data(), col_off, (size_t)n_out * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipMemcpyAsync(h_kind.data(), col_kind, (size_t)n_out * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    for (int64_t j = 0; j < n_out; ++j) {
        const int32_t kind = h_kind[(size_t)j];
        if (kind != ICNV_RDS_REAL && kind != ICNV_RDS_INT)
            ICNV_FAIL(ICNV_ERR_ARG, "rds_columns: col_kind[" + std::to_string(j) + "] = " + std::to_string(kind) + " is neither ICNV_RDS_REAL nor ICNV_RDS_INT");
        if (!rc_inside(h_off[(size_t)j], rows, kind == ICNV_RDS_REAL ? 8 : 4, stream_bytes))
            ICNV_FAIL(ICNV_ERR_ARG, "rds_columns: column " + std::to_string(j) + " at byte " + std::to_string(h_off[(size_t)j]) + " does not lie inside the stream of " +
                                        std::to_string(stream_bytes) + " bytes");
    }
    RdsColumnsArgs a{stream, stream_bytes, col_off, col_kind, n_out, rows, ld, reinterpret_cast<uint64_t *>(out)};
    int rc;
    if ((rc = launch_rds_columns(a, s))) return rc;
    g_rds_stats[0] += 1;
    g_rds_stats[1] += n_out;
    g_rds_stats[2] += n_out * rows;
    return ICNV_OK;
}

int icnv_rds_csc_check_dev(const uint8_t *stream, int64_t stream_bytes, int64_t i_off, int64_t p_off, int64_t x_off, int64_t G, int64_t C,
                           int64_t nnz, const int32_t *cells, int64_t n_out, int64_t *colptr, int64_t *status, int64_t *nnz_out,
                           void *hip_stream) {
    hipStream_t s = (hipStream_t)hip_stream;
    int rc;
    if (!colptr || !status || !nnz_out) ICNV_FAIL(ICNV_ERR_ARG, "rds_csc_check: null argument");
    if ((rc = rc_csc_args("rds_csc_check", stream, stream_bytes, i_off, p_off, x_off, G, C, nnz, cells, n_out, s))) return rc;
    DevBuf d_key;                                                        // the key word, then the column of an entry violation
    if ((rc = d_key.alloc(2 * sizeof(uint64_t)))) return rc;
    ICNV_HIP(hipMemsetAsync(d_key.p, 0xFF, sizeof(uint64_t), s));        // RC_NO_VIOLATION
    RdsCscArgs a{stream, stream_bytes, i_off, p_off, x_off, G, C, nnz, cells, n_out, d_key.as<unsigned long long>(), colptr, nullptr, nullptr, 0};
    if ((rc = launch_rds_csc_check(a, s))) return rc;
    uint64_t key = 0;
    ICNV_HIP(hipMemcpyAsync(&key, d_key.p, sizeof key, hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    g_rds_stats[3] += 1;
    if (key != RC_NO_VIOLATION) {
        const bool entry = (key & RC_ENTRY_PHASE) != 0;
        const int64_t index = (int64_t)((key & ~RC_ENTRY_PHASE) >> 3);
        int64_t column = index < C - 1 ? index : C - 1;
        if (entry) {                                                     // p passed: the column is a search in it
            if ((rc = launch_rds_csc_find_column(a, index, d_key.as<int64_t>() + 1, s))) return rc;
            ICNV_HIP(hipMemcpyAsync(&column, d_key.as<int64_t>() + 1, sizeof column, hipMemcpyDeviceToHost, s));
            ICNV_HIP(hipStreamSynchronize(s));
        }
        status[0] = (int64_t)(key & 7);
        status[1] = column;
        status[2] = index;
        g_rds_stats[5] += 1;
        return ICNV_OK;
    }
    if ((rc = launch_rds_csc_colptr(a, s))) return rc;
    ICNV_HIP(hipMemcpyAsync(nnz_out, colptr + n_out, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    status[0] = ICNV_RDS_OK;
    status[1] = status[2] = -1;
    g_rds_stats[4] += *nnz_out;
    return ICNV_OK;
}

int icnv_rds_csc_fill_dev(const uint8_t *stream, int64_t stream_bytes, int64_t i_off, int64_t p_off, int64_t x_off, int64_t G, int64_t C,
                          int64_t nnz, const int32_t *cells, int64_t n_out, const int64_t *colptr, int32_t *rowidx, int32_t *vals,
                          int64_t out_nnz, void *hip_stream) {
    hipStream_t s = (hipStream_t)hip_stream;
    int rc;
    if (!colptr || out_nnz < 0 || (out_nnz > 0 && (!rowidx || !vals))) ICNV_FAIL(ICNV_ERR_ARG, "rds_csc_fill: null argument or a negative out_nnz");
    if ((rc = rc_csc_args("rds_csc_fill", stream, stream_bytes, i_off, p_off, x_off, G, C, nnz, cells, n_out, s))) return rc;
    g_rds_stats[6] += 1;
    if (out_nnz == 0) return ICNV_OK;
    RdsCscArgs a{stream, stream_bytes, i_off, p_off, x_off, G, C, nnz, cells, n_out, nullptr, const_cast<int64_t *>(colptr), rowidx, vals, out_nnz};
    if ((rc = launch_rds_csc_fill(a, s))) return rc;
    ICNV_HIP(hipStreamSynchronize(s));
    g_rds_stats[7] += out_nnz;
    return ICNV_OK;
}

int icnv_rds_counts_stats(int64_t *out, int32_t n) {
    if (!out || n < 1) ICNV_FAIL(ICNV_ERR_ARG, "bad argument");
    for (int i = 0; i < n && i < 8; ++i) out[i] = g_rds_stats[i].load();
    return ICNV_OK;
}

void icnv_rds_counts_stats_reset(void) {
    for (auto &c : g_rds_stats) c.store(0);
}

}  // extern "C"
