// C ABI of K29 (include/icnv.h "INFLATE in independent units"): everything that can be refused is refused before the kernels that
// read or write the caller's buffers.  Kernels: inflate_kernels.hip.  DESIGN.md section 4 K29.
#include "icnv_internal.h"
#include "inflate_internal.h"
#include "../../include/icnv.h"

using namespace icnv;

namespace {

// start (and, for the decode, end / out_off / out_len) of every unit against n and out_cap: one small kernel, one word back
int check_units(const InflateArgs &a, bool units, const char *who, hipStream_t s) {
    return check_on_device([&](int32_t *bad, hipStream_t st) { return launch_inflate_check(a, units, bad, st); },
                           [&] {
                               return std::string(who) + (units ? ": a unit's start is outside [0, n), its end outside [start, n], or its output range outside [0, out_cap]"
                                                                : ": a unit's start is outside [0, n)");
                           },
                           s);
}

}  // namespace

extern "C" {

int icnv_inflate_scan_dev(const uint8_t *src, int64_t n, int64_t *cand, int64_t cand_cap, int64_t *n_cand, void *stream) {
    if (!n_cand) ICNV_FAIL(ICNV_ERR_ARG, "inflate_scan: null n_cand");
    *n_cand = 0;
    if (n < 0 || cand_cap < 0) ICNV_FAIL(ICNV_ERR_ARG, "inflate_scan: negative size");
    if (n < 4) return ICNV_OK;                                      // no room for a marker
    if (!src || (cand_cap > 0 && !cand)) ICNV_FAIL(ICNV_ERR_ARG, "inflate_scan: null argument");
    if (misaligned(cand, 8)) ICNV_FAIL(ICNV_ERR_ARG, "inflate_scan: cand is not aligned to 8 bytes");
    const int64_t n_blocks = n / (SC_NT * SC_ROUNDS) + 1;           // positions 0 .. n
    if (n_blocks > 0x7fffffff) ICNV_FAIL(ICNV_ERR_ARG, "inflate_scan: the stream is beyond 2^43 bytes");
    hipStream_t s = (hipStream_t)stream;
    DevBuf offsets;
    int rc;
    if ((rc = offsets.alloc((size_t)(n_blocks + 1) * sizeof(int64_t)))) return rc;
    KernelTimer kt("inflate_scan", s);
    if ((rc = launch_inflate_scan_count(src, n, n_blocks, offsets.as<int64_t>(), s))) return rc;
    int64_t total = 0;
    ICNV_HIP(hipMemcpyAsync(&total, offsets.as<int64_t>() + n_blocks, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    *n_cand = total;
    if (total > cand_cap)                                           // before the emit pass: nothing has touched `cand`
        ICNV_FAIL(ICNV_ERR_ARG, "inflate_scan: cand_cap " + std::to_string(cand_cap) + " is below the number of candidates " + std::to_string(total));
    if (total == 0) return ICNV_OK;
    if ((rc = launch_inflate_scan_emit(src, n, n_blocks, offsets.as<int64_t>(), cand, cand_cap, s))) return rc;
    ICNV_HIP(hipStreamSynchronize(s));                              // the offsets go back to the pool: the emit pass has read them
    return ICNV_OK;
}

int icnv_inflate_measure_dev(const uint8_t *src, int64_t n, const int64_t *start, int64_t n_units, int64_t max_in, int64_t *end,
                             int64_t *out_len, int32_t *status, void *stream) {
    if (n < 0 || n_units < 0 || max_in < 0) ICNV_FAIL(ICNV_ERR_ARG, "inflate_measure: negative size");
    if (n_units == 0) return ICNV_OK;
    if (!src || !start || !end || !out_len || !status) ICNV_FAIL(ICNV_ERR_ARG, "inflate_measure: null argument");
    if (misaligned(start, 8) || misaligned(end, 8) || misaligned(out_len, 8) || misaligned(status, 4))
        ICNV_FAIL(ICNV_ERR_ARG, "inflate_measure: start / end / out_len must be aligned to 8 bytes, status to 4");
    if (n_units > (int64_t)0x7fffffff * IF_WAVES) ICNV_FAIL(ICNV_ERR_ARG, "inflate_measure: too many units");
    hipStream_t s = (hipStream_t)stream;
    InflateArgs a{src, n, start, n_units, max_in, end, out_len, nullptr, nullptr, 0, status};
    int rc;
    if ((rc = check_units(a, false, "inflate_measure", s))) return rc;
    return launch_inflate_measure(a, s);
}

int icnv_inflate_units_dev(const uint8_t *src, int64_t n, const int64_t *start, const int64_t *end, const int64_t *out_off,
                           const int64_t *out_len, int64_t n_units, uint8_t *out, int64_t out_cap, int32_t *status, void *stream) {
    if (n < 0 || n_units < 0 || out_cap < 0) ICNV_FAIL(ICNV_ERR_ARG, "inflate_units: negative size");
    if (n_units == 0) return ICNV_OK;
    if (!src || !start || !end || !out_off || !out_len || !status || (out_cap > 0 && !out)) ICNV_FAIL(ICNV_ERR_ARG, "inflate_units: null argument");
    if (misaligned(start, 8) || misaligned(end, 8) || misaligned(out_off, 8) || misaligned(out_len, 8) || misaligned(status, 4))
        ICNV_FAIL(ICNV_ERR_ARG, "inflate_units: start / end / out_off / out_len must be aligned to 8 bytes, status to 4");
    if (n_units > (int64_t)0x7fffffff * IF_WAVES) ICNV_FAIL(ICNV_ERR_ARG, "inflate_units: too many units");
    hipStream_t s = (hipStream_t)stream;
    InflateArgs a{src, n, start, n_units, 0, const_cast<int64_t *>(end), const_cast<int64_t *>(out_len), out_off, out, out_cap, status};
    int rc;
    if ((rc = check_units(a, true, "inflate_units", s))) return rc;
    return launch_inflate_units(a, s);
}

int icnv_crc32_pieces_dev(const uint8_t *src, int64_t n, int64_t piece_bytes, uint32_t *crc, void *stream) {
    if (n < 0) ICNV_FAIL(ICNV_ERR_ARG, "crc32_pieces: negative length");
    if (piece_bytes < 1) ICNV_FAIL(ICNV_ERR_ARG, "crc32_pieces: piece_bytes must be at least 1");
    if (n == 0) return ICNV_OK;
    if (!src || !crc) ICNV_FAIL(ICNV_ERR_ARG, "crc32_pieces: null argument");
    if (misaligned(crc, 4)) ICNV_FAIL(ICNV_ERR_ARG, "crc32_pieces: crc is not aligned to 4 bytes");
    const int64_t n_pieces = (n - 1) / piece_bytes + 1;
    return launch_crc32_pieces(src, n, piece_bytes, n_pieces, crc, (hipStream_t)stream);
}

}  // extern "C"
