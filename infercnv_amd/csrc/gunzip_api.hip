// C ABI of K30 (include/icnv.h "INFLATE with unknown history"): everything that can be refused is refused before the kernels
// that read or write the caller's buffers.  Kernels: gunzip_kernels.hip.  DESIGN.md section 4 K30.
#include "icnv_internal.h"
#include "gunzip_internal.h"
#include "../../include/icnv.h"

using namespace icnv;

namespace {

// the units' starts / ends / places against n and cap: one small kernel, one word back
int check_units(const GunzipArgs &a, int mode, const char *who, hipStream_t s) {
    return check_on_device([&](int32_t *bad, hipStream_t st) { return launch_gunzip_check(a, mode, bad, st); },
                           [&] {
                               return std::string(who) + (mode == GZ_CHECK_MEASURE   ? ": a unit's start is outside [0, 8 n)"
                                                          : mode == GZ_CHECK_SYMBOLS ? ": a unit's start is outside [0, 8 n), its end outside [start, 8 n], or the units' places are not the "
                                                                                       "prefix sums of out_len inside [0, sym_cap]"
                                                                                     : ": the units' places are not the prefix sums of out_len inside [0, out_cap]");
                           },
                           s);
}

}  // namespace

extern "C" {

int icnv_gunzip_find_dev(const uint8_t *src, int64_t n, int64_t *cand, int64_t cand_cap, int64_t *n_cand, void *stream) {
    if (!n_cand) ICNV_FAIL(ICNV_ERR_ARG, "gunzip_find: null n_cand");
    *n_cand = 0;
    if (n < 0 || cand_cap < 0) ICNV_FAIL(ICNV_ERR_ARG, "gunzip_find: negative size");
    if (n < 3) return ICNV_OK;                                      // no room for the 17 bits in front of the code lengths
    if (!src || (cand_cap > 0 && !cand)) ICNV_FAIL(ICNV_ERR_ARG, "gunzip_find: null argument");
    if (misaligned(cand, 8)) ICNV_FAIL(ICNV_ERR_ARG, "gunzip_find: cand is not aligned to 8 bytes");
    if (n > ((int64_t)1 << 32)) ICNV_FAIL(ICNV_ERR_ARG, "gunzip_find: the stream is beyond 2^32 bytes");   // 2^23 workgroups: the grid stays below 2^32 lanes
    const int64_t n_blocks = (n * 8 - 1) / (SC_NT * SC_ROUNDS) + 1;    // bit offsets 0 .. 8 n - 1
    hipStream_t s = (hipStream_t)stream;
    DevBuf offsets;
    int rc;
    if ((rc = offsets.alloc((size_t)(n_blocks + 1) * sizeof(int64_t)))) return rc;
    KernelTimer kt("gunzip_find", s);
    if ((rc = launch_gunzip_find_count(src, n, n_blocks, offsets.as<int64_t>(), s))) return rc;
    int64_t total = 0;
    ICNV_HIP(hipMemcpyAsync(&total, offsets.as<int64_t>() + n_blocks, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    *n_cand = total;
    if (total > cand_cap)                                           // before the emit pass: nothing has touched `cand`
        ICNV_FAIL(ICNV_ERR_ARG, "gunzip_find: cand_cap " + std::to_string(cand_cap) + " is below the number of candidates " + std::to_string(total));
    if (total == 0) return ICNV_OK;
    if ((rc = launch_gunzip_find_emit(src, n, n_blocks, offsets.as<int64_t>(), cand, cand_cap, s))) return rc;
    ICNV_HIP(hipStreamSynchronize(s));                              // the offsets go back to the pool: the emit pass has read them
    return ICNV_OK;
}

int icnv_gunzip_measure_dev(const uint8_t *src, int64_t n, const int64_t *cand, int64_t n_cand, const int64_t *start, int64_t n_units,
                            int64_t max_in, int64_t *end, int64_t *out_len, int32_t *status, void *stream) {
    if (n < 0 || n_cand < 0 || n_units < 0 || max_in < 0) ICNV_FAIL(ICNV_ERR_ARG, "gunzip_measure: negative size");
    if (n_units == 0) return ICNV_OK;
    if (!src || (n_cand > 0 && !cand) || !start || !end || !out_len || !status) ICNV_FAIL(ICNV_ERR_ARG, "gunzip_measure: null argument");
    if (misaligned(cand, 8) || misaligned(start, 8) || misaligned(end, 8) || misaligned(out_len, 8) || misaligned(status, 4))
        ICNV_FAIL(ICNV_ERR_ARG, "gunzip_measure: cand / start / end / out_len must be aligned to 8 bytes, status to 4");
    if (n > ((int64_t)1 << 40)) ICNV_FAIL(ICNV_ERR_ARG, "gunzip_measure: the stream is beyond 2^40 bytes");
    if (n_units > (int64_t)0x7fffffff * IF_WAVES) ICNV_FAIL(ICNV_ERR_ARG, "gunzip_measure: too many units");
    hipStream_t s = (hipStream_t)stream;
    GunzipArgs a{src, n, cand, n_cand, start, n_units, max_in, end, out_len, nullptr, nullptr, nullptr, 0, status};
    int rc;
    if ((rc = check_units(a, GZ_CHECK_MEASURE, "gunzip_measure", s))) return rc;
    return launch_gunzip_measure(a, s);
}

int icnv_gunzip_symbols_dev(const uint8_t *src, int64_t n, const int64_t *cand, int64_t n_cand, const int64_t *start, const int64_t *end,
                            const int64_t *out_off, const int64_t *out_len, int64_t n_units, uint16_t *sym, int64_t sym_cap, int32_t *status,
                            void *stream) {
    if (n < 0 || n_cand < 0 || n_units < 0 || sym_cap < 0) ICNV_FAIL(ICNV_ERR_ARG, "gunzip_symbols: negative size");
    if (n_units == 0) return ICNV_OK;
    if (!src || (n_cand > 0 && !cand) || !start || !end || !out_off || !out_len || !status || (sym_cap > 0 && !sym))
        ICNV_FAIL(ICNV_ERR_ARG, "gunzip_symbols: null argument");
    if (misaligned(cand, 8) || misaligned(start, 8) || misaligned(end, 8) || misaligned(out_off, 8) || misaligned(out_len, 8) ||
        misaligned(status, 4) || misaligned(sym, 2))
        ICNV_FAIL(ICNV_ERR_ARG, "gunzip_symbols: cand / start / end / out_off / out_len must be aligned to 8 bytes, status to 4, sym to 2");
    if (n > ((int64_t)1 << 40)) ICNV_FAIL(ICNV_ERR_ARG, "gunzip_symbols: the stream is beyond 2^40 bytes");
    if (n_units > (int64_t)0x7fffffff * IF_WAVES) ICNV_FAIL(ICNV_ERR_ARG, "gunzip_symbols: too many units");
    hipStream_t s = (hipStream_t)stream;
    GunzipArgs a{src, n, cand, n_cand, start, n_units, 0, const_cast<int64_t *>(end), const_cast<int64_t *>(out_len), out_off, sym, nullptr, sym_cap, status};
    int rc;
    if ((rc = check_units(a, GZ_CHECK_SYMBOLS, "gunzip_symbols", s))) return rc;
    return launch_gunzip_symbols(a, s);
}

namespace {
int places_args(const char *who, const uint16_t *sym, const int64_t *out_off, const int64_t *out_len, int64_t n_units, uint8_t *out, int64_t out_cap,
                const void *bad, GunzipArgs &a) {
    if (n_units < 0 || out_cap < 0) ICNV_FAIL(ICNV_ERR_ARG, std::string(who) + ": negative size");
    if (!out_off || !out_len || !bad || (out_cap > 0 && (!sym || !out))) ICNV_FAIL(ICNV_ERR_ARG, std::string(who) + ": null argument");
    if (misaligned(out_off, 8) || misaligned(out_len, 8) || misaligned(bad, 4) || misaligned(sym, 2))
        ICNV_FAIL(ICNV_ERR_ARG, std::string(who) + ": out_off / out_len must be aligned to 8 bytes, bad to 4, sym to 2");
    a = GunzipArgs{nullptr, 0, nullptr, 0, nullptr, n_units, 0, nullptr, const_cast<int64_t *>(out_len), out_off, const_cast<uint16_t *>(sym), out, out_cap, nullptr};
    return ICNV_OK;
}
}  // namespace

int icnv_gunzip_tails_dev(const uint16_t *sym, const int64_t *out_off, const int64_t *out_len, int64_t n_units, uint8_t *out, int64_t out_cap,
                          int32_t *bad, int64_t *markers, void *stream) {
    if (n_units == 0) return ICNV_OK;
    GunzipArgs a;
    int rc;
    if ((rc = places_args("gunzip_tails", sym, out_off, out_len, n_units, out, out_cap, bad, a))) return rc;
    if (!markers || misaligned(markers, 8)) ICNV_FAIL(ICNV_ERR_ARG, "gunzip_tails: markers is null or not aligned to 8 bytes");
    hipStream_t s = (hipStream_t)stream;
    if ((rc = check_units(a, GZ_CHECK_PLACES, "gunzip_tails", s))) return rc;
    return launch_gunzip_tails(a, bad, markers, s);
}

int icnv_gunzip_resolve_dev(const uint16_t *sym, const int64_t *out_off, const int64_t *out_len, int64_t n_units, uint8_t *out, int64_t out_cap,
                            int32_t *bad, void *stream) {
    if (n_units == 0 || out_cap == 0) return ICNV_OK;
    GunzipArgs a;
    int rc;
    if ((rc = places_args("gunzip_resolve", sym, out_off, out_len, n_units, out, out_cap, bad, a))) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = check_units(a, GZ_CHECK_PLACES, "gunzip_resolve", s))) return rc;
    return launch_gunzip_resolve(a, bad, s);
}

}  // extern "C"
