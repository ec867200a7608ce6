// C ABI of K28 (include/icnv.h "DEFLATE in independent pieces"): everything that can be refused is refused before a launch.
// Kernels: deflate_kernels.hip.  DESIGN.md section 4 K28.
#include "icnv_internal.h"
#include "deflate_internal.h"
#include "../../include/icnv.h"

using namespace icnv;

extern "C" {

int64_t icnv_deflate_bound(int64_t piece_bytes) {
    if (piece_bytes < DF_MIN_PIECE || piece_bytes > DF_MAX_PIECE) return -1;
    return deflate_bound(piece_bytes);
}

int icnv_deflate_pieces_dev(const uint8_t *src, int64_t n, int64_t piece_bytes, uint8_t *dst, int64_t dst_stride, int32_t *piece_len,
                            uint32_t *piece_crc, void *stream) {
    if (n < 0) ICNV_FAIL(ICNV_ERR_ARG, "deflate_pieces: negative length");
    if (piece_bytes < DF_MIN_PIECE || piece_bytes > DF_MAX_PIECE)
        ICNV_FAIL(ICNV_ERR_ARG, "deflate_pieces: piece_bytes must lie in [" + std::to_string(DF_MIN_PIECE) + ", " + std::to_string(DF_MAX_PIECE) + "]");
    if (dst_stride < deflate_bound(piece_bytes))
        ICNV_FAIL(ICNV_ERR_ARG, "deflate_pieces: dst_stride is below icnv_deflate_bound(piece_bytes) = " + std::to_string(deflate_bound(piece_bytes)));
    if (n == 0) return ICNV_OK;
    if (!src || !dst || !piece_len || !piece_crc) ICNV_FAIL(ICNV_ERR_ARG, "deflate_pieces: null argument");
    if ((reinterpret_cast<uintptr_t>(piece_len) | reinterpret_cast<uintptr_t>(piece_crc)) & 3)
        ICNV_FAIL(ICNV_ERR_ARG, "deflate_pieces: piece_len or piece_crc is not aligned to 4 bytes");
    const int64_t n_pieces = (n + piece_bytes - 1) / piece_bytes;
    if (n_pieces > 0x7fffffff) ICNV_FAIL(ICNV_ERR_ARG, "deflate_pieces: more than 2^31 - 1 pieces");
    if (dst_stride > ((int64_t)1 << 59) / n_pieces) ICNV_FAIL(ICNV_ERR_ARG, "deflate_pieces: dst_stride * pieces is beyond 2^59");
    DeflateArgs a{src, n, (int32_t)piece_bytes, dst, dst_stride, (int32_t)deflate_bound(piece_bytes), piece_len, piece_crc, n_pieces};
    return launch_deflate_pieces(a, (hipStream_t)stream);
}

int icnv_deflate_pack_dev(const uint8_t *dst, int64_t dst_stride, const int32_t *piece_len, int64_t n_pieces, uint8_t *out, int64_t out_cap,
                          int64_t *out_len, void *stream) {
    if (!out_len) ICNV_FAIL(ICNV_ERR_ARG, "deflate_pack: null out_len");
    *out_len = 0;
    if (n_pieces < 0 || n_pieces > 0x7fffffff || out_cap < 0 || dst_stride < 1) ICNV_FAIL(ICNV_ERR_ARG, "deflate_pack: bad sizes");
    if (n_pieces == 0) return ICNV_OK;
    if (!dst || !piece_len || !out) ICNV_FAIL(ICNV_ERR_ARG, "deflate_pack: null argument");
    if (dst_stride > ((int64_t)1 << 59) / n_pieces) ICNV_FAIL(ICNV_ERR_ARG, "deflate_pack: dst_stride * pieces is beyond 2^59");
    hipStream_t s = (hipStream_t)stream;
    DevBuf offsets;
    int rc;
    if ((rc = offsets.alloc((size_t)(n_pieces + 1) * sizeof(int64_t)))) return rc;
    if ((rc = launch_deflate_offsets(piece_len, n_pieces, dst_stride, offsets.as<int64_t>(), s))) return rc;   // the lengths pass
    int64_t total = 0;
    ICNV_HIP(hipMemcpyAsync(&total, offsets.as<int64_t>() + n_pieces, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    if (total > out_cap)                                            // before the emit pass: nothing has touched `out`
        ICNV_FAIL(ICNV_ERR_ARG, "deflate_pack: out_cap " + std::to_string(out_cap) + " is below the packed size " + std::to_string(total));
    if ((rc = launch_deflate_copy(dst, dst_stride, offsets.as<int64_t>(), n_pieces, out, out_cap, s))) return rc;
    ICNV_HIP(hipStreamSynchronize(s));                              // the offsets go back to the pool: the copy has read them
    *out_len = total;
    return ICNV_OK;
}

}  // extern "C"
