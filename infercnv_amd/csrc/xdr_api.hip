// C ABI of K27 (include/icnv.h "R's XDR stream of a matrix"): everything that can be refused is refused before a launch.
// Kernels: xdr_kernels.hip.  DESIGN.md section 4 K27.
#include "icnv_internal.h"
#include "xdr_internal.h"
#include "../../include/icnv.h"

using namespace icnv;

namespace {

int xdr_check(const char *who, const void *mat, const void *stream, int32_t elem_size, int64_t rows, int64_t cols, int64_t ld,
              int32_t layout, int64_t e0, int64_t e1) {
    const std::string w(who);
    if (!mat || !stream) ICNV_FAIL(ICNV_ERR_ARG, w + ": null argument");
    if (elem_size != 8 && elem_size != 4) ICNV_FAIL(ICNV_ERR_ARG, w + ": elem_size must be 8 or 4");
    if (layout != ICNV_XDR_COLS && layout != ICNV_XDR_ROWS) ICNV_FAIL(ICNV_ERR_ARG, w + ": unknown layout");
    if (rows < 1 || cols < 1 || rows > ((int64_t)1 << 59) / cols) ICNV_FAIL(ICNV_ERR_ARG, w + ": bad matrix dimensions");
    const int64_t row_len = layout == ICNV_XDR_COLS ? rows : cols, n_rows = layout == ICNV_XDR_COLS ? cols : rows;
    if (ld < row_len || (n_rows > 1 && ld > ((int64_t)1 << 59) / n_rows))
        ICNV_FAIL(ICNV_ERR_ARG, w + ": ld is below the row length " + std::to_string(row_len) + " or beyond 2^59 elements in all");
    if (e0 < 0 || e0 > e1 || e1 > rows * cols) ICNV_FAIL(ICNV_ERR_ARG, w + ": the segment must satisfy 0 <= e0 <= e1 <= rows * cols");
    if ((reinterpret_cast<uintptr_t>(mat) | reinterpret_cast<uintptr_t>(stream)) & (uintptr_t)(elem_size - 1))
        ICNV_FAIL(ICNV_ERR_ARG, w + ": a pointer is not aligned to elem_size");
    return ICNV_OK;
}

}  // namespace

extern "C" {

int icnv_xdr_encode_dev(const void *src, int32_t elem_size, int64_t rows, int64_t cols, int64_t ld, int32_t layout, int64_t e0,
                        int64_t e1, void *dst, void *stream) {
    int rc;
    if ((rc = xdr_check("xdr_encode", src, dst, elem_size, rows, cols, ld, layout, e0, e1))) return rc;
    XdrArgs a{const_cast<void *>(src), dst, rows, cols, ld, e0, e1, elem_size, layout, 0};
    return launch_xdr(a, (hipStream_t)stream);
}

int icnv_xdr_decode_dev(const void *src, int32_t elem_size, int64_t rows, int64_t cols, int64_t ld, int32_t layout, int64_t e0,
                        int64_t e1, void *dst, void *stream) {
    int rc;
    if ((rc = xdr_check("xdr_decode", dst, src, elem_size, rows, cols, ld, layout, e0, e1))) return rc;
    XdrArgs a{dst, const_cast<void *>(src), rows, cols, ld, e0, e1, elem_size, layout, 1};
    return launch_xdr(a, (hipStream_t)stream);
}

}  // extern "C"
