// Shared between xdr_api.hip (validation, the choice of kernel) and xdr_kernels.hip (K27: a segment of R's XDR stream of a
// matrix: every element's bytes reversed, the matrix read or written in either layout).  DESIGN.md section 4 K27.
#pragma once
#include <stdint.h>

namespace icnv {

constexpr int XDR_NT = 256;     // lanes of a workgroup
constexpr int XDR_TILE = 64;    // the transposing kernel's tile: 64 stream rows x 64 stream columns

struct XdrArgs {
    void *mat;                  // the matrix: read by encode, written by decode
    void *stream;               // element e of the stream at stream + (e - e0) * elem_size: written by encode, read by decode
    int64_t rows, cols, ld;     // R's dim, and the elements between the matrix's contiguous rows
    int64_t e0, e1;             // the segment, e0 < e1
    int32_t elem_size;          // 8 or 4
    int32_t layout;             // ICNV_XDR_COLS or ICNV_XDR_ROWS
    int32_t decode;             // 0: matrix -> stream, 1: stream -> matrix
};

#ifdef __HIPCC__
int launch_xdr(const XdrArgs &a, hipStream_t s);
#endif

}  // namespace icnv
