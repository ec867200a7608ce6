// Shared between deflate_api.hip (validation) and deflate_kernels.hip (K28: bytes on the device into DEFLATE, RFC 1951, in
// independent pieces; the pieces packed into one buffer).  DESIGN.md section 4 K28.
#pragma once
#include <stdint.h>

namespace icnv {

constexpr int DF_NT = 256;              // lanes of a workgroup: one workgroup per piece
constexpr int DF_MIN_PIECE = 256;       // the allowed piece_bytes
constexpr int DF_MAX_PIECE = 16384;     // (input, match records, hash table and staging of one piece: 77 KiB of LDS, two per CU)
constexpr int DF_SUB = DF_MAX_PIECE / DF_NT;   // bytes of a piece one lane folds into the CRC

inline int64_t deflate_bound(int64_t piece_bytes) {   // stored blocks: 5 bytes of header per 65 535 bytes
    return piece_bytes + 5 * ((piece_bytes + 65534) / 65535);
}

struct DeflateArgs {
    const uint8_t *src;
    int64_t n;                  // bytes of src
    int32_t piece_bytes;
    uint8_t *dst;
    int64_t dst_stride;
    int32_t bound;              // deflate_bound(piece_bytes): no store lands at or beyond dst + i * dst_stride + bound
    int32_t *piece_len;
    uint32_t *piece_crc;
    int64_t n_pieces;
};

#ifdef __HIPCC__
int launch_deflate_pieces(const DeflateArgs &a, hipStream_t s);
// offsets: n_pieces + 1 int64 of device scratch; offsets[n_pieces] is the packed size
int launch_deflate_offsets(const int32_t *piece_len, int64_t n_pieces, int64_t dst_stride, int64_t *offsets, hipStream_t s);
int launch_deflate_copy(const uint8_t *dst, int64_t dst_stride, const int64_t *offsets, int64_t n_pieces, uint8_t *out, int64_t out_cap,
                        hipStream_t s);
#endif

}  // namespace icnv
