// Shared between matrix_sum_api.hip (validation, the carry and the one rounding) and matrix_sum_kernels.hip (K23: the exact
// sum of a matrix in a long fixed-point accumulator).  DESIGN.md section 4 K23.  The host part is plain C++: it compiles
// without HIP (a stand-alone check includes this header alone).
#pragma once
#include <math.h>
#include <stdint.h>

namespace icnv {

constexpr int MS_NT = 256;                       // lanes of a workgroup
constexpr int MS_WAVES = MS_NT / 64;
constexpr int MS_UNROLL = 8;                     // 16-byte loads of one lane per tile
constexpr int MS_TILE = MS_NT * MS_UNROLL * 2;   // values of one tile: a run of one row
// Bit b of the accumulator is worth 2^(b - 1074): bit 0 is the last bit of a subnormal.  The largest double,
// (2^53 - 1) * 2^971, ends at bit 2097; digit k holds bits 32 k .. 32 k + 31 in a signed 64-bit limb.  A value lands in
// three consecutive digits, the first at most 63; a lane's window of four starts at most there: 67 limbs, rounded up.
constexpr int MS_LIMBS = 68;
constexpr int MS_SLOTS = MS_LIMBS + 1;           // a workgroup's record: its limbs and the flags of what it met
constexpr int64_t MS_MAX_TILES_PER_WG = 1 << 18; // 2^22 values per lane: a workgroup's limb stays below 2^62
enum { MS_NAN = 1, MS_POS_INF = 2, MS_NEG_INF = 4 };

// The records of `n_wg` workgroups to the sum: limb by limb in 128 bits, one carry pass from the bottom, then the one
// rounding to nearest, ties to even.  flags: the OR of every record's last slot.
inline double ms_finish(const int64_t *records, int64_t n_wg) {
    int flags = 0;
    __int128 limb[MS_LIMBS];
    for (int k = 0; k < MS_LIMBS; ++k) limb[k] = 0;
    for (int64_t w = 0; w < n_wg; ++w) {
        for (int k = 0; k < MS_LIMBS; ++k) limb[k] += records[w * MS_SLOTS + k];
        flags |= (int)records[w * MS_SLOTS + MS_LIMBS];
    }
    if ((flags & MS_NAN) || ((flags & MS_POS_INF) && (flags & MS_NEG_INF))) return NAN;
    if (flags & MS_POS_INF) return INFINITY;
    if (flags & MS_NEG_INF) return -INFINITY;
    // digits of the two's-complement value; the carry out of the last limb is its sign extension
    constexpr int ND = MS_LIMBS + 4;
    uint32_t digit[ND];
    __int128 carry = 0;
    for (int k = 0; k < ND; ++k) {
        const __int128 v = (k < MS_LIMBS ? limb[k] : (__int128)0) + carry;
        digit[k] = (uint32_t)(v & 0xffffffff);
        carry = v >> 32;                          // arithmetic: floor division
    }
    const bool negative = carry < 0;              // (carry is 0 or -1 here: ND digits hold every sum of 2^62 values)
    if (negative) {                               // magnitude = two's complement
        uint64_t c = 1;
        for (int k = 0; k < ND; ++k) {
            const uint64_t v = (uint64_t)(uint32_t)~digit[k] + c;
            digit[k] = (uint32_t)v;
            c = v >> 32;
        }
    }
    int top = -1;                                 // index of the highest set bit
    for (int k = ND - 1; k >= 0 && top < 0; --k)
        if (digit[k]) top = 32 * k + 31 - __builtin_clz(digit[k]);
    if (top < 0) return 0.0;
    auto bit = [&](int b) -> uint64_t { return b < 0 ? 0 : (digit[b >> 5] >> (b & 31)) & 1u; };
    const int low = top > 52 ? top - 52 : 0;      // the last bit that is kept
    uint64_t mant = 0;
    for (int b = top; b >= low; --b) mant = (mant << 1) | bit(b);
    if (low > 0 && bit(low - 1)) {                // more than or exactly half of the last place
        bool sticky = false;
        for (int b = low - 2; b >= 0 && !sticky; --b) {
            if ((b & 31) == 31 && digit[b >> 5] == 0) { b -= 31; continue; }
            sticky = bit(b);
        }
        if (sticky || (mant & 1)) ++mant;         // (2^53 is a double too; ldexp carries it into the exponent)
    }
    const double r = ldexp((double)mant, low - 1074);   // exact, or +Inf beyond the range
    return negative ? -r : r;
}

#ifdef __HIPCC__
int launch_matrix_sum(const double *x, int64_t ld, int64_t G, int64_t C, int64_t *records, int64_t *n_wg, hipStream_t s);
int64_t matrix_sum_workgroups(int64_t ld, int64_t G, int64_t C);   // records the launch writes; 0 when it needs more than 2^31 - 1
#endif

}  // namespace icnv
