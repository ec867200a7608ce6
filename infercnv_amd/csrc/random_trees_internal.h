// Shared between random_trees_api.hip (validation, wave planning, stats) and random_trees_kernels.hip (K10, the permutation
// statistic of the random-trees subclustering).  DESIGN.md section 4 K10.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RT_HD __host__ __device__ __forceinline__
#else
#define RT_HD inline
#endif

namespace icnv {

// ---- NumPy's Philox (numpy/random/src/philox): Philox4x64-10, counter word 0 incremented BEFORE each 4-word block, 32-bit
// draws the low half of a 64-bit word first, then its high half.  The stream of (clade p, iteration r, gene g) is
// Generator(Philox(key=[seed, token_p], counter=[0, g, r, 0])).
RT_HD uint64_t rt_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

struct RtPhilox {
    uint64_t c0, c1, c2, c3, k0, k1;
    uint64_t b0, b1, b2, b3;   // the current block; b0 holds the next 64-bit word
    int pos;                   // 32-bit draws taken from the current block (8 = empty)

    // counter = [0, g, r, w3]: K10 uses w3 = 0, K11 (Leiden) puts its move cluster there
    RT_HD RtPhilox(uint64_t seed, uint64_t token, uint64_t g, uint64_t r, uint64_t w3 = 0)
        : c0(0), c1(g), c2(r), c3(w3), k0(seed), k1(token), b0(0), b1(0), b2(0), b3(0), pos(8) {}

    RT_HD void block() {
        if (++c0 == 0 && ++c1 == 0 && ++c2 == 0) ++c3;   // NumPy's carry
        uint64_t x0 = c0, x1 = c1, x2 = c2, x3 = c3, key0 = k0, key1 = k1;
        for (int round = 0; round < 10; ++round) {
            if (round) { key0 += 0x9E3779B97F4A7C15ull; key1 += 0xBB67AE8584CAA73Bull; }
            const uint64_t lo0 = 0xD2E7470EE14C6C93ull * x0, hi0 = rt_mulhi(0xD2E7470EE14C6C93ull, x0);
            const uint64_t lo1 = 0xCA5A826395121157ull * x2, hi1 = rt_mulhi(0xCA5A826395121157ull, x2);
            x0 = hi1 ^ x1 ^ key0;
            x1 = lo1;
            x2 = hi0 ^ x3 ^ key1;
            x3 = lo0;
        }
        b0 = x0; b1 = x1; b2 = x2; b3 = x3;
        pos = 0;
    }

    RT_HD uint32_t next32() {
        if (pos == 8) block();
        const uint32_t v = (pos & 1) ? (uint32_t)(b0 >> 32) : (uint32_t)b0;
        if (pos & 1) { b0 = b1; b1 = b2; b2 = b3; }
        ++pos;
        return v;
    }

    // philox_next: the next 64-bit word.  A stream takes either 32-bit or 64-bit draws, never both (NumPy caches the high
    // half of a 32-bit draw apart from the word buffer)
    RT_HD uint64_t next64() {
        if (pos >= 8) block();
        const uint64_t v = b0;
        b0 = b1; b1 = b2; b2 = b3;
        pos += 2;
        return v;
    }

    // Generator.random(): (next64 >> 11) * 2^-53
    RT_HD double random() { return (double)(next64() >> 11) * (1.0 / 9007199254740992.0); }

    // random_interval(max) for max < 2^32: masked rejection
    RT_HD uint32_t interval(uint32_t max) {
        uint32_t mask = max;
        mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
        uint32_t v;
        while ((v = next32() & mask) > max) {}
        return v;
    }
};

#if defined(__HIPCC__)
struct RtItems {                 // one wave: items = (clade, iteration) matrices, rows of G doubles, cell-major
    int32_t n_items;
    int32_t G;
    const double *x;             // the input, G x C column-major (a cell's genes contiguous)
    const int32_t *cell_idx;     // packed clade cell lists (device)
    const int64_t *cell_off;     // per clade
    const int32_t *item_clade;   // per item: clade
    const int32_t *item_iter;    // per item: iteration, -1 = the observed matrix
    const int64_t *item_row;     // per item: first row in `m` / `z`
    const uint64_t *token;       // per clade
    uint64_t seed;
    double *m;                   // permuted rows (rows of ld_m doubles)
    int64_t ld_m;
    double *z;                   // smoothed rows (rows of G doubles)
    int32_t window;
};

int launch_rt_check(const double *x, int32_t G, const int32_t *cells, int64_t n_cells, uint32_t *bad, hipStream_t s);
int launch_rt_permute(const RtItems &a, hipStream_t s);
int launch_rt_smooth(const RtItems &a, int64_t n_rows, hipStream_t s);
// per item i: out[out_idx[i]] = max of the raw merge dissimilarities mh[m_off[i] .. m_off[i] + n_i - 2], sqrt for ward.D2
int launch_rt_max_height(const double *mh, const int64_t *m_off, const int32_t *n, const int64_t *out_idx, int32_t n_items,
                         bool root, double *out, hipStream_t s);
#endif

}  // namespace icnv
