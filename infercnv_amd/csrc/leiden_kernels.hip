// Leiden community detection of the Leiden subclustering (.leiden_simple_snn, R/inferCNV_tumor_subclusters.R:726-741:
// igraph's cluster_leiden on the kNN graph of RANN::nn2).  DESIGN.md section 4 K11; the contract is in include/icnv.h and
// restated in tests/leiden_restate.py, which the kernels match bit for bit.
//
//   leiden_check_kernel   every nn_idx entry in [0, n_p) (before anything is clustered)
//   leiden_graph_kernel   one workgroup per problem: count, fill, per-row sort and dedupe -> ascending CSR rows, strengths
//                         (the rows of problem p in its region of 2 k n_p entries, offsets within it)
//   leiden_kernel         one wavefront per problem, persistent: every iteration and level (move, refine, aggregate)
//
// The move phase is sequential by definition: one node visit at a time, the lanes over the node's neighbour list (loops
// over rows longer than 64).  e_vC and each cluster's first position in the list go to per-problem scratch indexed by cluster
// id (integer atomics, a min for the position): candidate order is then the lanes' order and the choice a wave argmax.
// All weights are integers (int64), so every atomic sum is exact whatever its order; the doubles of the gains are
// evaluated by each lane in the contract's order.  This file is compiled with -ffp-contract=off (Makefile).
#include "icnv_internal.h"
#include "leiden_internal.h"
#include "random_trees_internal.h"

namespace icnv {

namespace {

constexpr int LD_WAVE = 64;
constexpr int LD_GRAPH_NT = 256;
constexpr int32_t LD_NONE = 0x7fffffff;

__device__ __forceinline__ int lane_id() { return threadIdx.x & (LD_WAVE - 1); }
__device__ __forceinline__ uint64_t lanes_below() { return (1ull << lane_id()) - 1ull; }

// exclusive scan of in[0, n) into out[0, n) (out[n] = total when out_total) by one wavefront; returns the total
template <typename TI, typename TO>
__device__ int64_t wave_scan(const TI *in, TO *out, int64_t n, bool out_total) {
    int64_t carry = 0;
    for (int64_t b = 0; b < n; b += LD_WAVE) {
        const int64_t i = b + lane_id();
        const int64_t x = i < n ? (int64_t)in[i] : 0;
        int64_t inc = x;
        for (int d = 1; d < LD_WAVE; d <<= 1) {
            const int64_t y = __shfl_up(inc, d, LD_WAVE);
            if (lane_id() >= d) inc += y;
        }
        if (i < n) out[i] = (TO)(carry + inc - x);
        carry += __shfl(inc, LD_WAVE - 1, LD_WAVE);
    }
    if (out_total && lane_id() == 0) out[n] = (TO)carry;
    return carry;
}

// ---------------------------------------------------------------------------------------------------------- graph
__global__ void leiden_check_kernel(LeidenGraph g) {
    const int p = blockIdx.x;
    const int64_t n0 = g.node_off[p], n = g.node_off[p + 1] - n0;
    const int32_t *nn = g.nn + n0 * g.k;
    uint32_t bad = 0;
    for (int64_t e = threadIdx.x; e < n * g.k; e += blockDim.x) {
        const int32_t j = nn[e];
        if (j < 0 || j >= n) bad = 1;
    }
    if (bad) atomicOr(g.bad, 1u);
}

// shell sort (Knuth's gaps) of a[0, n) by one lane
__device__ void lane_sort(int32_t *a, int64_t n) {
    int64_t h = 1;
    while (h < n / 3) h = 3 * h + 1;
    for (; h >= 1; h /= 3)
        for (int64_t i = h; i < n; ++i) {
            const int32_t x = a[i];
            int64_t j = i;
            while (j >= h && a[j - h] > x) { a[j] = a[j - h]; j -= h; }
            a[j] = x;
        }
}

// one workgroup per problem (its threads work as one wavefront each on strided items; the scans use wavefront 0)
__global__ void __launch_bounds__(LD_GRAPH_NT) leiden_graph_kernel(LeidenGraph g) {
    const int p = blockIdx.x;
    const int64_t n0 = g.node_off[p], n = g.node_off[p + 1] - n0, k = g.k;
    const int32_t *nn = g.nn + n0 * k;
    int32_t *cnt = g.cnt + n0, *loop = g.loop + n0, *raw = g.raw + 2 * k * n0, *col = g.col + 2 * k * n0;
    int64_t *raw_off = g.raw_off + n0 + p, *off = g.off + n0 + p, *strength = g.strength + n0;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) { cnt[i] = 0; loop[i] = 0; }
    __syncthreads();
    for (int64_t e = threadIdx.x; e < n * k; e += blockDim.x) {
        const int64_t i = e / k;
        const int32_t j = nn[e];
        if (j == i) loop[i] = 1;
        else { atomicAdd(&cnt[i], 1); atomicAdd(&cnt[j], 1); }
    }
    __syncthreads();
    if (threadIdx.x < LD_WAVE) wave_scan(cnt, raw_off, n, true);
    __syncthreads();
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) cnt[i] = 0;
    __syncthreads();
    for (int64_t e = threadIdx.x; e < n * k; e += blockDim.x) {
        const int32_t i = (int32_t)(e / k), j = nn[e];
        if (j == i) continue;
        raw[raw_off[i] + atomicAdd(&cnt[i], 1)] = j;
        raw[raw_off[j] + atomicAdd(&cnt[j], 1)] = i;
    }
    __syncthreads();
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {   // sort and dedupe each row in place (the order of the atomics is gone)
        int32_t *a = raw + raw_off[i];
        const int64_t m = raw_off[i + 1] - raw_off[i];
        lane_sort(a, m);
        int64_t u = 0;
        for (int64_t t = 0; t < m; ++t)
            if (u == 0 || a[t] != a[u - 1]) a[u++] = a[t];
        cnt[i] = (int32_t)u;
        strength[i] = u + 2 * loop[i];
    }
    __syncthreads();
    if (threadIdx.x < LD_WAVE) {
        wave_scan(cnt, off, n, true);
        int64_t s = 0;
        for (int64_t i = threadIdx.x; i < n; i += LD_WAVE) s += strength[i];
        for (int m = 1; m < LD_WAVE; m <<= 1) s += __shfl_xor(s, m, LD_WAVE);
        if (threadIdx.x == 0) g.strength_sum[p] = s;
    }
    __syncthreads();
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {   // the deduped rows into the compact CSR
        const int64_t d = off[i + 1] - off[i];
        for (int64_t t = 0; t < d; ++t) col[off[i] + t] = raw[raw_off[i] + t];
    }
}

// ---------------------------------------------------------------------------------------------------------- Leiden
struct Level {                    // the graph of one level of one problem
    const int64_t *off;
    const int32_t *nbr;
    const int64_t *ew;            // null: every edge weight 1 (level 0 of a kNN graph)
    const int64_t *w;             // null: every node weight 1 (CPM, level 0)
    __device__ int64_t wt(int64_t v) const { return w ? w[v] : 1; }
    __device__ int64_t ewt(int64_t t) const { return ew ? ew[t] : 1; }
};

struct Prob {                     // per-problem views of the scratch
    int64_t *W, *acc, *Wr, *ext, *wA, *wB, *T;
    int64_t *offA, *offB;
    int32_t *memb, *queue, *stable, *cnt, *stack, *first, *rm, *nonsingle, *amap, *aggof, *renum, *perm, *members, *boff,
        *cursor, *cands, *fin;
    double *cum;
    int32_t *nbrA, *nbrB;
    int64_t *ewA, *ewB;
};

// argmax over the lanes: larger diff, then smaller order
__device__ void wave_best(double &d, int32_t &ord, int32_t &c) {
    for (int m = 1; m < LD_WAVE; m <<= 1) {
        const double d2 = __shfl_xor(d, m, LD_WAVE);
        const int32_t o2 = __shfl_xor(ord, m, LD_WAVE), c2 = __shfl_xor(c, m, LD_WAVE);
        if (d2 > d || (d2 == d && o2 < ord)) { d = d2; ord = o2; c = c2; }
    }
}

__device__ int32_t wave_min(int32_t x) {
    for (int m = 1; m < LD_WAVE; m <<= 1) x = min(x, __shfl_xor(x, m, LD_WAVE));
    return x;
}

// Durstenfeld shuffle of a[i] = i by NumPy's Generator(Philox).permutation(n), on lane 0
__device__ void permutation(int32_t *a, int64_t n, RtPhilox &rng) {
    for (int64_t i = lane_id(); i < n; i += LD_WAVE) a[i] = (int32_t)i;
    __syncthreads();
    if (lane_id() == 0)
        for (int64_t i = n - 1; i >= 1; --i) {
            const int64_t j = rng.interval((uint32_t)i);
            if (j != i) { const int32_t t = a[i]; a[i] = a[j]; a[j] = t; }
        }
    __syncthreads();
}

// key[v] for v < n -> members[] grouped by key (keys < nk), ascending v within a group; boff[0, nk] the group offsets.
// cursor[] scratch (nk).  Chunks of 64 nodes in order; a lane's slot among equal keys of its chunk by the lower lanes.
__device__ void bucket(const int32_t *key, int64_t n, int64_t nk, int32_t *cnt, int32_t *boff, int32_t *cursor, int32_t *members) {
    for (int64_t c = lane_id(); c < nk; c += LD_WAVE) { cnt[c] = 0; cursor[c] = 0; }
    __syncthreads();
    for (int64_t v = lane_id(); v < n; v += LD_WAVE) atomicAdd(&cnt[key[v]], 1);
    __syncthreads();
    wave_scan(cnt, boff, nk, true);
    __syncthreads();
    for (int64_t b = 0; b < n; b += LD_WAVE) {
        const int64_t v = b + lane_id();
        const int32_t c = v < n ? key[v] : -1;
        int rank = 0, total = 0;
        for (int j = 0; j < LD_WAVE; ++j) {
            const int32_t cj = __shfl(c, j, LD_WAVE);
            if (cj == c) { total++; if (j < lane_id()) rank++; }
        }
        const int32_t cur = c >= 0 ? cursor[c] : 0;
        if (c >= 0) members[boff[c] + cur + rank] = (int32_t)v;
        __syncthreads();
        if (c >= 0 && rank == total - 1) cursor[c] = cur + total;
        __syncthreads();
    }
}

// memb[v] renumbered by first appearance in the order of list[0, n) (list null: node order) -> number of clusters.
// first[] must hold LD_NONE on entry and does on exit.
__device__ int64_t renumber(int32_t *memb, const int32_t *list, int64_t n, int32_t *first, int32_t *renum) {
    for (int64_t i = lane_id(); i < n; i += LD_WAVE) {
        const int32_t v = list ? list[i] : (int32_t)i;
        atomicMin(&first[memb[v]], (int32_t)i);
    }
    __syncthreads();
    int64_t K = 0;
    for (int64_t b = 0; b < n; b += LD_WAVE) {
        const int64_t i = b + lane_id();
        bool f = false;
        int32_t c = 0;
        if (i < n) { c = memb[list ? list[i] : i]; f = first[c] == i; }
        const uint64_t m = __ballot(f);
        if (f) renum[c] = (int32_t)(K + __popcll(m & lanes_below()));
        K += __popcll(m);
    }
    __syncthreads();
    for (int64_t i = lane_id(); i < n; i += LD_WAVE) {
        const int32_t v = list ? list[i] : (int32_t)i;
        first[memb[v]] = LD_NONE;
    }
    __syncthreads();
    for (int64_t v = lane_id(); v < n; v += LD_WAVE) memb[v] = renum[memb[v]];
    __syncthreads();
    return K;
}

// the move phase: memb in, renumbered memb out; returns K (or -1: cap exceeded)
__device__ int64_t move_nodes(const Level &L, int64_t N, double r, Prob &P, RtPhilox rng, int64_t &visits) {
    for (int64_t c = lane_id(); c < N; c += LD_WAVE) { P.W[c] = 0; P.cnt[c] = 0; P.stable[c] = 0; }
    __syncthreads();
    for (int64_t v = lane_id(); v < N; v += LD_WAVE) {
        atomicAdd((unsigned long long *)&P.W[P.memb[v]], (unsigned long long)L.wt(v));
        atomicAdd(&P.cnt[P.memb[v]], 1);
    }
    __syncthreads();
    int64_t sp = 0;                       // the stack of unused ids, pushed in increasing order
    for (int64_t b = 0; b < N; b += LD_WAVE) {
        const int64_t c = b + lane_id();
        const bool e = c < N && P.cnt[c] == 0;
        const uint64_t m = __ballot(e);
        if (e) P.stack[sp + __popcll(m & lanes_below())] = (int32_t)c;
        sp += __popcll(m);
    }
    permutation(P.queue, N, rng);
    int64_t head = 0, qlen = N, pops = 0;
    const int64_t cap = leiden_move_cap(N);
    while (qlen > 0) {
        if (++pops > cap) return -1;
        const int32_t v = P.queue[head];
        head = head + 1 == N ? 0 : head + 1;
        --qlen;
        const int32_t c0 = P.memb[v];
        const int64_t wv = L.wt(v);
        const int32_t cnt0 = P.cnt[c0] - 1;
        const int64_t W0 = P.W[c0] - wv;
        __syncthreads();
        if (lane_id() == 0) { P.cnt[c0] = cnt0; P.W[c0] = W0; if (cnt0 == 0) P.stack[sp] = c0; }
        if (cnt0 == 0) ++sp;
        const int64_t beg = L.off[v], d = L.off[v + 1] - beg;
        for (int64_t t = lane_id(); t < d; t += LD_WAVE) {
            const int32_t C = P.memb[L.nbr[beg + t]];
            atomicAdd((unsigned long long *)&P.acc[C], (unsigned long long)L.ewt(beg + t));
            atomicMin(&P.first[C], (int32_t)t);
        }
        __syncthreads();
        const double dwv = (double)wv;
        double bd = (double)P.acc[c0] - ((dwv * (double)W0) * r);
        int32_t bord = -2, best = c0;
        if (sp > 0) {
            const int32_t top = P.stack[sp - 1];
            const int64_t Wt = top == c0 ? W0 : P.W[top];
            const double dt = (double)P.acc[top] - ((dwv * (double)Wt) * r);
            if (dt > bd) { bd = dt; bord = -1; best = top; }
        }
        for (int64_t t = lane_id(); t < d; t += LD_WAVE) {
            const int32_t C = P.memb[L.nbr[beg + t]];
            if (P.first[C] != t) continue;
            const int64_t WC = C == c0 ? W0 : P.W[C];
            const double dc = (double)P.acc[C] - ((dwv * (double)WC) * r);
            if (dc > bd) { bd = dc; bord = (int32_t)t; best = C; }
        }
        wave_best(bd, bord, best);
        __syncthreads();
        for (int64_t t = lane_id(); t < d; t += LD_WAVE) {
            const int32_t C = P.memb[L.nbr[beg + t]];
            P.acc[C] = 0;
            P.first[C] = LD_NONE;
        }
        const int32_t cntb = best == c0 ? cnt0 : P.cnt[best];
        const int64_t Wb = best == c0 ? W0 : P.W[best];
        __syncthreads();
        if (cntb == 0) --sp;              // best was empty: it is the top of the stack
        if (lane_id() == 0) { P.memb[v] = best; P.W[best] = Wb + wv; P.cnt[best] = cntb + 1; P.stable[v] = 1; }
        __syncthreads();
        if (best != c0) {
            for (int64_t b = 0; b < d; b += LD_WAVE) {
                const int64_t t = b + lane_id();
                bool q = false;
                int32_t u = 0;
                if (t < d) { u = L.nbr[beg + t]; q = P.stable[u] && P.memb[u] != best; }
                const uint64_t m = __ballot(q);
                if (q) {
                    int64_t at = head + qlen + __popcll(m & lanes_below());
                    if (at >= N) at -= N;
                    P.queue[at] = u;
                    P.stable[u] = 0;
                }
                qlen += __popcll(m);
            }
            __syncthreads();
        }
    }
    visits += pops;
    return renumber(P.memb, nullptr, N, P.first, P.renum);
}

// the refinement of every move cluster; returns R, the number of refined clusters (numbered into P.amap)
__device__ int64_t refine(const Level &L, int64_t N, int64_t K, double r, double beta, uint64_t seed, uint64_t token, int it,
                          int level, Prob &P, int64_t &visits, int64_t &draws) {
    bucket(P.memb, N, K, P.cnt, P.boff, P.cursor, P.members);
    for (int64_t c = lane_id(); c < K; c += LD_WAVE) P.T[c] = 0;
    __syncthreads();
    for (int64_t v = lane_id(); v < N; v += LD_WAVE) {
        const int32_t c = P.memb[v];
        atomicAdd((unsigned long long *)&P.T[c], (unsigned long long)L.wt(v));
        int64_t e = 0;
        for (int64_t t = L.off[v]; t < L.off[v + 1]; ++t)
            if (P.memb[L.nbr[t]] == c) e += L.ewt(t);
        P.ext[v] = e;
        P.Wr[v] = L.wt(v);
        P.rm[v] = (int32_t)v;
        P.nonsingle[v] = 0;
    }
    __syncthreads();
    for (int64_t c = 0; c < K; ++c) {
        const int32_t *S = P.members + P.boff[c];
        const int64_t ns = P.boff[c + 1] - P.boff[c], T = P.T[c];
        RtPhilox order(seed, token, 2, ((uint64_t)it << 32) | (uint32_t)level, (uint64_t)c);
        RtPhilox rng(seed, token, 3, ((uint64_t)it << 32) | (uint32_t)level, (uint64_t)c);
        permutation(P.perm, ns, order);
        for (int64_t i = 0; i < ns; ++i) {
            const int32_t v = S[P.perm[i]];
            if (P.nonsingle[v]) continue;
            const int64_t wv = L.wt(v);
            const double dwv = (double)wv;
            if (!((double)P.ext[v] >= ((dwv * (double)(T - wv)) * r))) continue;
            ++visits;
            __syncthreads();
            if (lane_id() == 0) { P.Wr[v] = 0; P.ext[v] = 0; }
            const int64_t beg = L.off[v], d = L.off[v + 1] - beg;
            for (int64_t t = lane_id(); t < d; t += LD_WAVE) {
                const int32_t u = L.nbr[beg + t];
                if (P.memb[u] != c) continue;
                const int32_t D = P.rm[u];
                atomicAdd((unsigned long long *)&P.acc[D], (unsigned long long)L.ewt(beg + t));
                atomicMin(&P.first[D], (int32_t)t);
            }
            __syncthreads();
            // candidates: the emptied cluster v, then the neighbours' refined clusters by first appearance
            double bd = 0.0;
            int32_t bord = -1, best = v;
            int64_t nc = 1;
            if (lane_id() == 0) { P.cands[0] = v; P.cum[0] = lib_exp(0.0 / beta); }
            for (int64_t b = 0; b < d; b += LD_WAVE) {
                const int64_t t = b + lane_id();
                bool f = false;
                int32_t D = 0;
                if (t < d) {
                    const int32_t u = L.nbr[beg + t];
                    if (P.memb[u] == c) { D = P.rm[u]; f = P.first[D] == t; }
                }
                const uint64_t m = __ballot(f);
                if (f) {
                    const int64_t j = nc + __popcll(m & lanes_below());
                    const double WD = (double)P.Wr[D];
                    double term = -1.0;   // not part of the sum
                    if ((double)P.ext[D] >= ((WD * (double)(T - P.Wr[D])) * r)) {
                        const double dd = (double)P.acc[D] - ((dwv * WD) * r);
                        if (dd > bd) { bd = dd; bord = (int32_t)j; best = D; }
                        if (dd >= 0) term = lib_exp(dd / beta);
                    }
                    P.cands[j] = D;
                    P.cum[j] = term;
                }
                nc += __popcll(m);
            }
            wave_best(bd, bord, best);
            __syncthreads();
            // the running sum in candidate order, the draw and the choice (every lane the same, uniform loads)
            double total = 0.0;
            int64_t last = 0;
            for (int64_t j = 0; j < nc; ++j) {
                const double term = P.cum[j];
                if (term >= 0) { total = total + term; last = j; }
                P.cum[j] = total;   // every lane stores the same value
            }
            int32_t chosen = best;
            if (total < INFINITY) {
                const double tdraw = rng.random() * total;
                ++draws;
                int32_t jmin = LD_NONE;
                for (int64_t j = lane_id(); j < nc; j += LD_WAVE)
                    if (P.cum[j] > tdraw) { jmin = (int32_t)j; break; }
                jmin = wave_min(jmin);
                chosen = P.cands[jmin == LD_NONE ? last : jmin];
            }
            __syncthreads();
            for (int64_t t = lane_id(); t < d; t += LD_WAVE) {
                const int32_t u = L.nbr[beg + t];
                if (P.memb[u] != c) continue;
                const int32_t D = P.rm[u];
                P.acc[D] = 0;
                P.first[D] = LD_NONE;
                const int64_t e = L.ewt(beg + t);
                atomicAdd((unsigned long long *)&P.ext[chosen], (unsigned long long)(D == chosen ? -e : e));
            }
            __syncthreads();
            if (lane_id() == 0) {
                P.Wr[chosen] += wv;
                P.rm[v] = chosen;
                if (chosen != v) P.nonsingle[chosen] = 1;
            }
            __syncthreads();
        }
    }
    // number the refined clusters by (move cluster, first appearance in ascending node order)
    for (int64_t v = lane_id(); v < N; v += LD_WAVE) P.amap[v] = P.rm[v];
    __syncthreads();
    return renumber(P.amap, P.members, N, P.first, P.renum);
}

// the graph of the next level into (off2, nbr2, ew2, w2): one node per value of amap, weights and edges summed, no loops
__device__ void aggregate(const Level &L, int64_t N, int64_t n2, Prob &P, int64_t *off2, int32_t *nbr2, int64_t *ew2, int64_t *w2) {
    __shared__ int32_t touched;
    for (int64_t a = lane_id(); a < n2; a += LD_WAVE) w2[a] = 0;
    __syncthreads();
    for (int64_t v = lane_id(); v < N; v += LD_WAVE) atomicAdd((unsigned long long *)&w2[P.amap[v]], (unsigned long long)L.wt(v));
    bucket(P.amap, N, n2, P.cnt, P.boff, P.cursor, P.members);
    int64_t eo = 0;
    if (lane_id() == 0) off2[0] = 0;
    for (int64_t a = 0; a < n2; ++a) {
        if (lane_id() == 0) touched = 0;
        __syncthreads();
        for (int64_t m = P.boff[a]; m < P.boff[a + 1]; ++m) {
            const int32_t v = P.members[m];
            const int64_t beg = L.off[v], d = L.off[v + 1] - beg;
            for (int64_t t = lane_id(); t < d; t += LD_WAVE) {
                const int32_t b = P.amap[L.nbr[beg + t]];
                if (b == a) continue;
                atomicAdd((unsigned long long *)&P.acc[b], (unsigned long long)L.ewt(beg + t));
                if (atomicCAS(&P.first[b], LD_NONE, 0) == LD_NONE) P.cands[atomicAdd(&touched, 1)] = b;
            }
        }
        __syncthreads();
        const int64_t nt = touched;
        for (int64_t i = lane_id(); i < nt; i += LD_WAVE) {   // rank sort of the distinct neighbours
            const int32_t key = P.cands[i];
            int64_t rank = 0;
            for (int64_t j = 0; j < nt; ++j) rank += P.cands[j] < key;
            nbr2[eo + rank] = key;
            ew2[eo + rank] = P.acc[key];
        }
        __syncthreads();
        for (int64_t i = lane_id(); i < nt; i += LD_WAVE) {
            const int32_t key = P.cands[i];
            P.acc[key] = 0;
            P.first[key] = LD_NONE;
        }
        eo += nt;
        if (lane_id() == 0) off2[a + 1] = eo;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(LD_WAVE) leiden_kernel(LeidenArgs a) {
    const int p = blockIdx.x;
    const int64_t n0 = a.g.node_off[p], n = a.g.node_off[p + 1] - n0;
    const int64_t eb = a.edge_off ? a.edge_off[p] : 2 * (int64_t)a.g.k * n0;   // the problem's edge region
    const int64_t tn = a.total_n, to = a.total_n + a.g.n_prob;
    Prob P;
    int64_t *I = a.i64 + n0;
    P.W = I; P.acc = I + tn; P.Wr = I + 2 * tn; P.ext = I + 3 * tn; P.wA = I + 4 * tn; P.wB = I + 5 * tn; P.T = I + 6 * tn;
    P.offA = a.offs + n0 + p; P.offB = P.offA + to;
    int32_t *J = a.i32 + n0 + p;   // n + 1 slots per problem (boff)
    int32_t **arr[LEIDEN_I32_ARRAYS] = {&P.memb, &P.queue, &P.stable, &P.cnt, &P.stack, &P.first, &P.rm, &P.nonsingle, &P.amap,
                                        &P.aggof, &P.renum, &P.perm, &P.members, &P.boff, &P.cursor, &P.cands, &P.fin};
    for (int i = 0; i < LEIDEN_I32_ARRAYS; ++i) *arr[i] = J + i * (tn + a.g.n_prob);
    P.cum = a.cum + n0;
    P.nbrA = a.nbr + eb; P.nbrB = P.nbrA + a.total_e;
    P.ewA = a.ew + eb; P.ewB = P.ewA + a.total_e;
    const double r = a.r[p];
    const uint64_t token = a.token[p];
    int64_t cnt_levels = 0, cnt_move = 0, cnt_refine = 0, cnt_draws = 0;
    int status = LEIDEN_OK;
    int64_t K = 0;

    for (int64_t v = lane_id(); v < n; v += LD_WAVE) { P.fin[v] = (int32_t)v; P.first[v] = LD_NONE; P.acc[v] = 0; }
    __syncthreads();
    for (int it = 0; it < a.n_iterations && status == LEIDEN_OK; ++it) {
        Level L;
        L.off = a.g.off + n0 + p; L.nbr = a.g.col + eb; L.ew = a.ew0 ? a.ew0 + eb : nullptr;
        L.w = a.objective == ICNV_LEIDEN_MODULARITY ? a.g.strength + n0 : nullptr;
        for (int64_t v = lane_id(); v < n; v += LD_WAVE) { P.memb[v] = P.fin[v]; P.aggof[v] = (int32_t)v; }
        __syncthreads();
        int64_t N = n;
        for (int level = 0;; ++level) {
            if (level >= LEIDEN_MAX_LEVELS) { status = LEIDEN_LEVEL_CAP; break; }
            ++cnt_levels;
            RtPhilox order(a.seed, token, 1, ((uint64_t)it << 32) | (uint32_t)level, 0);
            K = move_nodes(L, N, r, P, order, cnt_move);
            if (K < 0) { status = LEIDEN_MOVE_CAP; break; }
            if (K == N) break;
            const int64_t R = refine(L, N, K, r, a.beta, a.seed, token, it, level, P, cnt_refine, cnt_draws);
            int64_t n2;
            if (R == N) {                         // the refinement did not aggregate: aggregate on the move clusters
                n2 = K;
                for (int64_t v = lane_id(); v < N; v += LD_WAVE) P.amap[v] = P.memb[v];
                __syncthreads();
            } else {
                n2 = R;
            }
            const bool toA = (level & 1) == 0;
            int64_t *off2 = toA ? P.offA : P.offB, *ew2 = toA ? P.ewA : P.ewB, *w2 = toA ? P.wA : P.wB;
            int32_t *nbr2 = toA ? P.nbrA : P.nbrB;
            aggregate(L, N, n2, P, off2, nbr2, ew2, w2);
            // each aggregate starts the next level in its move cluster; the original nodes follow their aggregates
            for (int64_t v = lane_id(); v < N; v += LD_WAVE) P.cursor[P.amap[v]] = R == N ? P.amap[v] : P.memb[v];
            __syncthreads();
            for (int64_t x = lane_id(); x < n2; x += LD_WAVE) P.memb[x] = P.cursor[x];
            for (int64_t v = lane_id(); v < n; v += LD_WAVE) P.aggof[v] = P.amap[P.aggof[v]];
            __syncthreads();
            L.off = off2; L.nbr = nbr2; L.ew = ew2; L.w = w2;
            N = n2;
        }
        if (status != LEIDEN_OK) break;
        for (int64_t v = lane_id(); v < n; v += LD_WAVE) P.fin[v] = P.memb[P.aggof[v]];
        __syncthreads();
        K = renumber(P.fin, nullptr, n, P.first, P.renum);
    }
    for (int64_t v = lane_id(); v < n; v += LD_WAVE) a.membership[n0 + v] = P.fin[v] + 1;
    if (lane_id() == 0) {
        a.n_clusters[p] = (int32_t)K;
        a.status[p] = status;
        int64_t *c = a.counters + (int64_t)p * LEIDEN_CNT_N;
        c[LEIDEN_CNT_LEVELS] = cnt_levels; c[LEIDEN_CNT_MOVE] = cnt_move; c[LEIDEN_CNT_REFINE] = cnt_refine; c[LEIDEN_CNT_DRAWS] = cnt_draws;
    }
}

}  // namespace

int launch_leiden_check(const LeidenGraph &g, hipStream_t s) {
    hipLaunchKernelGGL(leiden_check_kernel, dim3(g.n_prob), dim3(LD_GRAPH_NT), 0, s, g);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_leiden_graph(const LeidenGraph &g, hipStream_t s) {
    hipLaunchKernelGGL(leiden_graph_kernel, dim3(g.n_prob), dim3(LD_GRAPH_NT), 0, s, g);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_leiden(const LeidenArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(leiden_kernel, dim3(a.g.n_prob), dim3(LD_WAVE), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

}  // namespace icnv
