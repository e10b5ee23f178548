// What the translation units of libdeeprob_clt.so share: the library's instance of the shared entry-point scaffolding
// (error text, checks, check_net for the arguments every network query takes), lse2 / lse64 of the header's order of
// operations, pack_tile (a tile of x to bit planes) and pair_tile (the 32 x 32 pair-count tile, plain, segmented or under a
// cut) of the learners, copy_rows (a work-group's rows of x to out), a tree as a Leaf
// with its passes (gather, upward, beliefs: a leaf of a cutset network, or with COLS = false a stand-alone tree), and a
// cutset network as a Net with THE walk of its OR tree: or_walk owns the explicit stack and the guard that keeps a row
// inside it, a visitor says what a query computes on the way (ValueVisitor here: the log likelihood, for cnet.hip and
// the first walk of marginals.hip; cnet_queries.hip and marginals.hip bring their own).  The samplers draw with
// dp_device::counter_uniform (shared/device.h).
#pragma once
#include "../../../include/deeprob_clt.h"
#define DP_ENTRY_NS dpc_detail
#define DP_ENTRY_ELAUNCH DPC_ELAUNCH
#include "../shared/entry.h"
#include "../shared/device.h"

#define DPC_REQUIRE(cond, ...) DP_REQUIRE(cond, DPC_EINVAL, __VA_ARGS__)
#define DPC_LAUNCH DP_LAUNCH

namespace dpc_detail {

// The pair counts (clt.hip, cnet.hip, cut.hip): a work-group of kPairThreads owns kPairTile x kPairTile variable pairs
// and stages kPairWords plane words of both operands per step; grid.z is the task or the entry of the segmented ones.
constexpr int kPairThreads = 256;
constexpr int kPairTile = 32;
constexpr int kPairWords = 32;
constexpr int kPackThreads = 256;
constexpr int kPackTile = 64;      // rows and columns of x per packing work-group
constexpr int kMaxGridZ = 65535;
constexpr int64_t kMaxGridX = 2147483647;
static_assert(kPairThreads % kPairWords == 0, "a thread stages one word column");

// Rows of x to bit planes, the step pack_bits_kernel (clt.hip) and gather_pack_kernel (cnet.hip) share: a work-group of
// kPackThreads owns plane word `word` of the 64 columns from 64 blockIdx.y.  value(rr, c) is x at line rr of the tile,
// column c (0 past the rows or the columns); a line is loaded by one wave, coalesced, and the tile is read back by column.
template <typename Value>
__device__ __forceinline__ void pack_tile(Value value, int64_t word, int d, int64_t n_words,
                                          unsigned long long *__restrict__ planes) {
    __shared__ float tile[kPackTile][kPackTile + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = blockIdx.y * kPackTile;
    for (int rr = wave; rr < kPackTile; rr += kPackThreads / 64) tile[rr][lane] = value(rr, c0 + lane);
    __syncthreads();
    // wave w owns columns 16 w .. 16 w + 15 of the tile; lane c keeps the word of "its" column and stores it
    unsigned long long mine = 0;
    for (int cc = 0; cc < 16; ++cc) {
        const unsigned long long m = __ballot(tile[lane][wave * 16 + cc] == 1.f);
        if (lane == cc) mine = m;
    }
    const int c = c0 + wave * 16 + lane;
    if (lane < 16 && c < d) planes[(int64_t)c * n_words + word] = mine;
}

// One 32 x 32 tile of co-occurrence counts over the plane words [w_begin, w_end): out[i][j] = sum_w popc(plane_i & plane_j
// [& cut]) for the pairs of tile (blockIdx.y, blockIdx.x).  Only tiles on or above the diagonal are computed, each writes
// its mirror image too.  Thread (ty, tx) of the 16 x 16 work-group owns the pairs (ty + 16 a, tx + 16 b), a, b in {0, 1}.
// The rows of the LDS tiles are padded to kPairWords + 1 words: the 16 rows a half-wave reads then lie 2 banks apart (66
// dwords a row, 64 banks for a 64-bit read), and the lanes that share a row read one address.  CUT: the words of the plane
// `cut` are ANDed into the j operand while the step is staged, so the popcount loop is that of the unconditioned counts
// (`cut` is one of `planes`: both are only read; without CUT it is not read at all and may be null).
template <bool CUT>
__device__ __forceinline__ void pair_tile(const unsigned long long *__restrict__ planes, int64_t n_words, int d,
                                          int64_t w_begin, int64_t w_end, const unsigned long long *__restrict__ cut,
                                          int32_t *__restrict__ out) {
    typedef unsigned long long u64;
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (tj < ti) return;            // the mirror image is written by tile (tj, ti)
    __shared__ u64 pi[kPairTile][kPairWords + 1], pj[kPairTile][kPairWords + 1];
    const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
    int acc[2][2] = {{0, 0}, {0, 0}};
    for (int64_t w0 = w_begin; w0 < w_end; w0 += kPairWords) {
        // kPairThreads is a multiple of kPairWords: a thread stages the same word of every row it touches
        const int w = t % kPairWords;
        const bool in = w0 + w < w_end;
        const u64 pc = (CUT && in) ? cut[w0 + w] : 0ull;
        for (int e = t; e < kPairTile * kPairWords; e += kPairThreads) {
            const int r = e / kPairWords;
            const int i = ti * kPairTile + r, j = tj * kPairTile + r;
            pi[r][w] = (in && i < d) ? planes[(int64_t)i * n_words + w0 + w] : 0ull;
            pj[r][w] = (in && j < d) ? planes[(int64_t)j * n_words + w0 + w] & (CUT ? pc : ~0ull) : 0ull;
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < kPairWords; ++k) {
            const u64 a0 = pi[ty][k], a1 = pi[ty + 16][k], b0 = pj[tx][k], b1 = pj[tx + 16][k];
            acc[0][0] += __popcll(a0 & b0);
            acc[0][1] += __popcll(a0 & b1);
            acc[1][0] += __popcll(a1 & b0);
            acc[1][1] += __popcll(a1 & b1);
        }
        __syncthreads();
    }
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) {
            const int i = ti * kPairTile + ty + 16 * a, j = tj * kPairTile + tx + 16 * b;
            if (i < d && j < d) {
                out[(int64_t)i * d + j] = acc[a][b];
                out[(int64_t)j * d + i] = acc[a][b];
            }
        }
}

__device__ __forceinline__ float lse2(float a, float b) {
    const float hi = fmaxf(a, b), lo = fminf(a, b);
    if (hi == -INFINITY) return -INFINITY;
    return hi + log1pf(expf(lo - hi));
}

__device__ __forceinline__ double lse64(double x, double y) {
    const double hi = fmax(x, y), lo = fmin(x, y);
    if (hi == -INFINITY) return -INFINITY;
    return hi + log1p(exp(lo - hi));
}

// the work-group's rows of x to out as bits, consecutive lanes on consecutive addresses: rows r0 .. r0 + THREADS of b are
// one contiguous piece of [b][d].  The caller synchronises before a row's thread overwrites what another lane copied.
template <int THREADS>
__device__ __forceinline__ void copy_rows(const uint32_t *x, uint32_t *out, int64_t b, int d) {
    const int64_t r0 = (int64_t)blockIdx.x * THREADS;
    const int64_t rows = b - r0 < THREADS ? b - r0 : THREADS;
    const int64_t e0 = r0 * d, n = rows * d;
    for (int64_t e = threadIdx.x; e < n; e += THREADS) out[e0 + e] = x[e0 + e];
}

// ---- a tree: one thread per row, codes as q[col * B], the pass's state as t[(2 j + l) * B] ------------------------------
struct Leaf {
    int d;
    const int32_t *col, *bfs, *parent, *child_off, *child_idx;
    const float *params;
};

// the tables of a cutset network in the order of the entry points' arguments, and the levels they declare
struct Net {
    const int32_t *node_col, *node_child;
    const double *node_logw;
    const int32_t *leaf_meta, *leaf_ints;
    const float *leaf_params;
    int levels;
};

__device__ __forceinline__ Leaf leaf_of(const Net &net, int l) {
    const int32_t *m = net.leaf_meta + 3 * (int64_t)l;
    const int d = m[0];
    const int32_t *ints = net.leaf_ints + m[1];
    return {d, ints, ints + d, ints + 2 * d, ints + 3 * d, ints + 4 * d + 1, net.leaf_params + m[2]};
}

// s += params[i][x_parent(i)][x_i] over the tree's positions in order; false (and s unspecified) if an entry is missing.
// COLS = false: a stand-alone tree, position i is column i and f.col is unused.  A leaf of a network leaves at the first
// missing entry (most of the leaves a row with NaN visits hold one); the stand-alone tree, whose complete rows are the
// case that counts, has no exit inside the loop, so that the loads of successive positions overlap (measured on 784
// columns: 1.14 ms against 1.33 ms with the exit).
template <bool COLS = true>
__device__ __forceinline__ bool leaf_gather(const Leaf &f, const uint8_t *q, int64_t B, double &s) {
    bool whole = true;
    for (int i = 0; i < f.d; ++i) {
        const int pa = f.parent[i];
        const int ci = q[(int64_t)(COLS ? f.col[i] : i) * B], cp = pa < 0 ? 0 : q[(int64_t)(COLS ? f.col[pa] : pa) * B];
        if (ci != DPC_MISSING && cp != DPC_MISSING) s += (double)f.params[i * 4 + cp * 2 + ci];
        else if (COLS) return false;
        else whole = false;
    }
    return whole;
}

__device__ __forceinline__ void leaf_pull(const Leaf &f, const float *t, int64_t B, int j, float &m0, float &m1) {
    m0 = 0.f;
    m1 = 0.f;
    const int e1 = f.child_off[j + 1];
    for (int e = f.child_off[j]; e < e1; ++e) {
        const int64_t c = f.child_idx[e];
        m0 += t[2 * c * B];
        m1 += t[(2 * c + 1) * B];
    }
}

// the upward pass of dpc_clt_log_likelihood (R = lse) or of dpc_clt_mpe (MAX: R = max) over the tree's columns, in two
// parts: the messages t_j of every node but the root, children before parents, and the root's value, which is the log
// likelihood (a query that only goes back down never asks for it).  COLS as in leaf_gather.
// TB: the stride of the state t, where it is not the stride B of the codes (dpc_mix_log_likelihood gathers its rows
// through an index: the codes keep the stride of the whole batch, the state has that of the rows evaluated).
template <bool MAX, bool COLS = true>
__device__ void leaf_messages(const Leaf &f, const uint8_t *q, int64_t B, float *t, int64_t TB) {
    for (int p = f.d - 1; p >= 1; --p) {
        const int j = f.bfs[p];
        const float *pj = f.params + j * 4;
        const int cj = q[(int64_t)(COLS ? f.col[j] : j) * B];
        float m0, m1;
        leaf_pull(f, t, TB, j, m0, m1);
        float t0, t1;
        if (cj != DPC_MISSING) {
            const float m = cj ? m1 : m0;
            t0 = pj[cj] + m;
            t1 = pj[2 + cj] + m;
        } else if (MAX) {
            t0 = fmaxf(pj[0] + m0, pj[1] + m1);
            t1 = fmaxf(pj[2] + m0, pj[3] + m1);
        } else {
            t0 = lse2(pj[0] + m0, pj[1] + m1);
            t1 = lse2(pj[2] + m0, pj[3] + m1);
        }
        t[2 * (int64_t)j * TB] = t0;
        t[(2 * (int64_t)j + 1) * TB] = t1;
    }
}

template <bool MAX, bool COLS = true>
__device__ __forceinline__ void leaf_messages(const Leaf &f, const uint8_t *q, int64_t B, float *t) {
    leaf_messages<MAX, COLS>(f, q, B, t, B);
}

template <bool MAX, bool COLS = true>
__device__ __forceinline__ float leaf_root(const Leaf &f, const uint8_t *q, int64_t B, const float *t, int64_t TB) {
    const int j = f.bfs[0];
    const float *pj = f.params + j * 4;
    const int cj = q[(int64_t)(COLS ? f.col[j] : j) * B];
    float m0, m1;
    leaf_pull(f, t, TB, j, m0, m1);
    if (cj != DPC_MISSING) return pj[cj] + (cj ? m1 : m0);
    return MAX ? fmaxf(pj[0] + m0, pj[1] + m1) : lse2(pj[0] + m0, pj[1] + m1);
}

template <bool MAX, bool COLS = true>
__device__ __forceinline__ float leaf_root(const Leaf &f, const uint8_t *q, int64_t B, const float *t) {
    return leaf_root<MAX, COLS>(f, q, B, t, B);
}

template <bool MAX, bool COLS = true>
__device__ __forceinline__ float leaf_upward(const Leaf &f, const uint8_t *q, int64_t B, float *t) {
    leaf_messages<MAX, COLS>(f, q, B, t);
    return leaf_root<MAX, COLS>(f, q, B, t);
}

// dpc_clt_log_likelihood for one row of a stand-alone tree, which dpc_mix_log_likelihood evaluates per component: the
// gather path for a complete row, else the pulled upward pass with R = lse (state t of stride TB).  t may be null where
// the caller has no state to give (dpc_mix_log_likelihood without `work`): a row with NaN then gets NaN and writes nothing.
__device__ __forceinline__ float tree_log_likelihood(const Leaf &f, const uint8_t *q, int64_t B, float *t, int64_t TB) {
    double s = 0.0;
    if (leaf_gather<false>(f, q, B, s)) return (float)s;
    if (!t) return NAN;
    leaf_messages<false, false>(f, q, B, t, TB);
    return leaf_root<false, false>(f, q, B, t, TB);
}

// the downward pass of the posterior marginals (dpc_mar_*), after leaf_messages<false>: in `bfs` order the normalised log
// belief b_j takes the slot of t_j (t_j is read here for the last time; the children's t are still whole when j pulls
// them), and sink(column, expf(b_j[1])) is called for every NaN position
template <bool COLS, typename Sink>
__device__ __forceinline__ void leaf_beliefs(const Leaf &f, const uint8_t *q, int64_t B, float *t, Sink sink) {
    for (int p = 0; p < f.d; ++p) {
        const int64_t j = f.bfs[p];
        const int64_t pa = f.parent[j];
        const int col = COLS ? f.col[j] : (int)j;
        const int cj = q[(int64_t)col * B];
        const float *pj = f.params + j * 4;
        float m0, m1;
        leaf_pull(f, t, B, (int)j, m0, m1);
        const float e0 = cj == 1 ? -INFINITY : 0.f, e1 = cj == 0 ? -INFINITY : 0.f;
        float a0, a1;
        if (pa < 0) {
            a0 = pj[0] + m0 + e0;
            a1 = pj[1] + m1 + e1;
        } else {
            const float bp0 = t[2 * pa * B], bp1 = t[(2 * pa + 1) * B];
            const float c0 = bp0 == -INFINITY ? -INFINITY : bp0 - t[2 * j * B];
            const float c1 = bp1 == -INFINITY ? -INFINITY : bp1 - t[(2 * j + 1) * B];
            a0 = lse2(c0 + pj[0], c1 + pj[2]) + m0 + e0;
            a1 = lse2(c0 + pj[1], c1 + pj[3]) + m1 + e1;
        }
        const float z = lse2(a0, a1);
        const float b1 = a1 - z;
        t[2 * j * B] = a0 - z;
        t[(2 * j + 1) * B] = b1;
        if (cj == DPC_MISSING) sink(col, expf(b1));
    }
}

// ---- the walk of a cutset network's OR tree ----------------------------------------------------------------------------
// One row, depth first, with an explicit stack ns[depth * B] of at most `levels` entries.  An entry is 4 * node + state:
// 0 = new, 1 = NaN, left child running, 2 = NaN, right child running, 3 = observed, its one child running.  What a query
// computes is its visitor's business; depth * B is the slot of the node in the visitor's own [levels][b] scratch:
//     v.leaf(k, depth)             node k is a leaf (its tree: leaf_of(net, net.node_child[2 * k]))
//     v.left_done(k, depth)        the left side of the NaN node k has returned, the right side is about to start
//     v.descend(k, side, depth)    the walk goes down to child `side` of k, whose slot will be depth + 1
//     v.both_done(k, col, depth)   the right side of the NaN node k, of column col, has returned
//     v.one_done(k, c, depth)      the one side c of the observed node k has returned
// False if the tables are deeper than `levels`: the walk stops before it writes past the stack, the visitor's scratch is
// then half used and the caller writes its own NaN answer.
template <typename Visitor>
__device__ __forceinline__ bool or_walk(const Net &net, const uint8_t *q, int64_t B, int32_t *ns, Visitor &v) {
    int depth = 0;
    ns[0] = 0;
    while (depth >= 0) {
        const int enc = ns[depth * B], k = enc >> 2, st = enc & 3;
        const int col = net.node_col[k];
        if (col < 0) {
            v.leaf(k, depth);
            --depth;
            continue;
        }
        const int c = q[(int64_t)col * B];
        if (st == 0 || st == 1) {
            if (depth + 1 >= net.levels) return false;
            int side;
            if (st == 1) {
                v.left_done(k, depth);
                ns[depth * B] = 4 * k + 2;
                side = 1;
            } else if (c != DPC_MISSING) {
                ns[depth * B] = 4 * k + 3;
                side = c;
            } else {
                ns[depth * B] = 4 * k + 1;
                side = 0;
            }
            v.descend(k, side, depth);
            const int next = net.node_child[2 * k + side];
            ++depth;
            ns[depth * B] = 4 * next;
        } else if (st == 2) {
            v.both_done(k, col, depth);
            --depth;
        } else {
            v.one_done(k, c, depth);
            --depth;
        }
    }
    return true;
}

// the value of a tree under the row's evidence: the gather path where nothing of it is missing, else the upward pass
template <bool MAX>
__device__ __forceinline__ double leaf_value(const Leaf &f, const uint8_t *q, int64_t B, float *t) {
    double s = 0.0;
    return leaf_gather(f, q, B, s) ? (double)(float)s : (double)leaf_upward<MAX>(f, q, B, t);
}

// The log likelihood: `ret` is the value the node just left returned, in float64; val [levels][b], t [2 max_leaf_d][b].
struct ValueVisitor {
    const Net &net;
    const uint8_t *q;
    int64_t B;
    double *val;
    float *t;
    double ret;

    __device__ __forceinline__ void leaf(int k, int) { ret = leaf_value<false>(leaf_of(net, net.node_child[2 * k]), q, B, t); }
    __device__ __forceinline__ void left_done(int k, int depth) { val[depth * B] = net.node_logw[2 * k] + ret; }
    __device__ __forceinline__ void descend(int, int, int) {}
    __device__ __forceinline__ void both_done(int k, int, int depth) {
        ret = lse64(val[depth * B], net.node_logw[2 * k + 1] + ret);
    }
    __device__ __forceinline__ void one_done(int k, int c, int) { ret = net.node_logw[2 * k + c] + ret; }
};

// the checks every network query makes of its arguments, in this order; `pointers`: whether the entry point's own
// pointers (all but node_logw, which a network of one node may leave out) are there
inline int check_net(const char *what, int64_t b, int d, int n_nodes, int levels, int max_leaf_d, bool pointers,
                     const double *node_logw, const void *work) {
    DPC_REQUIRE(d >= 1 && d <= DPC_MAX_D, "%s: d = %d is outside 1..%d", what, d, DPC_MAX_D);
    DPC_REQUIRE(b >= 0 && b <= kMaxGridX, "%s: b = %lld is out of domain", what, (long long)b);
    DPC_REQUIRE(n_nodes >= 1 && n_nodes < (1 << 29), "%s: n_nodes = %d is outside 1..2^29-1", what, n_nodes);
    DPC_REQUIRE(levels >= 1 && levels <= d + 1, "%s: levels = %d is outside 1..d+1", what, levels);
    DPC_REQUIRE(max_leaf_d >= 1 && max_leaf_d <= d, "%s: max_leaf_d = %d is outside 1..d", what, max_leaf_d);
    DPC_REQUIRE(pointers, "%s: null pointer", what);
    DPC_REQUIRE(node_logw || n_nodes == 1, "%s: null pointer (node_logw)", what);
    DPC_REQUIRE(((uintptr_t)work & 7) == 0, "%s: work is not 8-byte aligned", what);
    return DPC_OK;
}

}  // namespace dpc_detail
