// What the translation units of libdeeprob_clt.so share: the library's instance of the shared entry-point scaffolding
// (error text, checks), lse2 / lse64 of the header's order of operations, the shape of the segmented pair-count tile, and a
// cutset network's leaf: its tables, the gather path and the upward pass (cnet.hip evaluates with them, cnet_queries.hip
// evaluates and then walks back down).  The samplers draw with dp_device::counter_uniform (shared/device.h).
#pragma once
#include "../../../include/deeprob_clt.h"
#define DP_ENTRY_NS dpc_detail
#define DP_ENTRY_ELAUNCH DPC_ELAUNCH
#include "../shared/entry.h"
#include "../shared/device.h"

#define DPC_REQUIRE(cond, ...) DP_REQUIRE(cond, DPC_EINVAL, __VA_ARGS__)
#define DPC_LAUNCH DP_LAUNCH

namespace dpc_detail {

// The segmented pair counts (cnet.hip, cut.hip): a work-group of kPairThreads owns kPairTile x kPairTile variable pairs
// and stages kPairWords plane words of both operands per step; grid.z is the task or the entry.
constexpr int kPairThreads = 256;
constexpr int kPairTile = 32;
constexpr int kPairWords = 32;
constexpr int kMaxGridZ = 65535;
constexpr int64_t kMaxGridX = 2147483647;

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

// ---- a leaf of a cutset network: one thread per row, codes as q[col * B], the pass's state as t[(2 j + l) * B] ----------
struct Leaf {
    int d;
    const int32_t *col, *bfs, *parent, *child_off, *child_idx;
    const float *params;
};

__device__ __forceinline__ Leaf leaf_of(const int32_t *leaf_meta, const int32_t *leaf_ints, const float *leaf_params, int l) {
    const int32_t *m = leaf_meta + 3 * (int64_t)l;
    const int d = m[0];
    const int32_t *ints = leaf_ints + m[1];
    return {d, ints, ints + d, ints + 2 * d, ints + 3 * d, ints + 4 * d + 1, leaf_params + m[2]};
}

// s += params[i][x_parent(i)][x_i] over the leaf's positions in order; false (and s unspecified) if an entry is missing
__device__ __forceinline__ bool leaf_gather(const Leaf &f, const uint8_t *q, int64_t B, double &s) {
    for (int i = 0; i < f.d; ++i) {
        const int pa = f.parent[i];
        const int ci = q[(int64_t)f.col[i] * B], cp = pa < 0 ? 0 : q[(int64_t)f.col[pa] * B];
        if (ci == DPC_MISSING) return false;
        s += (double)f.params[i * 4 + cp * 2 + ci];
    }
    return true;
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

// the upward pass of dpc_clt_log_likelihood (R = lse) or of dpc_clt_mpe (MAX: R = max) over the leaf's columns, ending
// at the root as the log likelihood does.  COLS = false: a stand-alone tree, position j is column j and f.col is unused.
template <bool MAX, bool COLS = true>
__device__ float leaf_upward(const Leaf &f, const uint8_t *q, int64_t B, float *t) {
    for (int p = f.d - 1; p >= 1; --p) {
        const int j = f.bfs[p];
        const float *pj = f.params + j * 4;
        const int cj = q[(int64_t)(COLS ? f.col[j] : j) * B];
        float m0, m1;
        leaf_pull(f, t, B, j, m0, m1);
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
        t[2 * (int64_t)j * B] = t0;
        t[(2 * (int64_t)j + 1) * B] = t1;
    }
    const int j = f.bfs[0];
    const float *pj = f.params + j * 4;
    const int cj = q[(int64_t)(COLS ? f.col[j] : j) * B];
    float m0, m1;
    leaf_pull(f, t, B, j, m0, m1);
    if (cj != DPC_MISSING) return pj[cj] + (cj ? m1 : m0);
    return MAX ? fmaxf(pj[0] + m0, pj[1] + m1) : lse2(pj[0] + m0, pj[1] + m1);
}

// the downward pass of the posterior marginals (dpc_mar_*), after leaf_upward<false>: in `bfs` order the normalised log
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

}  // namespace dpc_detail
