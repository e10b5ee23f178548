// libdeeprob_clt.so, the queries of a cutset network that fill a row in (the dpc_cnq_* entry points of
// include/deeprob_clt.h): exact MPE and exact conditional sampling, each in one launch.  Built with -ffp-contract=off like
// cnet.hip: every floating-point expression is evaluated operation by operation in the order the header states.
//
// Layout of the work.  One thread per row, one wave per work-group.  The wave first copies its 64 rows of x to `out`
// (copy_rows); after that a thread touches `out` only where its row had NaN.  The row walks the OR tree with or_walk of
// clt_common.h, but every node returns a PAIR: its value and the leaf chosen below it (drawn with the posterior odds of
// the two sides, or the better side).  The stack therefore carries one more int32 per level, the leaf the left side
// returned.  At the root the pair names the leaf of the whole row; the walk back up through node_parent fills the NaN cut
// variables of that one path, and the leaf's own NaN columns are filled by the leaf's messages once more and the
// downward pass over them.  Nothing is visited twice on the way down, there are no atomics, and no work-group waits on
// another.  Scratch is [slot][b], so the lanes of a wave read and write consecutive addresses.
#include "clt_common.h"

namespace {

using dpc_detail::Leaf;
using dpc_detail::leaf_messages;
using dpc_detail::leaf_of;
using dpc_detail::leaf_pull;
using dpc_detail::leaf_value;
using dpc_detail::lse2;
using dpc_detail::lse64;
using dpc_detail::Net;
using dpc_detail::or_walk;
using dp_device::counter_uniform;

typedef unsigned long long u64;
constexpr int kRowThreads = 64;

enum : int { kMpe = 0, kSample = 1 };

struct QueryArgs {
    const uint32_t *x;      // the rows as bits: observed entries come back bit for bit
    const uint8_t *codes;
    int64_t b;
    int d, n_nodes;
    Net net;
    const int32_t *node_parent;
    u64 seed;
    int64_t row0;
    double *val;        // [levels][b]
    float *t;           // [2 max_leaf_d][b]
    int32_t *ns;        // [levels][b]
    int32_t *lf;        // [levels][b]: the leaf the left side of a NaN node returned
    uint32_t *out;
    int32_t *choice;
};

// The value and the leaf: `ret` as in ValueVisitor (the maximum in place of the sum for MODE = kMpe), `ret_leaf` the node
// number of the leaf chosen below the node just left.  A NaN node keeps its left side's leaf in lf [levels][b].
template <int MODE>
struct FillVisitor {
    const Net &net;
    const uint8_t *q;
    int64_t B;
    double *val;
    int32_t *lf;
    float *t;
    u64 seed, ctr0;
    double ret;
    int ret_leaf;

    __device__ __forceinline__ void leaf(int k, int) {
        ret = leaf_value<MODE == kMpe>(leaf_of(net, net.node_child[2 * k]), q, B, t);
        ret_leaf = k;
    }
    __device__ __forceinline__ void left_done(int k, int depth) {
        val[depth * B] = net.node_logw[2 * k] + ret;
        lf[depth * B] = ret_leaf;
    }
    __device__ __forceinline__ void descend(int, int, int) {}
    __device__ __forceinline__ void both_done(int k, int, int depth) {
        const double a0 = val[depth * B], a1 = net.node_logw[2 * k + 1] + ret;
        bool right;
        if (MODE == kMpe) {
            right = a1 > a0;
            ret = right ? a1 : a0;
        } else {
            const double t = lse64(a0, a1);
            const double p1 = t == -INFINITY ? 0.0 : exp(a1 - t);
            right = (double)counter_uniform(seed, ctr0 + (u64)k) < p1;
            ret = t;
        }
        if (!right) ret_leaf = lf[depth * B];
    }
    __device__ __forceinline__ void one_done(int k, int c, int) { ret = net.node_logw[2 * k + c] + ret; }
};

template <int MODE>
__global__ __launch_bounds__(kRowThreads) void cnet_fill_kernel(const QueryArgs a) {
    const int64_t B = a.b;
    const int D = a.d;
    dpc_detail::copy_rows<kRowThreads>(a.x, a.out, B, D);
    __syncthreads();        // a row's thread overwrites what another lane copied
    const int64_t r = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
    if (r >= B) return;
    const uint8_t *q = a.codes + r;
    uint32_t *o = a.out + r * D;
    const u64 ctr0 = (u64)(a.row0 + r) * ((u64)a.n_nodes + (u64)D);
    float *t = a.t + r;

    FillVisitor<MODE> pair = {a.net, q, B, a.val + r, a.lf + r, t, a.seed, ctr0, 0.0, 0};
    if (!or_walk(a.net, q, B, a.ns + r, pair)) {    // the tables are not a tree of `levels` levels
        const uint32_t nan_bits = 0x7FC00000u;
        for (int j = 0; j < D; ++j) o[j] = nan_bits;
        if (a.choice) a.choice[r] = -1;
        return;
    }
    const int ret_leaf = pair.ret_leaf;
    if (a.choice) a.choice[r] = ret_leaf;

    // up from the leaf: a NaN cut variable takes the side the path went (at most levels - 1 steps in a tree of `levels`)
    {
        int k = ret_leaf;
        for (int step = 1; step < a.net.levels; ++step) {
            const int up = a.node_parent[k];
            if (up < 0) break;
            k = up >> 1;
            const int col = a.net.node_col[k];
            if (col >= 0 && q[(int64_t)col * B] == DPC_MISSING) o[col] = __float_as_uint((float)(up & 1));
        }
    }

    // the leaf: its messages again (the scratch held the last leaf visited), then parents before children.  Once j has
    // its value, t_j is dead (only j's parent pulled it, and that came first): slot 2 j keeps the value for j's children.
    const Leaf f = leaf_of(a.net, a.net.node_child[2 * ret_leaf]);
    bool missing = false;
    for (int i = 0; i < f.d; ++i) missing = missing || q[(int64_t)f.col[i] * B] == DPC_MISSING;
    if (!missing) return;
    leaf_messages<MODE == kMpe>(f, q, B, t);
    for (int p = 0; p < f.d; ++p) {
        const int j = f.bfs[p];
        const int pa = f.parent[j];
        const int col = f.col[j];
        const int cj = q[(int64_t)col * B];
        int v = cj;
        if (cj == DPC_MISSING) {
            const int xp = pa < 0 ? 0 : (int)t[2 * (int64_t)pa * B];
            const float *pj = f.params + j * 4 + xp * 2;
            float m0, m1;
            leaf_pull(f, t, B, j, m0, m1);
            const float a0 = pj[0] + m0, a1 = pj[1] + m1;
            if (MODE == kMpe) {
                v = a1 > a0;
            } else {
                const float p1 = expf(a1 - lse2(a0, a1));
                v = counter_uniform(a.seed, ctr0 + (u64)a.n_nodes + (u64)col) < p1;
            }
            o[col] = __float_as_uint((float)v);
        }
        t[2 * (int64_t)j * B] = (float)v;
    }
}

template <int MODE>
int run(const char *what, const float *x, const uint8_t *codes, int64_t b, int d, int n_nodes, const int32_t *node_col,
        const int32_t *node_child, const int32_t *node_parent, const double *node_logw, const int32_t *leaf_meta,
        const int32_t *leaf_ints, const float *leaf_params, int levels, int max_leaf_d, uint64_t seed, int64_t row0,
        void *work, float *out, int32_t *choice, void *stream) {
    if (int rc = dpc_detail::check_net(what, b, d, n_nodes, levels, max_leaf_d,
                                       x && codes && node_col && node_child && node_parent && leaf_meta && leaf_ints &&
                                           leaf_params && work && out,
                                       node_logw, work))
        return rc;
    DPC_REQUIRE(row0 >= 0, "%s: row0 = %lld is negative", what, (long long)row0);
    if (b == 0) return DPC_OK;
    char *w = (char *)work;
    const int64_t o_t = 8 * (int64_t)levels * b, o_ns = o_t + 8 * (int64_t)max_leaf_d * b, o_lf = o_ns + 4 * (int64_t)levels * b;
    const QueryArgs a = {(const uint32_t *)x, codes, b, d, n_nodes,
                         {node_col, node_child, node_logw, leaf_meta, leaf_ints, leaf_params, levels}, node_parent, (u64)seed,
                         row0, (double *)w, (float *)(w + o_t), (int32_t *)(w + o_ns), (int32_t *)(w + o_lf), (uint32_t *)out,
                         choice};
    DPC_LAUNCH(what, cnet_fill_kernel<MODE>, dim3((unsigned)((b + kRowThreads - 1) / kRowThreads)), dim3(kRowThreads), 0,
               (hipStream_t)stream, a);
    return DPC_OK;
}

}  // namespace

extern "C" {

int dpc_cnq_mpe(const float *x, const uint8_t *codes, int64_t b, int d, int n_nodes, const int32_t *node_col,
                const int32_t *node_child, const int32_t *node_parent, const double *node_logw, const int32_t *leaf_meta,
                const int32_t *leaf_ints, const float *leaf_params, int levels, int max_leaf_d, void *work, float *out,
                int32_t *choice, void *stream) {
    return run<kMpe>("dpc_cnq_mpe", x, codes, b, d, n_nodes, node_col, node_child, node_parent, node_logw, leaf_meta, leaf_ints,
                     leaf_params, levels, max_leaf_d, 0, 0, work, out, choice, stream);
}

int dpc_cnq_sample(const float *x, const uint8_t *codes, int64_t b, int d, int n_nodes, const int32_t *node_col,
                   const int32_t *node_child, const int32_t *node_parent, const double *node_logw, const int32_t *leaf_meta,
                   const int32_t *leaf_ints, const float *leaf_params, int levels, int max_leaf_d, uint64_t seed, int64_t row0,
                   void *work, float *out, int32_t *choice, void *stream) {
    return run<kSample>("dpc_cnq_sample", x, codes, b, d, n_nodes, node_col, node_child, node_parent, node_logw, leaf_meta,
                        leaf_ints, leaf_params, levels, max_leaf_d, seed, row0, work, out, choice, stream);
}

}  // extern "C"
