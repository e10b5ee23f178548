// libdeeprob_clt.so, posterior marginals (the dpc_mar_* entry points of include/deeprob_clt.h): for every NaN entry of a
// row, p(x_j = 1 | the row's observed entries), exact, for a Chow-Liu tree and for a cutset network, one launch each.
// Built with -ffp-contract=off like the other queries: every floating-point expression is evaluated operation by
// operation in the order the header states.
//
// Layout of the work.  One thread per row, one wave per work-group, scratch as [slot][b] so that the lanes of a wave read
// and write consecutive addresses and the tables are wave-uniform loads.
//
// The tree: the wave copies its 64 rows of x to `out` (copy_rows); a row with NaN then runs the messages of
// dpc_clt_log_likelihood and one downward pass (clt_common.h, leaf_beliefs) that turns them into normalised beliefs in
// place, and overwrites its NaN entries of `out`.
//
// The network: a row with NaN walks the OR tree twice with or_walk of clt_common.h.  The first walk is the log
// likelihood (ValueVisitor) and keeps log P(e) in float64.  The second carries the prefix weight of the path down; at a
// leaf it forms pi_l = exp(W_l - log P(e)) and, where the leaf holds NaN columns, runs the leaf's two passes and adds
// pi_l * mu_l to the row's accumulators; every node returns the sum of pi_l below it, which is what a NaN cut variable
// adds to its own accumulator for the right side.  The D accumulators of a row are float64 scratch [d][b]: a leaf's pass
// adds into them with coalesced accesses, once per consistent leaf and NaN column, where `out` at stride D would cost a
// cache line per lane each time and could hold float32 only; the price is 8 D bytes of scratch per row and one scattered
// read per NaN entry when the wave writes its rows out, x and `out` on consecutive addresses.  No atomics, and no
// work-group waits on another.
#include "clt_common.h"

namespace {

using dpc_detail::Leaf;
using dpc_detail::leaf_beliefs;
using dpc_detail::leaf_gather;
using dpc_detail::leaf_of;
using dpc_detail::leaf_messages;
using dpc_detail::leaf_upward;
using dpc_detail::Net;
using dpc_detail::or_walk;
using dpc_detail::kMaxGridX;

constexpr int kRowThreads = 64;
constexpr uint32_t kNanBits = 0x7FC00000u;

__device__ __forceinline__ bool is_nan_bits(uint32_t v) { return (v & 0x7FFFFFFFu) > 0x7F800000u; }

// ---- the tree ----------------------------------------------------------------------------------------------------------
struct TreeArgs {
    const uint32_t *x;      // the rows as bits: observed entries come back bit for bit
    const uint8_t *codes;
    int64_t b;
    int d;
    const int32_t *bfs, *parent;
    const float *params;
    const int32_t *child_off, *child_idx;
    float *work;            // [2 d][b]
    uint32_t *out;
};

__global__ __launch_bounds__(kRowThreads) void clt_marginals_kernel(const TreeArgs a) {
    const int64_t B = a.b;
    const int D = a.d;
    dpc_detail::copy_rows<kRowThreads>(a.x, a.out, B, D);
    __syncthreads();        // a row's thread overwrites what another lane copied
    const int64_t r = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
    if (r >= B) return;
    const uint8_t *q = a.codes + r;
    bool missing = false;
    for (int i = 0; i < D; ++i) missing = missing || q[(int64_t)i * B] == DPC_MISSING;
    if (!missing) return;
    const Leaf f = {D, nullptr, a.bfs, a.parent, a.child_off, a.child_idx, a.params};
    float *t = a.work + r;
    uint32_t *o = a.out + r * D;
    leaf_messages<false, false>(f, q, B, t);
    leaf_beliefs<false>(f, q, B, t, [o](int col, float p1) { o[col] = __float_as_uint(p1); });
}

// ---- the network -------------------------------------------------------------------------------------------------------
struct NetArgs {
    const uint32_t *x;
    const uint8_t *codes;
    int64_t b;
    int d;
    Net net;
    double *val;        // [levels][b]: the value (first walk) or the sum of pi (second walk) the left side returned
    double *pre;        // [levels][b]: the prefix weight of the node on the stack
    double *acc;        // [d][b]
    float *t;           // [2 max_leaf_d][b]
    int32_t *ns;        // [levels][b]
    uint32_t *out;
};

// The second walk: pre[depth * B] is the prefix weight W of the node on the stack, `ret` the sum of pi_l over the
// consistent leaves below the node just left; acc [d][b] takes pi_l * mu_l of every such leaf with NaN columns and, at a NaN
// cut variable, the sum of pi_l of its right side.
struct PrefixVisitor {
    const Net &net;
    const uint8_t *q;
    int64_t B;
    double *val, *pre, *acc;
    float *t;
    double log_pe, ret;

    __device__ __forceinline__ void leaf(int k, int depth) {
        const Leaf f = leaf_of(net, net.node_child[2 * k]);
        const double p = pre[depth * B];
        double s = 0.0;
        if (leaf_gather(f, q, B, s)) {
            ret = exp((p + (double)(float)s) - log_pe);
        } else {
            const double pi = exp((p + (double)leaf_upward<false>(f, q, B, t)) - log_pe);
            if (pi > 0.0)
                leaf_beliefs<true>(f, q, B, t, [acc = acc, B = B, pi](int c, float p1) { acc[(int64_t)c * B] += pi * (double)p1; });
            ret = pi;
        }
    }
    __device__ __forceinline__ void left_done(int, int depth) { val[depth * B] = ret; }
    __device__ __forceinline__ void descend(int k, int side, int depth) {
        pre[(depth + 1) * B] = pre[depth * B] + net.node_logw[2 * k + side];
    }
    __device__ __forceinline__ void both_done(int, int col, int depth) {
        acc[(int64_t)col * B] += ret;
        ret = val[depth * B] + ret;
    }
    __device__ __forceinline__ void one_done(int, int, int) {}
};

__device__ __forceinline__ void fill_nan(const NetArgs &a, int64_t r) {
    for (int c = 0; c < a.d; ++c) a.acc[(int64_t)c * a.b + r] = (double)NAN;
}

// the row's accumulators: p(x_c = 1 | e) for every NaN column c, NaN in all of them for a row that cannot be answered
// (tables that are not a tree of `levels` levels, or evidence of probability zero)
__device__ void net_row(const NetArgs &a, int64_t r) {
    const int64_t B = a.b;
    const uint8_t *q = a.codes + r;
    bool missing = false;
    for (int c = 0; c < a.d; ++c) missing = missing || q[(int64_t)c * B] == DPC_MISSING;
    if (!missing) return;       // nothing of the accumulators is read
    double *acc = a.acc + r;

    dpc_detail::ValueVisitor value = {a.net, q, B, a.val + r, a.t + r, 0.0};
    if (!or_walk(a.net, q, B, a.ns + r, value) || value.ret == -INFINITY) {
        fill_nan(a, r);
        return;
    }
    for (int c = 0; c < a.d; ++c) acc[(int64_t)c * B] = 0.0;

    PrefixVisitor prefix = {a.net, q, B, a.val + r, a.pre + r, acc, a.t + r, value.ret, 0.0};
    prefix.pre[0] = 0.0;
    if (!or_walk(a.net, q, B, a.ns + r, prefix)) fill_nan(a, r);
}

__global__ __launch_bounds__(kRowThreads) void cnet_marginals_kernel(const NetArgs a) {
    const int64_t B = a.b;
    const int D = a.d;
    const int64_t r0 = (int64_t)blockIdx.x * kRowThreads;
    if (r0 + threadIdx.x < B) net_row(a, r0 + threadIdx.x);
    __syncthreads();        // the accumulators of the wave's rows are read by other lanes
    const int64_t rows = B - r0 < kRowThreads ? B - r0 : kRowThreads;
    const int64_t e0 = r0 * D, n = rows * D;
    for (int64_t e = threadIdx.x; e < n; e += kRowThreads) {
        uint32_t v = a.x[e0 + e];
        if (is_nan_bits(v)) {
            const double p1 = a.acc[(e % D) * B + r0 + e / D];
            v = p1 == p1 ? __float_as_uint((float)p1) : kNanBits;
        }
        a.out[e0 + e] = v;
    }
}

}  // namespace

extern "C" {

int dpc_mar_clt(const float *x, const uint8_t *codes, int64_t b, int d, const int32_t *bfs, const int32_t *parent,
                const float *params, const int32_t *child_off, const int32_t *child_idx, float *work, float *out,
                void *stream) {
    DPC_REQUIRE(d >= 1 && d <= DPC_MAX_D, "dpc_mar_clt: d = %d is outside 1..%d", d, DPC_MAX_D);
    DPC_REQUIRE(b >= 0 && b <= kMaxGridX, "dpc_mar_clt: b = %lld is out of domain", (long long)b);
    DPC_REQUIRE(x && codes && bfs && parent && params && child_off && work && out, "dpc_mar_clt: null pointer");
    DPC_REQUIRE(child_idx || d == 1, "dpc_mar_clt: null pointer (child_idx)");
    if (b == 0) return DPC_OK;
    const TreeArgs a = {(const uint32_t *)x, codes, b, d, bfs, parent, params, child_off, child_idx, work, (uint32_t *)out};
    DPC_LAUNCH("dpc_mar_clt", clt_marginals_kernel, dim3((unsigned)((b + kRowThreads - 1) / kRowThreads)), dim3(kRowThreads),
               0, (hipStream_t)stream, a);
    return DPC_OK;
}

int dpc_mar_cnet(const float *x, const uint8_t *codes, int64_t b, int d, int n_nodes, const int32_t *node_col,
                 const int32_t *node_child, const double *node_logw, const int32_t *leaf_meta, const int32_t *leaf_ints,
                 const float *leaf_params, int levels, int max_leaf_d, void *work, float *out, void *stream) {
    if (int rc = dpc_detail::check_net("dpc_mar_cnet", b, d, n_nodes, levels, max_leaf_d,
                                       x && codes && node_col && node_child && leaf_meta && leaf_ints && leaf_params && work && out,
                                       node_logw, work))
        return rc;
    if (b == 0) return DPC_OK;
    char *w = (char *)work;
    const int64_t o_pre = 8 * (int64_t)levels * b, o_acc = 2 * o_pre, o_t = o_acc + 8 * (int64_t)d * b,
                  o_ns = o_t + 8 * (int64_t)max_leaf_d * b;
    const NetArgs a = {(const uint32_t *)x, codes, b, d,
                       {node_col, node_child, node_logw, leaf_meta, leaf_ints, leaf_params, levels}, (double *)w, (double *)(w + o_pre), (double *)(w + o_acc), (float *)(w + o_t),
                       (int32_t *)(w + o_ns), (uint32_t *)out};
    DPC_LAUNCH("dpc_mar_cnet", cnet_marginals_kernel, dim3((unsigned)((b + kRowThreads - 1) / kRowThreads)),
               dim3(kRowThreads), 0, (hipStream_t)stream, a);
    return DPC_OK;
}

}  // extern "C"
