// libdeeprob_clt.so, the queries of a cutset network that fill a row in (the dpc_cnq_* entry points of
// include/deeprob_clt.h): exact MPE and exact conditional sampling, each in one launch.  Built with -ffp-contract=off like
// cnet.hip: every floating-point expression is evaluated operation by operation in the order the header states.
//
// Layout of the work.  One thread per row, one wave per work-group.  The wave first copies its 64 rows of x to `out`
// with consecutive lanes on consecutive addresses; after that a thread touches `out` only where its row had NaN.  The row
// walks the OR tree depth first exactly as cnet_query_kernel does, but every node returns a PAIR: its value and the leaf
// chosen below it (drawn with the posterior odds of the two sides, or the better side).  The stack therefore carries
// one more int32 per level, the leaf the left side returned.  At the root the pair names the leaf of the whole row; the walk
// back up through node_parent fills the NaN cut variables of that one path, and the leaf's own NaN columns are filled
// by one more upward pass of the leaf and the downward pass over it.  Nothing is visited twice on the way down, there
// are no atomics, and no work-group waits on another.  Scratch is [slot][b], so the lanes of a wave read and write
// consecutive addresses.
#include "clt_common.h"

namespace {

using dpc_detail::Leaf;
using dpc_detail::leaf_gather;
using dpc_detail::leaf_of;
using dpc_detail::leaf_pull;
using dpc_detail::leaf_upward;
using dpc_detail::lse2;
using dpc_detail::lse64;
using dp_device::counter_uniform;
using dpc_detail::kMaxGridX;

typedef unsigned long long u64;
constexpr int kRowThreads = 64;

enum : int { kMpe = 0, kSample = 1 };

struct QueryArgs {
    const uint32_t *x;      // the rows as bits: observed entries come back bit for bit
    const uint8_t *codes;
    int64_t b;
    int d, n_nodes;
    const int32_t *node_col, *node_child, *node_parent;
    const double *node_logw;
    const int32_t *leaf_meta, *leaf_ints;
    const float *leaf_params;
    int levels;
    u64 seed;
    int64_t row0;
    double *val;        // [levels][b]
    float *t;           // [2 max_leaf_d][b]
    int32_t *ns;        // [levels][b]
    int32_t *lf;        // [levels][b]: the leaf the left side of a NaN node returned
    uint32_t *out;
    int32_t *choice;
};

template <int MODE>
__global__ __launch_bounds__(kRowThreads) void cnet_fill_kernel(const QueryArgs a) {
    const int64_t B = a.b;
    const int D = a.d;
    {   // the work-group's rows are one contiguous piece of x
        const int64_t r0 = (int64_t)blockIdx.x * kRowThreads;
        const int64_t rows = B - r0 < kRowThreads ? B - r0 : kRowThreads;
        const int64_t e0 = r0 * D, n = rows * D;
        for (int64_t e = threadIdx.x; e < n; e += kRowThreads) a.out[e0 + e] = a.x[e0 + e];
    }
    __syncthreads();        // a row's thread overwrites what another lane copied
    const int64_t r = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
    if (r >= B) return;
    const uint8_t *q = a.codes + r;
    uint32_t *o = a.out + r * D;
    const u64 ctr0 = (u64)(a.row0 + r) * ((u64)a.n_nodes + (u64)D);

    // depth first; a stack entry is 4 * node + state: 0 = new, 1 = NaN, left child running, 2 = NaN, right child
    // running, 3 = observed, its one child running
    double *val = a.val + r;
    int32_t *ns = a.ns + r, *lf = a.lf + r;
    int depth = 0;
    double ret = 0.0;
    int ret_leaf = 0;
    ns[0] = 0;
    while (depth >= 0) {
        const int enc = ns[depth * B], k = enc >> 2, st = enc & 3;
        const int col = a.node_col[k];
        if (col < 0) {
            const Leaf f = leaf_of(a.leaf_meta, a.leaf_ints, a.leaf_params, a.node_child[2 * k]);
            double s = 0.0;
            ret = leaf_gather(f, q, B, s) ? (double)(float)s : (double)leaf_upward<MODE == kMpe>(f, q, B, a.t + r);
            ret_leaf = k;
            --depth;
            continue;
        }
        const int c = q[(int64_t)col * B];
        if (st == 0 || st == 1) {
            if (depth + 1 >= a.levels) {        // the tables are not a tree of `levels` levels: no write past the stack
                const uint32_t nan_bits = 0x7FC00000u;
                for (int j = 0; j < D; ++j) o[j] = nan_bits;
                if (a.choice) a.choice[r] = -1;
                return;
            }
            int next;
            if (st == 1) {
                val[depth * B] = a.node_logw[2 * k] + ret;
                lf[depth * B] = ret_leaf;
                ns[depth * B] = 4 * k + 2;
                next = a.node_child[2 * k + 1];
            } else if (c != DPC_MISSING) {
                ns[depth * B] = 4 * k + 3;
                next = a.node_child[2 * k + c];
            } else {
                ns[depth * B] = 4 * k + 1;
                next = a.node_child[2 * k];
            }
            ++depth;
            ns[depth * B] = 4 * next;
        } else if (st == 2) {
            const double a0 = val[depth * B], a1 = a.node_logw[2 * k + 1] + ret;
            bool right;
            if (MODE == kMpe) {
                right = a1 > a0;
                ret = right ? a1 : a0;
            } else {
                const double t = lse64(a0, a1);
                const double p1 = t == -INFINITY ? 0.0 : exp(a1 - t);
                right = (double)counter_uniform(a.seed, ctr0 + (u64)k) < p1;
                ret = t;
            }
            if (!right) ret_leaf = lf[depth * B];
            --depth;
        } else {
            ret = a.node_logw[2 * k + c] + ret;
            --depth;
        }
    }
    if (a.choice) a.choice[r] = ret_leaf;

    // up from the leaf: a NaN cut variable takes the side the path went (at most levels - 1 steps in a tree of `levels`)
    {
        int k = ret_leaf;
        for (int step = 1; step < a.levels; ++step) {
            const int up = a.node_parent[k];
            if (up < 0) break;
            k = up >> 1;
            const int col = a.node_col[k];
            if (col >= 0 && q[(int64_t)col * B] == DPC_MISSING) o[col] = __float_as_uint((float)(up & 1));
        }
    }

    // the leaf: its upward pass again (the scratch held the last leaf visited), then parents before children.  Once j
    // has its value, t_j is dead (only j's parent pulled it, and that came first): slot 2 j keeps the value for j's children.
    const Leaf f = leaf_of(a.leaf_meta, a.leaf_ints, a.leaf_params, a.node_child[2 * ret_leaf]);
    bool missing = false;
    for (int i = 0; i < f.d; ++i) missing = missing || q[(int64_t)f.col[i] * B] == DPC_MISSING;
    if (!missing) return;
    float *t = a.t + r;
    leaf_upward<MODE == kMpe>(f, q, B, t);
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

int check(const char *what, const QueryArgs &a, int max_leaf_d, const void *work) {
    DPC_REQUIRE(a.d >= 1 && a.d <= DPC_MAX_D, "%s: d = %d is outside 1..%d", what, a.d, DPC_MAX_D);
    DPC_REQUIRE(a.b >= 0 && a.b <= kMaxGridX, "%s: b = %lld is out of domain", what, (long long)a.b);
    DPC_REQUIRE(a.n_nodes >= 1 && a.n_nodes < (1 << 29), "%s: n_nodes = %d is outside 1..2^29-1", what, a.n_nodes);
    DPC_REQUIRE(a.levels >= 1 && a.levels <= a.d + 1, "%s: levels = %d is outside 1..d+1", what, a.levels);
    DPC_REQUIRE(max_leaf_d >= 1 && max_leaf_d <= a.d, "%s: max_leaf_d = %d is outside 1..d", what, max_leaf_d);
    DPC_REQUIRE(a.x && a.codes && a.node_col && a.node_child && a.node_parent && a.leaf_meta && a.leaf_ints && a.leaf_params &&
                    work && a.out,
                "%s: null pointer", what);
    DPC_REQUIRE(a.node_logw || a.n_nodes == 1, "%s: null pointer (node_logw)", what);
    DPC_REQUIRE(((uintptr_t)work & 7) == 0, "%s: work is not 8-byte aligned", what);
    DPC_REQUIRE(a.row0 >= 0, "%s: row0 = %lld is negative", what, (long long)a.row0);
    return DPC_OK;
}

template <int MODE>
int run(const char *what, const float *x, const uint8_t *codes, int64_t b, int d, int n_nodes, const int32_t *node_col,
        const int32_t *node_child, const int32_t *node_parent, const double *node_logw, const int32_t *leaf_meta,
        const int32_t *leaf_ints, const float *leaf_params, int levels, int max_leaf_d, uint64_t seed, int64_t row0,
        void *work, float *out, int32_t *choice, void *stream) {
    char *w = (char *)work;
    // (the offsets are only used after `check`: levels and max_leaf_d are then at most d + 1)
    const int64_t o_t = 8 * (int64_t)levels * b, o_ns = o_t + 8 * (int64_t)max_leaf_d * b, o_lf = o_ns + 4 * (int64_t)levels * b;
    const QueryArgs a = {(const uint32_t *)x, codes, b, d, n_nodes, node_col, node_child, node_parent, node_logw, leaf_meta,
                         leaf_ints, leaf_params, levels, (u64)seed, row0, (double *)w, (float *)(w + o_t),
                         (int32_t *)(w + o_ns), (int32_t *)(w + o_lf), (uint32_t *)out, choice};
    if (int rc = check(what, a, max_leaf_d, work)) return rc;
    if (b == 0) return DPC_OK;
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
