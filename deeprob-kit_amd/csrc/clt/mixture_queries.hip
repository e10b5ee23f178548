// libdeeprob_clt.so, the posterior queries of a mixture of Chow-Liu trees (the dpc_mixq_* entry points of
// include/deeprob_clt.h, last section): posterior marginals, conditional sampling and max-product MPE, one launch each.
// Built with -ffp-contract=off like its neighbours: every floating-point expression is evaluated operation by operation
// in the order the header states.
//
// Layout of the work.  One thread per row, one wave per work-group, scratch as [slot][b] so that the lanes of a wave read
// and write consecutive addresses.  The wave first copies its 64 rows of x to `out` (copy_rows); after that a thread
// touches `out` only where its row had NaN.  The trees are visited ONE AT A TIME, in increasing k, through one [2 d] float
// message table per row: the loop over the components is wave uniform, so the tables of tree k are scalar loads for every
// lane, and a lane that has no use for tree k (its weight in the row's posterior is zero, or the row chose another
// component) sits the pass out under the execution mask.  The first loop keeps a_k = logw[k] + V_k of every component in
// float64 (val [K][b]); the mixture level -- M, S, T, pi_k -- is float64 arithmetic on those K numbers.  A tree that is
// needed again is passed again: the marginals run the messages of every tree with pi_k > 0 a second time and follow them
// with the downward pass of dpc_mar_clt, which adds pi_k * mu_k into the row's d float64 accumulators; the fills run the
// messages of the ONE component of the row again and fill its NaN columns parents first.  Scratch does not grow with
// K * d.  No atomics, and no work-group waits on another.
#include "clt_common.h"

namespace {

using dpc_detail::kMaxGridX;
using dpc_detail::Leaf;
using dpc_detail::leaf_beliefs;
using dpc_detail::leaf_gather;
using dpc_detail::leaf_messages;
using dpc_detail::leaf_pull;
using dpc_detail::leaf_root;
using dpc_detail::lse2;
using dp_device::counter_uniform;

typedef unsigned long long u64;
constexpr int kRowThreads = 64;
constexpr uint32_t kNanBits = 0x7FC00000u;

enum : int { kMarginals = 0, kSample = 1, kMpe = 2 };

struct MixqArgs {
    const uint32_t *x;      // the rows as bits: observed entries come back bit for bit
    const uint8_t *codes;
    int64_t b;
    int d, n_comp;
    const int32_t *bfs, *parent;
    const float *params;
    const int32_t *child_off, *child_idx;
    const float *logw;
    u64 seed;
    int64_t row0;
    double *val;            // [n_comp][b]: a_k
    double *acc;            // [d][b], the marginals only
    float *t;               // [2 d][b]
    uint32_t *out;
    int32_t *component;
};

__device__ __forceinline__ Leaf tree_of(const MixqArgs &a, int k) {
    const int64_t D = a.d;
    return {a.d, nullptr, a.bfs + k * D, a.parent + k * D, a.child_off + k * (D + 1), a.child_idx + k * (D - 1),
            a.params + k * D * 4};
}

// V_k: the value dpc_clt_log_likelihood gives the tree (MAX: the same with R = max).  `missing` is what leaf_gather would
// find out: every column is a position of every tree, so a row holds NaN for all components or for none.
template <bool MAX>
__device__ __forceinline__ float tree_value(const Leaf &f, const uint8_t *q, int64_t B, float *t, bool missing) {
    if (!missing) {
        double s = 0.0;
        leaf_gather<false>(f, q, B, s);
        return (float)s;
    }
    leaf_messages<MAX, false>(f, q, B, t);
    return leaf_root<MAX, false>(f, q, B, t);
}

// the NaN columns of the row filled from tree f, parents before children, after the tree's messages.  Once j has its
// value, t_j is dead (only j's parent pulled it, and that came first): slot 2 j keeps the value for j's children.
template <int MODE>
__device__ __forceinline__ void fill_row(const MixqArgs &a, const Leaf &f, const uint8_t *q, int64_t B, float *t, uint32_t *o,
                                         u64 ctr0) {
    leaf_messages<MODE == kMpe, false>(f, q, B, t);
    for (int p = 0; p < f.d; ++p) {
        const int j = f.bfs[p];
        const int pa = f.parent[j];
        const int cj = q[(int64_t)j * B];
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
                v = counter_uniform(a.seed, ctr0 + 1ull + (u64)j) < p1;
            }
            o[j] = __float_as_uint((float)v);
        }
        t[2 * (int64_t)j * B] = (float)v;
    }
}

template <int MODE>
__global__ __launch_bounds__(kRowThreads) void mixq_kernel(const MixqArgs a) {
    const int64_t B = a.b;
    const int D = a.d, K = a.n_comp;
    dpc_detail::copy_rows<kRowThreads>(a.x, a.out, B, D);
    __syncthreads();        // a row's thread overwrites what another lane copied
    const int64_t r = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
    if (r >= B) return;
    const uint8_t *q = a.codes + r;
    bool missing = false;
    for (int i = 0; i < D; ++i) missing = missing || q[(int64_t)i * B] == DPC_MISSING;
    if (MODE == kMarginals && !missing) return;     // a copy
    float *t = a.t + r;
    double *val = a.val + r;
    uint32_t *o = a.out + r * D;

    // a_k of every component, their maximum and the smallest k that attains it
    double top = -INFINITY;
    int best = 0;
    for (int k = 0; k < K; ++k) {
        const double ak = (double)a.logw[k] + (double)tree_value<MODE == kMpe>(tree_of(a, k), q, B, t, missing);
        val[k * B] = ak;
        if (k == 0 || ak > top) {
            top = ak;
            best = k;
        }
    }
    if (!(top > -INFINITY)) {       // impossible under every component, or all weights zero
        if (MODE == kMarginals) {
            for (int j = 0; j < D; ++j)
                if (q[(int64_t)j * B] == DPC_MISSING) o[j] = kNanBits;
        } else if (a.component) {
            a.component[r] = -1;
        }
        return;
    }

    int comp = best;
    double total = 0.0;     // T
    if (MODE != kMpe) {
        double sum = 0.0;
        for (int k = 0; k < K; ++k) sum += exp(val[k * B] - top);
        total = top + log(sum);
    }

    if (MODE == kMarginals) {
        double *acc = a.acc + r;
        for (int j = 0; j < D; ++j) acc[(int64_t)j * B] = 0.0;
        for (int k = 0; k < K; ++k) {
            const double pi = exp(val[k * B] - total);
            if (pi > 0.0) {
                const Leaf f = tree_of(a, k);
                leaf_messages<false, false>(f, q, B, t);
                leaf_beliefs<false>(f, q, B, t, [acc, B, pi](int c, float p1) { acc[(int64_t)c * B] += pi * (double)p1; });
            }
        }
        for (int j = 0; j < D; ++j)
            if (q[(int64_t)j * B] == DPC_MISSING) o[j] = __float_as_uint((float)acc[(int64_t)j * B]);
        return;
    }

    const u64 ctr0 = (u64)(a.row0 + r) * (1ull + (u64)D);
    if (MODE == kSample) {
        const double u = (double)counter_uniform(a.seed, ctr0);
        double c = 0.0;
        int last = -1;
        comp = -1;
        for (int k = 0; k < K; ++k) {
            const double pi = exp(val[k * B] - total);
            c += pi;
            if (pi > 0.0) last = k;
            if (comp < 0 && u < c) comp = k;
        }
        if (comp < 0) comp = last;
    }
    if (a.component) a.component[r] = comp;
    if (!missing) return;
    // (the loop is wave uniform, so that the tables of the pass are scalar loads: a lane waits while the others' trees run)
    for (int k = 0; k < K; ++k)
        if (comp == k) fill_row<MODE>(a, tree_of(a, k), q, B, t, o, ctr0);
}

template <int MODE>
int run(const char *what, const float *x, const uint8_t *codes, int64_t b, int d, int n_comp, const int32_t *bfs,
        const int32_t *parent, const float *params, const int32_t *child_off, const int32_t *child_idx, const float *logw,
        uint64_t seed, int64_t row0, void *work, float *out, int32_t *component, void *stream) {
    DPC_REQUIRE(d >= 1 && d <= DPC_MAX_D, "%s: d = %d is outside 1..%d", what, d, DPC_MAX_D);
    DPC_REQUIRE(n_comp >= 1 && n_comp <= DPC_MIX_MAX_K, "%s: n_comp = %d is outside 1..%d (DPC_MIX_MAX_K)", what, n_comp,
                DPC_MIX_MAX_K);
    DPC_REQUIRE(b >= 0 && b <= kMaxGridX, "%s: b = %lld is out of domain", what, (long long)b);
    DPC_REQUIRE(row0 >= 0, "%s: row0 = %lld is negative", what, (long long)row0);
    DPC_REQUIRE(x && codes && bfs && parent && params && child_off && logw && work && out, "%s: null pointer", what);
    DPC_REQUIRE(child_idx || d == 1, "%s: null pointer (child_idx)", what);
    DPC_REQUIRE(((uintptr_t)work & 7) == 0, "%s: work is not 8-byte aligned", what);
    if (b == 0) return DPC_OK;
    char *w = (char *)work;
    const int64_t o_acc = 8 * (int64_t)n_comp * b, o_t = o_acc + (MODE == kMarginals ? 8 * (int64_t)d * b : 0);
    const MixqArgs a = {(const uint32_t *)x, codes, b, d, n_comp, bfs, parent, params, child_off, child_idx, logw, (u64)seed,
                        row0, (double *)w, (double *)(w + o_acc), (float *)(w + o_t), (uint32_t *)out, component};
    DPC_LAUNCH(what, mixq_kernel<MODE>, dim3((unsigned)((b + kRowThreads - 1) / kRowThreads)), dim3(kRowThreads), 0,
               (hipStream_t)stream, a);
    return DPC_OK;
}

}  // namespace

extern "C" {

int dpc_mixq_marginals(const float *x, const uint8_t *codes, int64_t b, int d, int n_comp, const int32_t *bfs,
                       const int32_t *parent, const float *params, const int32_t *child_off, const int32_t *child_idx,
                       const float *logw, void *work, float *out, void *stream) {
    return run<kMarginals>("dpc_mixq_marginals", x, codes, b, d, n_comp, bfs, parent, params, child_off, child_idx, logw, 0, 0,
                           work, out, nullptr, stream);
}

int dpc_mixq_sample(const float *x, const uint8_t *codes, int64_t b, int d, int n_comp, const int32_t *bfs,
                    const int32_t *parent, const float *params, const int32_t *child_off, const int32_t *child_idx,
                    const float *logw, uint64_t seed, int64_t row0, void *work, float *out, int32_t *component, void *stream) {
    return run<kSample>("dpc_mixq_sample", x, codes, b, d, n_comp, bfs, parent, params, child_off, child_idx, logw, seed, row0,
                        work, out, component, stream);
}

int dpc_mixq_mpe(const float *x, const uint8_t *codes, int64_t b, int d, int n_comp, const int32_t *bfs, const int32_t *parent,
                 const float *params, const int32_t *child_off, const int32_t *child_idx, const float *logw, void *work,
                 float *out, int32_t *component, void *stream) {
    return run<kMpe>("dpc_mixq_mpe", x, codes, b, d, n_comp, bfs, parent, params, child_off, child_idx, logw, 0, 0, work, out,
                     component, stream);
}

}  // extern "C"
