// libdeeprob_clt.so: binary Chow-Liu trees (include/deeprob_clt.h).  Built with -ffp-contract=off: the float32
// expressions of the queries are evaluated operation by operation, in the order the header states, so that a host
// restatement in the same order reproduces them up to the rounding of expf / log1pf.
//
// Layout of the work.  Learning: the data become bit planes (one 64 x 64 tile of x per work-group, transposed through
// LDS, a ballot per column: pack_tile of clt_common.h), then work-groups tile the (i, j) pairs 32 x 32, stage 32 words of
// each plane in LDS and add popcounts in registers; only tiles on or above the diagonal are computed, each writes its
// mirror image too (pair_tile of clt_common.h, which the cutset learners' kernels in cnet.hip and cut.hip call too).  Queries:
// one thread per row over column-major codes, the row's 2 D floats of state in `work` as [2 D][B], so that the lanes of
// a wave read and write consecutive addresses and the tree tables are wave-uniform loads; the passes over the tree are the
// Leaf functions of clt_common.h, which the leaves of a cutset network and the marginals use too.
#include "clt_common.h"

namespace {

using dpc_detail::Leaf;
using dpc_detail::leaf_messages;
using dpc_detail::leaf_pull;
using dp_device::counter_uniform;

typedef unsigned long long u64;
using dpc_detail::kMaxGridX;
using dpc_detail::kPackThreads;
using dpc_detail::kPairThreads;
using dpc_detail::kPairTile;
using dpc_detail::pack_tile;
using dpc_detail::pair_tile;
constexpr int kThreads = 256;
constexpr int kTile = dpc_detail::kPackTile;      // rows and columns of x per packing work-group
constexpr int kRowThreads = 64;    // query rows per work-group: one wave, so that few rows still spread over the CUs

// ---- packing ---------------------------------------------------------------------------------------------------------
// One work-group per 64 rows x 64 columns of x: line rr of the tile is row r0 + rr.
__global__ __launch_bounds__(kPackThreads) void pack_bits_kernel(const float *__restrict__ x, int64_t n, int d,
                                                                 int64_t n_words, u64 *__restrict__ planes) {
    const int64_t word = blockIdx.x, r0 = word * kTile;
    pack_tile([&](int rr, int c) { return (r0 + rr < n && c < d) ? x[(r0 + rr) * d + c] : 0.f; }, word, d, n_words, planes);
}

__global__ __launch_bounds__(kThreads) void pack_query_kernel(const float *__restrict__ x, int64_t b, int d,
                                                              uint8_t *__restrict__ codes) {
    __shared__ uint8_t tile[kTile][kTile + 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * kTile;
    const int c0 = blockIdx.y * kTile;
    for (int rr = wave; rr < kTile; rr += kThreads / 64) {
        const int64_t r = r0 + rr;
        const int c = c0 + lane;
        uint8_t code = 0;
        if (r < b && c < d) {
            const float v = x[r * d + c];
            code = (v != v) ? (uint8_t)DPC_MISSING : (v != 0.f ? 1 : 0);
        }
        tile[rr][lane] = code;
    }
    __syncthreads();
    for (int cc = wave; cc < kTile; cc += kThreads / 64) {
        const int c = c0 + cc;
        const int64_t r = r0 + lane;
        if (c < d && r < b) codes[(int64_t)c * b + r] = tile[lane][cc];
    }
}

// ---- pair counts -----------------------------------------------------------------------------------------------------
// the whole plane, one matrix (pair_tile of clt_common.h)
__global__ __launch_bounds__(kPairThreads) void pair_counts_kernel(const u64 *__restrict__ planes, int64_t n_words, int d,
                                                                   int32_t *__restrict__ ones) {
    pair_tile<false>(planes, n_words, d, 0, n_words, nullptr, ones);
}

// ---- queries -----------------------------------------------------------------------------------------------------------
enum : int { kLogLikelihood = 0, kMpe = 1, kSample = 2 };

struct QueryArgs {
    const float *x;
    const uint8_t *codes;
    int64_t b;
    int d;
    const int32_t *bfs, *parent;
    const float *params;
    const int32_t *child_off, *child_idx;
    u64 seed;
    int64_t row0;
    float *work, *out;
};

// The tree's passes are those of a leaf of a cutset network (clt_common.h) with position j as column j.
template <int MODE>
__global__ __launch_bounds__(kRowThreads) void query_kernel(const QueryArgs a) {
    const int64_t r = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
    if (r >= a.b) return;
    const int64_t B = a.b;
    const int D = a.d;
    const uint8_t *q = a.codes + r;     // q[j * B]
    float *t = a.work + r;              // t[(2 j + l) * B]
    const Leaf f = {D, nullptr, a.bfs, a.parent, a.child_off, a.child_idx, a.params};

    if (MODE == kLogLikelihood) {
        a.out[r] = dpc_detail::tree_log_likelihood(f, q, B, t, B);
        return;
    }

    // upward: t_j of every node but the root, children before parents
    leaf_messages<MODE == kMpe, false>(f, q, B, t);

    // downward: parents before children.  Once j has its value, t_j is dead (only j's parent pulled it, and that came
    // first): slot 2 j keeps the value for j's children.
    for (int p = 0; p < D; ++p) {
        const int j = a.bfs[p];
        const int pa = a.parent[j];
        const int cj = q[(int64_t)j * B];
        const int xp = pa < 0 ? 0 : (int)t[2 * (int64_t)pa * B];
        float value;
        int v;
        if (cj != DPC_MISSING) {
            v = cj;
            value = a.x[r * D + j];
        } else {
            const float *pj = a.params + j * 4 + xp * 2;
            float m0, m1;
            leaf_pull(f, t, B, j, m0, m1);
            if (MODE == kMpe) {
                v = (pj[1] + m1) > (pj[0] + m0);
            } else {
                const float prob = expf(pj[1] + (pa < 0 ? m1 : (xp ? m1 : m0)));
                v = counter_uniform(a.seed, (u64)(a.row0 + r) * (u64)D + (u64)j) < prob;
            }
            value = (float)v;
        }
        a.out[r * D + j] = value;
        t[2 * (int64_t)j * B] = (float)v;
    }
}

int check_query(const char *what, const void *x, bool needs_x, const QueryArgs &a) {
    DPC_REQUIRE(a.d >= 1 && a.d <= DPC_MAX_D, "%s: d = %d is outside 1..%d", what, a.d, DPC_MAX_D);
    DPC_REQUIRE(a.b >= 0 && a.b <= kMaxGridX, "%s: b = %lld is out of domain", what, (long long)a.b);
    DPC_REQUIRE(a.codes && a.bfs && a.parent && a.params && a.child_off && a.work && a.out && (x || !needs_x),
                "%s: null pointer", what);
    DPC_REQUIRE(a.child_idx || a.d == 1, "%s: null pointer (child_idx)", what);
    return DPC_OK;
}

template <int MODE>
int launch_query(const char *what, const QueryArgs &a, void *stream) {
    if (a.b == 0) return DPC_OK;
    const unsigned grid = (unsigned)((a.b + kRowThreads - 1) / kRowThreads);
    DPC_LAUNCH(what, query_kernel<MODE>, dim3(grid), dim3(kRowThreads), 0, (hipStream_t)stream, a);
    return DPC_OK;
}

}  // namespace

extern "C" {

const char *dpc_last_error(void) { return dpc_detail::g_error; }

int dpc_abi_version(void) { return 6; }

int dpc_pack_bits(const float *x, int64_t n, int d, uint64_t *planes, void *stream) {
    DPC_REQUIRE(d >= 1 && d <= DPC_MAX_D, "dpc_pack_bits: d = %d is outside 1..%d", d, DPC_MAX_D);
    DPC_REQUIRE(n >= 1 && n < 2147483648ll, "dpc_pack_bits: n = %lld is outside 1..2^31-1", (long long)n);
    DPC_REQUIRE(x && planes, "dpc_pack_bits: null pointer");
    const int64_t n_words = (n + 63) / 64;
    DPC_LAUNCH("dpc_pack_bits", pack_bits_kernel, dim3((unsigned)n_words, (unsigned)((d + kTile - 1) / kTile)),
               dim3(kPackThreads), 0, (hipStream_t)stream, x, n, d, n_words, (u64 *)planes);
    return DPC_OK;
}

int dpc_pack_query(const float *x, int64_t b, int d, uint8_t *codes, void *stream) {
    DPC_REQUIRE(d >= 1 && d <= DPC_MAX_D, "dpc_pack_query: d = %d is outside 1..%d", d, DPC_MAX_D);
    DPC_REQUIRE(b >= 0 && b <= kMaxGridX, "dpc_pack_query: b = %lld is out of domain", (long long)b);
    DPC_REQUIRE(x && codes, "dpc_pack_query: null pointer");
    if (b == 0) return DPC_OK;
    DPC_LAUNCH("dpc_pack_query", pack_query_kernel, dim3((unsigned)((b + kTile - 1) / kTile), (unsigned)((d + kTile - 1) / kTile)),
               dim3(kThreads), 0, (hipStream_t)stream, x, b, d, codes);
    return DPC_OK;
}

int dpc_pair_counts(const uint64_t *planes, int64_t n_words, int d, int32_t *ones, void *stream) {
    DPC_REQUIRE(d >= 1 && d <= DPC_MAX_D, "dpc_pair_counts: d = %d is outside 1..%d", d, DPC_MAX_D);
    DPC_REQUIRE(n_words >= 1 && n_words <= (1ll << 25), "dpc_pair_counts: n_words = %lld is outside 1..2^25 (n < 2^31)",
                (long long)n_words);
    DPC_REQUIRE(planes && ones, "dpc_pair_counts: null pointer");
    const unsigned nt = (unsigned)((d + kPairTile - 1) / kPairTile);
    DPC_LAUNCH("dpc_pair_counts", pair_counts_kernel, dim3(nt, nt), dim3(kPairThreads), 0, (hipStream_t)stream,
               (const u64 *)planes, n_words, d, ones);
    return DPC_OK;
}

int dpc_clt_log_likelihood(const uint8_t *codes, int64_t b, int d, const int32_t *bfs, const int32_t *parent,
                           const float *params, const int32_t *child_off, const int32_t *child_idx, float *work,
                           float *out, void *stream) {
    const QueryArgs a = {nullptr, codes, b, d, bfs, parent, params, child_off, child_idx, 0ull, 0, work, out};
    if (int rc = check_query("dpc_clt_log_likelihood", nullptr, false, a)) return rc;
    return launch_query<kLogLikelihood>("dpc_clt_log_likelihood", a, stream);
}

int dpc_clt_mpe(const float *x, const uint8_t *codes, int64_t b, int d, const int32_t *bfs, const int32_t *parent,
                const float *params, const int32_t *child_off, const int32_t *child_idx, float *work, float *out,
                void *stream) {
    const QueryArgs a = {x, codes, b, d, bfs, parent, params, child_off, child_idx, 0ull, 0, work, out};
    if (int rc = check_query("dpc_clt_mpe", x, true, a)) return rc;
    return launch_query<kMpe>("dpc_clt_mpe", a, stream);
}

int dpc_clt_sample(const float *x, const uint8_t *codes, int64_t b, int d, const int32_t *bfs, const int32_t *parent,
                   const float *params, const int32_t *child_off, const int32_t *child_idx, uint64_t seed, int64_t row0,
                   float *work, float *out, void *stream) {
    const QueryArgs a = {x, codes, b, d, bfs, parent, params, child_off, child_idx, (u64)seed, row0, work, out};
    if (int rc = check_query("dpc_clt_sample", x, true, a)) return rc;
    DPC_REQUIRE(row0 >= 0, "dpc_clt_sample: row0 = %lld is negative", (long long)row0);
    return launch_query<kSample>("dpc_clt_sample", a, stream);
}

}  // extern "C"
