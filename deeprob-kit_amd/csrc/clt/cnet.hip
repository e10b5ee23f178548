// libdeeprob_clt.so, the cutset-network part (the dpc_cnet_* entry points of include/deeprob_clt.h).  Built with
// -ffp-contract=off like clt.hip: every floating-point expression is evaluated operation by operation in the order the
// header states.
//
// Layout of the work.  Learning is level synchronous: a generation is every open node of one depth, each with a segment
// of a row-index array.  gather_pack_kernel makes bit planes of the generation's rows through the index, every segment on
// a word boundary (pack_tile of clt_common.h, a tile line taken through `rows`); seg_pair_counts_kernel is the 32 x 32
// pair tile of clt_common.h (pair_tile, the one clt.hip and cut.hip call) with the task on grid.z and the task's words only; the scores are one thread per (task, column) for the conditional entropies and one thread per task for the
// serial sums the header orders; partition_kernel splits a segment by the bits of its cut column, one work-group per task,
// the position of a row from popcounts (no atomics, no scan through memory).  The query is one thread per row: a complete
// row walks one path, a row with NaN walks the OR tree depth first with its stack in `work` (or_walk of clt_common.h).
#include "clt_common.h"

namespace {

using dpc_detail::leaf_gather;
using dpc_detail::leaf_of;
using dpc_detail::Net;
using dpc_detail::or_walk;
using dpc_detail::ValueVisitor;

typedef unsigned long long u64;
using dpc_detail::kMaxGridX;
using dpc_detail::kMaxGridZ;
using dpc_detail::kPackThreads;
using dpc_detail::kPairThreads;
using dpc_detail::kPairTile;
using dpc_detail::pack_tile;
using dpc_detail::pair_tile;
constexpr int kThreads = 256;
constexpr int kTile = dpc_detail::kPackTile;
constexpr int kRowThreads = 64;
constexpr int kScoreThreads = 64;

// ---- gather-pack ---------------------------------------------------------------------------------------------------------
// One work-group per plane word x 64 columns; the word's task is found by bisection of word_off (empty tasks own no word).
__global__ __launch_bounds__(kPackThreads) void gather_pack_kernel(const float *__restrict__ x, int64_t n, int d,
                                                               const int32_t *__restrict__ rows,
                                                               const int32_t *__restrict__ seg_off,
                                                               const int32_t *__restrict__ word_off, int n_tasks,
                                                               int64_t n_words, u64 *__restrict__ planes) {
    const int64_t word = blockIdx.x;
    int lo = 0, hi = n_tasks - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)word_off[mid + 1] <= word) lo = mid + 1; else hi = mid;
    }
    const int64_t p0 = (int64_t)seg_off[lo] + (word - word_off[lo]) * kTile, p_end = seg_off[lo + 1];
    pack_tile(
        [&](int rr, int c) {
            const int64_t p = p0 + rr;
            float v = 0.f;
            if (p < p_end && c < d) {
                const int64_t r = rows[p];
                if (r >= 0 && r < n) v = x[r * d + c];
            }
            return v;
        },
        word, d, n_words, planes);
}

// ---- segmented pair counts -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPairThreads) void seg_pair_counts_kernel(const u64 *__restrict__ planes, int64_t n_words, int d,
                                                                   const int32_t *__restrict__ word_off,
                                                                   int32_t *__restrict__ ones) {
    pair_tile<false>(planes, n_words, d, word_off[blockIdx.z], word_off[blockIdx.z + 1], nullptr,
                     ones + (int64_t)blockIdx.z * d * d);
}

// ---- scores --------------------------------------------------------------------------------------------------------------
// h(c0, c1) = -(c0 ln c0 + c1 ln c1)
__device__ __forceinline__ double entropy2(double c0, double c1) { return -(c0 * log(c0) + c1 * log(c1)); }

// gains[t][i] <- E_i = (c_i / n) H_i,1 + (1 - c_i / n) H_i,0 for an active i (score_select_kernel turns it into the gain).
// ones[t] is symmetric: thread i reads ones[j][i], consecutive over the threads.
__global__ __launch_bounds__(kScoreThreads) void score_entropy_kernel(const int32_t *__restrict__ ones,
                                                                      const int32_t *__restrict__ seg_off,
                                                                      const uint8_t *__restrict__ active, int d, double alpha,
                                                                      double *__restrict__ gains) {
    const int t = blockIdx.y, i = blockIdx.x * kScoreThreads + threadIdx.x;
    if (i >= d) return;
    const int32_t *o = ones + (int64_t)t * d * d;
    const uint8_t *act = active + (int64_t)t * d;
    double *g = gains + (int64_t)t * d;
    if (!act[i]) {
        g[i] = -INFINITY;
        return;
    }
    const double n = (double)(seg_off[t + 1] - seg_off[t]);
    const double ci = (double)o[(int64_t)i * d + i];
    const double den1 = ci + 4.0 * alpha, den0 = (n - ci) + 4.0 * alpha, a2 = 2.0 * alpha;
    double h1 = 0.0, h0 = 0.0;
    int others = 0;
    for (int j = 0; j < d; ++j) {
        if (j == i || !act[j]) continue;
        const double cj = (double)o[(int64_t)j * d + j], oij = (double)o[(int64_t)j * d + i];
        // the four cells of (x_i = a, x_j = b) in exact integers (held exactly by a double)
        const double c11 = oij, c10 = ci - oij, c01 = cj - oij, c00 = ((n - ci) - cj) + oij;
        h1 += entropy2((c10 + a2) / den1, (c11 + a2) / den1);
        h0 += entropy2((c00 + a2) / den0, (c01 + a2) / den0);
        ++others;
    }
    if (others) {
        h1 = h1 / (double)others;
        h0 = h0 / (double)others;
    }
    const double ratio = n > 0.0 ? ci / n : 0.0;
    g[i] = ratio * h1 + (1.0 - ratio) * h0;
}

__global__ __launch_bounds__(kScoreThreads) void score_select_kernel(const int32_t *__restrict__ ones,
                                                                     const int32_t *__restrict__ seg_off,
                                                                     const uint8_t *__restrict__ active, int n_tasks, int d,
                                                                     double alpha, double *__restrict__ gains,
                                                                     double *__restrict__ stats, int32_t *__restrict__ best) {
    const int t = blockIdx.x * kScoreThreads + threadIdx.x;
    if (t >= n_tasks) return;
    const int32_t *o = ones + (int64_t)t * d * d;
    const uint8_t *act = active + (int64_t)t * d;
    double *g = gains + (int64_t)t * d;
    const double n = (double)(seg_off[t + 1] - seg_off[t]);
    double s = 0.0;
    int d_active = 0;
    for (int i = 0; i < d; ++i) {
        if (!act[i]) continue;
        const double p1 = ((double)o[(int64_t)i * d + i] + 2.0 * alpha) / (n + 4.0 * alpha), p0 = 1.0 - p1;
        s += p0 * log(p0) + p1 * log(p1);
        ++d_active;
    }
    const double mean_entropy = d_active ? -s / (double)d_active : 0.0;
    int arg = -1;
    double top = -INFINITY;
    for (int i = 0; i < d; ++i) {
        if (!act[i]) continue;
        const double gain = mean_entropy - g[i];
        g[i] = gain;
        if (arg < 0 || gain > top) {
            arg = i;
            top = gain;
        }
    }
    stats[2 * t] = mean_entropy;
    stats[2 * t + 1] = top;
    best[2 * t] = arg;
    best[2 * t + 1] = arg < 0 ? 0 : o[(int64_t)arg * d + arg];
}

// ---- partition -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 shfl64(u64 v, int src) {
    const unsigned lo = __shfl((unsigned)v, src), hi = __shfl((unsigned)(v >> 32), src);
    return ((u64)hi << 32) | lo;
}

// One work-group per task.  Every wave reads all words of the task's cut plane (64 at a time, one per lane) and keeps the
// count of ones before the current word; wave w places the rows of the words k with k % 4 == w.
__global__ __launch_bounds__(kThreads) void partition_kernel(const u64 *__restrict__ planes, int64_t n_words,
                                                             const int32_t *__restrict__ rows,
                                                             const int32_t *__restrict__ seg_off,
                                                             const int32_t *__restrict__ word_off,
                                                             const int32_t *__restrict__ cut,
                                                             const int32_t *__restrict__ out_off,
                                                             int32_t *__restrict__ rows_out, int32_t *__restrict__ child_n) {
    const int t = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = cut[t];
    if (c < 0) {
        if (threadIdx.x < 2) child_n[2 * t + threadIdx.x] = 0;
        return;
    }
    const int64_t s0 = seg_off[t], n = seg_off[t + 1] - s0;
    const int64_t nw = word_off[t + 1] - word_off[t];
    const u64 *plane = planes + (int64_t)c * n_words + word_off[t];
    int cnt = 0;
    for (int64_t k = lane; k < nw; k += 64) cnt += __popcll(plane[k]);
    for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m);
    const int64_t n_left = n - cnt;
    if (threadIdx.x == 0) {
        child_n[2 * t] = (int32_t)n_left;
        child_n[2 * t + 1] = cnt;
    }
    const int64_t left0 = out_off[t], right0 = left0 + n_left;
    int64_t before = 0;             // ones in the words in front of the current one
    for (int64_t k0 = 0; k0 < nw; k0 += 64) {
        const u64 mine = k0 + lane < nw ? plane[k0 + lane] : 0ull;
        const int steps = nw - k0 < 64 ? (int)(nw - k0) : 64;
        for (int i = 0; i < steps; ++i) {
            const u64 word = shfl64(mine, i);
            if (((k0 + i) & (kThreads / 64 - 1)) == wave) {
                const int64_t p = (k0 + i) * 64 + lane;
                if (p < n) {
                    const int64_t ob = before + __popcll(word & ((1ull << lane) - 1ull));
                    const int64_t dst = ((word >> lane) & 1ull) ? right0 + ob : left0 + (p - ob);
                    rows_out[dst] = rows[s0 + p];
                }
            }
            before += __popcll(word);
        }
    }
}

// ---- query ---------------------------------------------------------------------------------------------------------------
struct CnetArgs {
    const uint8_t *codes;
    int64_t b;
    Net net;
    double *val;        // [levels][b]
    float *t;           // [2 max_leaf_d][b]
    int32_t *ns;        // [levels][b]
    float *out;
};

__global__ __launch_bounds__(kRowThreads) void cnet_query_kernel(const CnetArgs a) {
    const int64_t r = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
    if (r >= a.b) return;
    const int64_t B = a.b;
    const uint8_t *q = a.codes + r;

    {   // a complete row: one path
        int k = 0;
        double s = 0.0;
        bool complete = true;
        for (int col = a.net.node_col[k]; col >= 0; col = a.net.node_col[k]) {
            const int c = q[(int64_t)col * B];
            if (c == DPC_MISSING) {
                complete = false;
                break;
            }
            s += a.net.node_logw[2 * k + c];
            k = a.net.node_child[2 * k + c];
        }
        if (complete && leaf_gather(leaf_of(a.net, a.net.node_child[2 * k]), q, B, s)) {
            a.out[r] = (float)s;
            return;
        }
    }

    // a row with NaN: the walk of clt_common.h; tables that are not a tree of `levels` levels give NaN
    ValueVisitor v = {a.net, q, B, a.val + r, a.t + r, 0.0};
    a.out[r] = or_walk(a.net, q, B, a.ns + r, v) ? (float)v.ret : NAN;
}

}  // namespace

extern "C" {

int dpc_cnet_gather_pack(const float *x, int64_t n, int d, const int32_t *rows, const int32_t *seg_off,
                         const int32_t *word_off, int n_tasks, int64_t n_words, uint64_t *planes, void *stream) {
    DPC_REQUIRE(d >= 1 && d <= DPC_MAX_D, "dpc_cnet_gather_pack: d = %d is outside 1..%d", d, DPC_MAX_D);
    DPC_REQUIRE(n >= 1 && n < 2147483648ll, "dpc_cnet_gather_pack: n = %lld is outside 1..2^31-1", (long long)n);
    DPC_REQUIRE(n_tasks >= 1, "dpc_cnet_gather_pack: n_tasks = %d is not positive", n_tasks);
    DPC_REQUIRE(n_words >= 0 && n_words <= kMaxGridX, "dpc_cnet_gather_pack: n_words = %lld is out of domain",
                (long long)n_words);
    DPC_REQUIRE(x && rows && seg_off && word_off && planes, "dpc_cnet_gather_pack: null pointer");
    if (n_words == 0) return DPC_OK;
    DPC_LAUNCH("dpc_cnet_gather_pack", gather_pack_kernel, dim3((unsigned)n_words, (unsigned)((d + kTile - 1) / kTile)),
               dim3(kPackThreads), 0, (hipStream_t)stream, x, n, d, rows, seg_off, word_off, n_tasks, n_words, (u64 *)planes);
    return DPC_OK;
}

int dpc_cnet_pair_counts(const uint64_t *planes, int64_t n_words, int d, const int32_t *word_off, int n_tasks,
                         int32_t *ones, void *stream) {
    DPC_REQUIRE(d >= 1 && d <= DPC_MAX_D, "dpc_cnet_pair_counts: d = %d is outside 1..%d", d, DPC_MAX_D);
    DPC_REQUIRE(n_tasks >= 1 && n_tasks <= kMaxGridZ, "dpc_cnet_pair_counts: n_tasks = %d is outside 1..%d", n_tasks,
                kMaxGridZ);
    DPC_REQUIRE(n_words >= 0 && n_words <= kMaxGridX, "dpc_cnet_pair_counts: n_words = %lld is out of domain",
                (long long)n_words);
    DPC_REQUIRE((planes || n_words == 0) && word_off && ones, "dpc_cnet_pair_counts: null pointer");
    const unsigned nt = (unsigned)((d + kPairTile - 1) / kPairTile);
    DPC_LAUNCH("dpc_cnet_pair_counts", seg_pair_counts_kernel, dim3(nt, nt, (unsigned)n_tasks), dim3(kPairThreads), 0,
               (hipStream_t)stream, (const u64 *)planes, n_words, d, word_off, ones);
    return DPC_OK;
}

int dpc_cnet_scores(const int32_t *ones, const int32_t *seg_off, const uint8_t *active, int n_tasks, int d, double alpha,
                    double *gains, double *stats, int32_t *best, void *stream) {
    DPC_REQUIRE(d >= 1 && d <= DPC_MAX_D, "dpc_cnet_scores: d = %d is outside 1..%d", d, DPC_MAX_D);
    DPC_REQUIRE(n_tasks >= 1 && n_tasks <= kMaxGridZ, "dpc_cnet_scores: n_tasks = %d is outside 1..%d", n_tasks, kMaxGridZ);
    DPC_REQUIRE(alpha >= 0.0, "dpc_cnet_scores: alpha = %g is negative", alpha);
    DPC_REQUIRE(ones && seg_off && active && gains && stats && best, "dpc_cnet_scores: null pointer");
    DPC_LAUNCH("dpc_cnet_scores", score_entropy_kernel, dim3((unsigned)((d + kScoreThreads - 1) / kScoreThreads), (unsigned)n_tasks),
               dim3(kScoreThreads), 0, (hipStream_t)stream, ones, seg_off, active, d, alpha, gains);
    DPC_LAUNCH("dpc_cnet_scores", score_select_kernel, dim3((unsigned)((n_tasks + kScoreThreads - 1) / kScoreThreads)),
               dim3(kScoreThreads), 0, (hipStream_t)stream, ones, seg_off, active, n_tasks, d, alpha, gains, stats, best);
    return DPC_OK;
}

int dpc_cnet_partition(const uint64_t *planes, int64_t n_words, const int32_t *rows, const int32_t *seg_off,
                       const int32_t *word_off, const int32_t *cut, const int32_t *out_off, int n_tasks,
                       int32_t *rows_out, int32_t *child_n, void *stream) {
    DPC_REQUIRE(n_tasks >= 1 && n_tasks <= kMaxGridX, "dpc_cnet_partition: n_tasks = %d is not positive", n_tasks);
    DPC_REQUIRE(n_words >= 0 && n_words <= kMaxGridX, "dpc_cnet_partition: n_words = %lld is out of domain",
                (long long)n_words);
    DPC_REQUIRE((planes || n_words == 0) && rows && seg_off && word_off && cut && out_off && rows_out && child_n,
                "dpc_cnet_partition: null pointer");
    DPC_LAUNCH("dpc_cnet_partition", partition_kernel, dim3((unsigned)n_tasks), dim3(kThreads), 0, (hipStream_t)stream,
               (const u64 *)planes, n_words, rows, seg_off, word_off, cut, out_off, rows_out, child_n);
    return DPC_OK;
}

int dpc_cnet_log_likelihood(const uint8_t *codes, int64_t b, int d, int n_nodes, const int32_t *node_col,
                            const int32_t *node_child, const double *node_logw, const int32_t *leaf_meta,
                            const int32_t *leaf_ints, const float *leaf_params, int levels, int max_leaf_d, void *work,
                            float *out, void *stream) {
    if (int rc = dpc_detail::check_net("dpc_cnet_log_likelihood", b, d, n_nodes, levels, max_leaf_d,
                                       codes && node_col && node_child && leaf_meta && leaf_ints && leaf_params && work && out,
                                       node_logw, work))
        return rc;
    if (b == 0) return DPC_OK;
    char *w = (char *)work;
    const CnetArgs a = {codes, b, {node_col, node_child, node_logw, leaf_meta, leaf_ints, leaf_params, levels},
                        (double *)w, (float *)(w + 8 * (int64_t)levels * b),
                        (int32_t *)(w + (8 * (int64_t)levels + 8 * (int64_t)max_leaf_d) * b), out};
    DPC_LAUNCH("dpc_cnet_log_likelihood", cnet_query_kernel, dim3((unsigned)((b + kRowThreads - 1) / kRowThreads)),
               dim3(kRowThreads), 0, (hipStream_t)stream, a);
    return DPC_OK;
}

}  // extern "C"
