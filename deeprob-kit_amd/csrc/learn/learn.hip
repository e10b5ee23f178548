// libdeeprob_learn.so: the statistics of LearnSPN for discrete data, segmented over the tasks of one generation
// (include/deeprob_learn.h).  Built with -ffp-contract=off: the float64 expressions below are evaluated operation by
// operation, in the order the header states, so that a host restatement in the same order reproduces them.
#include "learn_common.h"

namespace {

using dpl_detail::common_ok;
using dpl_detail::kMaxGrid;
using dpl_detail::kThreads;
using dpl_detail::set_error;
constexpr double kEps32 = 1.1920928955078125e-07;   // np.finfo(np.float32).eps (gvs.py:193)

// ---- column counts ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void column_counts_kernel(
    const uint8_t *__restrict__ x, int64_t n_rows, const int32_t *__restrict__ row_index,
    const int32_t *__restrict__ item_col, const int64_t *__restrict__ item_row_off, const int32_t *__restrict__ item_n,
    int kmax, int32_t *__restrict__ counts) {
    __shared__ int cnt[DPL_MAX_K];
    const int64_t item = blockIdx.x;
    if (threadIdx.x < DPL_MAX_K) cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint8_t *col = x + (int64_t)item_col[item] * n_rows;
    const int32_t *rows = row_index + item_row_off[item];
    const int n = item_n[item];
    if (kmax <= 2) {
        // binary data: count the ones in registers, one LDS add per thread
        int ones = 0, seen = 0;
        for (int r = threadIdx.x; r < n; r += kThreads) {
            const int v = col[rows[r]];
            ones += (v == 1);
            seen += (v <= 1);
        }
        if (seen) {
            atomicAdd(&cnt[0], seen - ones);
            if (ones) atomicAdd(&cnt[1], ones);
        }
    } else {
        for (int r = threadIdx.x; r < n; r += kThreads) {
            const int v = col[rows[r]];
            if (v < kmax) atomicAdd(&cnt[v], 1);
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < kmax) counts[item * kmax + threadIdx.x] = cnt[threadIdx.x];
}

// ---- joint counts of a column pair (shared by the G statistic and the maximal correlation) -------------------------------
// joint[a * kj + b] = rows of the segment with (ci, cj) == (a, b), a < ki, b < kj; all kThreads threads call it, and the
// counts are complete for every thread when it returns.
__device__ __forceinline__ void count_joint(int *joint, const uint8_t *__restrict__ ci, const uint8_t *__restrict__ cj,
                                            const int32_t *__restrict__ rows, int n, int ki, int kj) {
    joint[threadIdx.x] = 0;     // (kThreads == DPL_MAX_K * DPL_MAX_K)
    __syncthreads();
    if (ki * kj <= 4) {
        // binary pairs: the (up to) four cells in registers, one LDS add per thread and cell
        int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
        for (int r = threadIdx.x; r < n; r += kThreads) {
            const int row = rows[r];
            const int a = ci[row], b = cj[row];
            const int cell = (a < ki && b < kj) ? a * kj + b : -1;
            c0 += (cell == 0);
            c1 += (cell == 1);
            c2 += (cell == 2);
            c3 += (cell == 3);
        }
        if (c0) atomicAdd(&joint[0], c0);
        if (c1) atomicAdd(&joint[1], c1);
        if (c2) atomicAdd(&joint[2], c2);
        if (c3) atomicAdd(&joint[3], c3);
    } else {
        for (int r = threadIdx.x; r < n; r += kThreads) {
            const int row = rows[r];
            const int a = ci[row], b = cj[row];
            if (a < ki && b < kj) atomicAdd(&joint[a * kj + b], 1);
        }
    }
    __syncthreads();
}

// ---- G statistics ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void pair_g_kernel(
    const uint8_t *__restrict__ x, int64_t n_rows, const int32_t *__restrict__ row_index,
    const int32_t *__restrict__ pair_col_i, const int32_t *__restrict__ pair_col_j, const int64_t *__restrict__ pair_row_off,
    const int32_t *__restrict__ pair_n, const int32_t *__restrict__ pair_ki, const int32_t *__restrict__ pair_kj,
    double *__restrict__ g) {
    __shared__ int joint[DPL_MAX_K * DPL_MAX_K];
    __shared__ double term[DPL_MAX_K * DPL_MAX_K];
    __shared__ double m1[DPL_MAX_K], m2[DPL_MAX_K];
    const int64_t q = blockIdx.x;
    const int ki = pair_ki[q], kj = pair_kj[q], n = pair_n[q], cells = ki * kj;
    count_joint(joint, x + (int64_t)pair_col_i[q] * n_rows, x + (int64_t)pair_col_j[q] * n_rows, row_index + pair_row_off[q], n,
                ki, kj);
    const int t = threadIdx.x;
    if (t < ki) {
        double s = 0.0;
        for (int b = 0; b < kj; ++b) s = (b == 0) ? ((double)joint[t * kj] + kEps32) : s + ((double)joint[t * kj + b] + kEps32);
        m1[t] = s;
    }
    if (t >= 64 && t < 64 + kj) {      // (the second wave: no divergence with the rows above)
        const int b = t - 64;
        double s = 0.0;
        for (int a = 0; a < ki; ++a) s = (a == 0) ? ((double)joint[b] + kEps32) : s + ((double)joint[a * kj + b] + kEps32);
        m2[b] = s;
    }
    __syncthreads();
    if (t < cells) {
        const int a = t / kj, b = t - a * kj;
        const double h = (double)joint[t] + kEps32;
        const double e = m1[a] * m2[b] / (double)n;
        term[t] = h * log(h / e);
    }
    __syncthreads();
    if (t == 0) {
        double s = term[0];
        for (int c = 1; c < cells; ++c) s += term[c];
        g[q] = 2.0 * s;
    }
}

// ---- maximal correlation (the exact value of the RDC score of two discrete columns) ---------------------------------
// The header states the order of operations; tests/rdc_ref.py:maxcorr_jacobi restates it.  Every thread of the block
// forms the three dot products of a rotation itself (broadcast LDS reads, the same sequential order), so every branch
// below is block-uniform and the barriers around the update are reached by all threads or by none.
constexpr double kJacobiTol = 3.552713678800501e-15;    // 2^-48
constexpr int kJacobiSweeps = 30;

__global__ __launch_bounds__(kThreads) void pair_maxcorr_kernel(
    const uint8_t *__restrict__ x, int64_t n_rows, const int32_t *__restrict__ row_index,
    const int32_t *__restrict__ pair_col_i, const int32_t *__restrict__ pair_col_j, const int64_t *__restrict__ pair_row_off,
    const int32_t *__restrict__ pair_n, const int32_t *__restrict__ pair_ki, const int32_t *__restrict__ pair_kj,
    double *__restrict__ score) {
    __shared__ int joint[DPL_MAX_K * DPL_MAX_K];
    __shared__ double w[DPL_MAX_K * DPL_MAX_K];        // vector v of the shorter side at w[v * DPL_MAX_K ...]
    __shared__ int r[DPL_MAX_K], s[DPL_MAX_K], pa[DPL_MAX_K], pb[DPL_MAX_K], sizes[2];
    const int64_t q = blockIdx.x;
    const int ki = min(pair_ki[q], DPL_MAX_K), kj = min(pair_kj[q], DPL_MAX_K);
    count_joint(joint, x + (int64_t)pair_col_i[q] * n_rows, x + (int64_t)pair_col_j[q] * n_rows, row_index + pair_row_off[q],
                pair_n[q], ki, kj);
    const int t = threadIdx.x;
    if (t < ki) {
        int sum = 0;
        for (int b = 0; b < kj; ++b) sum += joint[t * kj + b];
        r[t] = sum;
    }
    if (t >= 64 && t < 64 + kj) {
        const int b = t - 64;
        int sum = 0;
        for (int a = 0; a < ki; ++a) sum += joint[a * kj + b];
        s[b] = sum;
    }
    __syncthreads();
    if (t == 0) {       // the present values of each side, in increasing order
        int na = 0, nb = 0;
        for (int a = 0; a < ki; ++a)
            if (r[a] > 0) pa[na++] = a;
        for (int b = 0; b < kj; ++b)
            if (s[b] > 0) pb[nb++] = b;
        sizes[0] = na;
        sizes[1] = nb;
    }
    __syncthreads();
    const int na = sizes[0], nb = sizes[1];
    if (na < 2 || nb < 2) {
        if (t == 0) score[q] = 0.0;
        return;
    }
    if (na == 2 && nb == 2) {
        if (t == 0) {
            const int64_t c00 = joint[pa[0] * kj + pb[0]], c01 = joint[pa[0] * kj + pb[1]];
            const int64_t c10 = joint[pa[1] * kj + pb[0]], c11 = joint[pa[1] * kj + pb[1]];
            const int64_t det = c00 * c11 - c01 * c10;
            const double num = (double)(det < 0 ? -det : det);
            const double den = sqrt((double)((int64_t)r[pa[0]] * r[pa[1]]) * (double)((int64_t)s[pb[0]] * s[pb[1]]));
            score[q] = fmin(1.0, num / den);
        }
        return;
    }
    const bool rows_are_vectors = na <= nb;
    const int p = rows_are_vectors ? na : nb, len = rows_are_vectors ? nb : na;
    if (t < p * len) {
        const int v = t / len, e = t - v * len;
        const int a = pa[rows_are_vectors ? v : e], b = pb[rows_are_vectors ? e : v];
        int64_t total = 0;
        for (int k = 0; k < na; ++k) total += r[pa[k]];
        const int64_t rs = (int64_t)r[a] * s[b];
        const double num = (double)((int64_t)joint[a * kj + b] * total - rs);
        const double den = (double)total * sqrt((double)rs);
        w[v * DPL_MAX_K + e] = num / den;
    }
    __syncthreads();
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
        bool rotated = false;
        for (int i = 0; i < p - 1; ++i) {
            for (int j = i + 1; j < p; ++j) {
                const double *wi = w + i * DPL_MAX_K, *wj = w + j * DPL_MAX_K;
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
                for (int e = 0; e < len; ++e) {
                    const double u = wi[e], v = wj[e];
                    alpha = alpha + u * u;
                    beta = beta + v * v;
                    gamma = gamma + u * v;
                }
                if (!(fabs(gamma) > kJacobiTol * sqrt(alpha * beta))) continue;
                rotated = true;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double tn = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + tn * tn);
                const double sn = cs * tn;
                __syncthreads();        // every thread has read both vectors
                if (t < len) {
                    const double u = wi[t], v = wj[t];
                    w[i * DPL_MAX_K + t] = cs * u - sn * v;
                    w[j * DPL_MAX_K + t] = sn * u + cs * v;
                }
                __syncthreads();
            }
        }
        if (!rotated) break;
    }
    if (t == 0) {
        double best = 0.0;
        for (int v = 0; v < p; ++v) {
            double sq = 0.0;
            for (int e = 0; e < len; ++e) sq = sq + w[v * DPL_MAX_K + e] * w[v * DPL_MAX_K + e];
            best = sq > best ? sq : best;
        }
        score[q] = fmin(1.0, sqrt(best));
    }
}

// ---- stable partition of row segments -------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void partition_rows_kernel(
    const int32_t *__restrict__ row_index, const int64_t *__restrict__ child_src_off, const int32_t *__restrict__ child_src_n,
    const int64_t *__restrict__ child_label_off, const int32_t *__restrict__ child_label,
    const int64_t *__restrict__ child_dst_off, const int32_t *__restrict__ child_dst_n, const uint8_t *__restrict__ labels,
    int32_t *__restrict__ out_index) {
    __shared__ int wave_count[kThreads / 64];
    const int64_t c = blockIdx.x;
    const int32_t *src = row_index + child_src_off[c];
    int32_t *dst = out_index + child_dst_off[c];
    const int n = child_src_n[c], want = child_label[c], cap = child_dst_n[c];
    if (want < 0) {
        for (int r = threadIdx.x; r < n && r < cap; r += kThreads) dst[r] = src[r];
        return;
    }
    const uint8_t *lab = labels + child_label_off[c];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0;
    for (int r0 = 0; r0 < n; r0 += kThreads) {      // (n is block-uniform: every thread takes every trip)
        const int r = r0 + threadIdx.x;
        const bool keep = r < n && (int)lab[r] == want;
        const unsigned long long mask = __ballot(keep);
        const int before = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) wave_count[wave] = __popcll(mask);
        __syncthreads();
        int off = base, total = 0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) {
            const int cw = wave_count[w];
            if (w < wave) off += cw;
            total += cw;
        }
        if (keep && off + before < cap) dst[off + before] = src[r];
        base += total;
        __syncthreads();
    }
}

// ---- k-means ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void kmeans_init_kernel(
    const uint8_t *__restrict__ x, int64_t n_rows, const int32_t *__restrict__ row_index,
    const int32_t *__restrict__ task_col_off, const int32_t *__restrict__ col_index, const int64_t *__restrict__ task_row_off,
    const int64_t *__restrict__ task_cent_off, const int32_t *__restrict__ seeds, int n_rc, int kmax,
    double *__restrict__ cent) {
    const int t = blockIdx.x, rc = blockIdx.y;
    const int c0 = task_col_off[t], ncols = task_col_off[t + 1] - c0;
    const int row = row_index[task_row_off[t] + seeds[(int64_t)t * n_rc + rc]];
    double *out = cent + task_cent_off[t] + (int64_t)rc * ncols * kmax;
    for (int e = threadIdx.x; e < ncols * kmax; e += kThreads) {
        const int p = e / kmax, k = e - p * kmax;
        const int v = x[(int64_t)col_index[c0 + p] * n_rows + row];
        out[e] = (v == k) ? 1.0 : 0.0;
    }
}

// One-hot columns, the policy of the shared k-means kernels (learn_common.h): a centroid holds kmax value frequencies per
// column; col_k is the domain size of every column of the generation's column table.
struct OneHotColumns {
    using value = uint8_t;
    const int32_t *__restrict__ col_k;
    int kmax;
    __device__ int stride() const { return kmax; }
    // squared distance of a row to one centroid: columns in order, values in order, one multiply and one add per feature
    __device__ __forceinline__ double sq_dist(const uint8_t *__restrict__ x, int64_t n_rows, int row,
                                              const int32_t *__restrict__ cols, int c0, int ncols,
                                              const double *__restrict__ cen) const {
        const int32_t *ks = col_k + c0;
        double d = 0.0;
        for (int p = 0; p < ncols; ++p) {
            const int v = x[(int64_t)cols[p] * n_rows + row], K = ks[p];
            const double *f = cen + (int64_t)p * kmax;
            if (K <= 2) {
                const double u = (double)v - f[1];      // (kmax >= 2)
                d += u * u;
            } else {
                for (int k = 0; k < K; ++k) {
                    const double u = ((v == k) ? 1.0 : 0.0) - f[k];
                    d += u * u;
                }
            }
        }
        return d;
    }
};

__global__ __launch_bounds__(kThreads) void kmeans_update_kernel(
    const uint8_t *__restrict__ x, int64_t n_rows, const int32_t *__restrict__ row_index,
    const int32_t *__restrict__ task_col_off, const int32_t *__restrict__ col_index, const int64_t *__restrict__ task_row_off,
    const int32_t *__restrict__ task_n, const int64_t *__restrict__ task_cent_off, const int64_t *__restrict__ task_lab_off,
    const int32_t *__restrict__ item_task, const int32_t *__restrict__ item_p, int n_clusters, int kmax,
    const uint8_t *__restrict__ labels, int64_t n_lab, double *__restrict__ cent) {
    __shared__ int cnt[DPL_MAX_CLUSTERS * DPL_MAX_K];
    const int t = item_task[blockIdx.x], p = item_p[blockIdx.x], rs = blockIdx.y;
    if (threadIdx.x < DPL_MAX_CLUSTERS * DPL_MAX_K) cnt[threadIdx.x] = 0;
    __syncthreads();
    const int c0 = task_col_off[t], ncols = task_col_off[t + 1] - c0, n = task_n[t];
    const uint8_t *col = x + (int64_t)col_index[c0 + p] * n_rows;
    const int32_t *rows = row_index + task_row_off[t];
    const uint8_t *lab = labels + (int64_t)rs * n_lab + task_lab_off[t];
    for (int r = threadIdx.x; r < n; r += kThreads) {
        const int v = col[rows[r]], c = lab[r];
        if (v < kmax && c < n_clusters) atomicAdd(&cnt[c * kmax + v], 1);
    }
    __syncthreads();
    const int e = threadIdx.x;
    if (e < n_clusters * kmax) {
        const int c = e / kmax, k = e - c * kmax;
        int size = 0;
        for (int v = 0; v < kmax; ++v) size += cnt[c * kmax + v];
        if (size > 0)
            cent[task_cent_off[t] + (((int64_t)rs * n_clusters + c) * ncols + p) * kmax + k] = (double)cnt[e] / (double)size;
    }
}

bool kmeans_ok(int n_restarts, int n_clusters, int kmax, const char *who) {
    if (n_restarts < 1 || n_restarts > 65535 || n_clusters < 1 || n_clusters > DPL_MAX_CLUSTERS || kmax < 2 || kmax > DPL_MAX_K ||
        n_restarts * n_clusters > 65535) {
        set_error("%s: n_restarts = %d, n_clusters = %d (<= %d), kmax = %d (2..%d) out of domain", who, n_restarts, n_clusters,
                  DPL_MAX_CLUSTERS, kmax, DPL_MAX_K);
        return false;
    }
    return true;
}

}  // namespace

extern "C" {

const char *dpl_last_error(void) { return dpl_detail::g_error; }
int dpl_abi_version(void) { return 6; }

int dpl_column_counts(const uint8_t *x, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
                      const int32_t *item_col, const int64_t *item_row_off, const int32_t *item_n, int64_t n_items,
                      int kmax, int32_t *counts, void *stream) {
    if (!common_ok(x, n_rows, n_cols, row_index, n_index, "dpl_column_counts")) return DPL_EINVAL;
    DPL_REQUIRE(item_col && item_row_off && item_n && counts, "dpl_column_counts: null argument");
    DPL_REQUIRE(n_items >= 1 && n_items <= kMaxGrid, "dpl_column_counts: n_items = %lld out of domain", (long long)n_items);
    DPL_REQUIRE(kmax >= 2 && kmax <= DPL_MAX_K, "dpl_column_counts: kmax = %d outside 2..%d", kmax, DPL_MAX_K);
    DPL_LAUNCH("dpl_column_counts", column_counts_kernel, dim3((unsigned)n_items), dim3(kThreads), 0, (hipStream_t)stream, x,
               n_rows, row_index, item_col, item_row_off, item_n, kmax, counts);
    return DPL_OK;
}

int dpl_pair_g(const uint8_t *x, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
               const int32_t *pair_col_i, const int32_t *pair_col_j, const int64_t *pair_row_off, const int32_t *pair_n,
               const int32_t *pair_ki, const int32_t *pair_kj, int64_t n_pairs, double *g, void *stream) {
    static_assert(kThreads == DPL_MAX_K * DPL_MAX_K, "one thread per joint cell");
    if (!common_ok(x, n_rows, n_cols, row_index, n_index, "dpl_pair_g")) return DPL_EINVAL;
    DPL_REQUIRE(pair_col_i && pair_col_j && pair_row_off && pair_n && pair_ki && pair_kj && g, "dpl_pair_g: null argument");
    DPL_REQUIRE(n_pairs >= 1 && n_pairs <= kMaxGrid, "dpl_pair_g: n_pairs = %lld out of domain", (long long)n_pairs);
    DPL_LAUNCH("dpl_pair_g", pair_g_kernel, dim3((unsigned)n_pairs), dim3(kThreads), 0, (hipStream_t)stream, x, n_rows,
               row_index, pair_col_i, pair_col_j, pair_row_off, pair_n, pair_ki, pair_kj, g);
    return DPL_OK;
}

int dpl_pair_maxcorr(const uint8_t *x, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
                     const int32_t *pair_col_i, const int32_t *pair_col_j, const int64_t *pair_row_off, const int32_t *pair_n,
                     const int32_t *pair_ki, const int32_t *pair_kj, int64_t n_pairs, double *score, void *stream) {
    static_assert(kThreads == DPL_MAX_K * DPL_MAX_K, "one thread per joint cell");
    if (!common_ok(x, n_rows, n_cols, row_index, n_index, "dpl_pair_maxcorr")) return DPL_EINVAL;
    DPL_REQUIRE(pair_col_i && pair_col_j && pair_row_off && pair_n && pair_ki && pair_kj && score,
                "dpl_pair_maxcorr: null argument");
    DPL_REQUIRE(n_pairs >= 1 && n_pairs <= kMaxGrid, "dpl_pair_maxcorr: n_pairs = %lld out of domain", (long long)n_pairs);
    DPL_LAUNCH("dpl_pair_maxcorr", pair_maxcorr_kernel, dim3((unsigned)n_pairs), dim3(kThreads), 0, (hipStream_t)stream, x, n_rows,
               row_index, pair_col_i, pair_col_j, pair_row_off, pair_n, pair_ki, pair_kj, score);
    return DPL_OK;
}

int dpl_partition_rows(const int32_t *row_index, int64_t n_index, const int64_t *child_src_off, const int32_t *child_src_n,
                       const int64_t *child_label_off, const int32_t *child_label, const int64_t *child_dst_off,
                       const int32_t *child_dst_n, int64_t n_children, const uint8_t *labels, int64_t n_labels,
                       int32_t *out_index, int64_t n_out, void *stream) {
    DPL_REQUIRE(row_index && child_src_off && child_src_n && child_label_off && child_label && child_dst_off && child_dst_n &&
                    out_index, "dpl_partition_rows: null argument");
    DPL_REQUIRE(n_index >= 1 && n_out >= 1 && n_labels >= 0 && n_children >= 1 && n_children <= kMaxGrid,
                "dpl_partition_rows: n_index = %lld, n_out = %lld, n_children = %lld out of domain", (long long)n_index,
                (long long)n_out, (long long)n_children);
    DPL_LAUNCH("dpl_partition_rows", partition_rows_kernel, dim3((unsigned)n_children), dim3(kThreads), 0, (hipStream_t)stream,
               row_index, child_src_off, child_src_n, child_label_off, child_label, child_dst_off, child_dst_n, labels,
               out_index);
    return DPL_OK;
}

int dpl_kmeans_init(const uint8_t *x, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
                    const int32_t *task_col_off, const int32_t *col_index, const int64_t *task_row_off,
                    const int32_t *task_n, const int64_t *task_cent_off, const int32_t *seeds, int n_tasks,
                    int n_restarts, int n_clusters, int kmax, double *cent, int64_t n_cent, void *stream) {
    if (!common_ok(x, n_rows, n_cols, row_index, n_index, "dpl_kmeans_init")) return DPL_EINVAL;
    if (!kmeans_ok(n_restarts, n_clusters, kmax, "dpl_kmeans_init")) return DPL_EINVAL;
    DPL_REQUIRE(task_col_off && col_index && task_row_off && task_n && task_cent_off && seeds && cent,
                "dpl_kmeans_init: null argument");
    DPL_REQUIRE(n_tasks >= 1 && n_cent >= 1, "dpl_kmeans_init: n_tasks = %d, n_cent = %lld out of domain", n_tasks,
                (long long)n_cent);
    DPL_LAUNCH("dpl_kmeans_init", kmeans_init_kernel, dim3((unsigned)n_tasks, (unsigned)(n_restarts * n_clusters)),
               dim3(kThreads), 0, (hipStream_t)stream, x, n_rows, row_index, task_col_off, col_index, task_row_off,
               task_cent_off, seeds, n_restarts * n_clusters, kmax, cent);
    return DPL_OK;
}

int dpl_kmeans_assign(const uint8_t *x, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
                      const int32_t *task_col_off, const int32_t *col_index, const int32_t *col_k,
                      const int64_t *task_row_off, const int32_t *task_n, const int64_t *task_cent_off,
                      const int64_t *task_lab_off, const int32_t *block_task, const int32_t *block_row0, int64_t n_blocks,
                      int n_restarts, int n_clusters, int kmax, const double *cent, uint8_t *labels, int64_t n_lab,
                      int first, int32_t *changed, void *stream) {
    if (!common_ok(x, n_rows, n_cols, row_index, n_index, "dpl_kmeans_assign")) return DPL_EINVAL;
    if (!kmeans_ok(n_restarts, n_clusters, kmax, "dpl_kmeans_assign")) return DPL_EINVAL;
    DPL_REQUIRE(task_col_off && col_index && col_k && task_row_off && task_n && task_cent_off && task_lab_off && block_task &&
                    block_row0 && cent && labels && changed, "dpl_kmeans_assign: null argument");
    DPL_REQUIRE(n_blocks >= 1 && n_blocks <= kMaxGrid && n_lab >= 1, "dpl_kmeans_assign: n_blocks = %lld, n_lab = %lld out of domain",
                (long long)n_blocks, (long long)n_lab);
    DPL_LAUNCH("dpl_kmeans_assign", dpl_detail::kmeans_assign_kernel<OneHotColumns>, dim3((unsigned)n_blocks, (unsigned)n_restarts),
               dim3(kThreads), 0, (hipStream_t)stream, x, n_rows, row_index, task_col_off, col_index, (OneHotColumns{col_k, kmax}),
               task_row_off, task_n, task_cent_off, task_lab_off, block_task, block_row0, n_clusters, cent, labels, n_lab, first,
               changed);
    return DPL_OK;
}

int dpl_kmeans_update(const uint8_t *x, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
                      const int32_t *task_col_off, const int32_t *col_index, const int64_t *task_row_off,
                      const int32_t *task_n, const int64_t *task_cent_off, const int64_t *task_lab_off,
                      const int32_t *item_task, const int32_t *item_p, int64_t n_items, int n_restarts, int n_clusters,
                      int kmax, const uint8_t *labels, int64_t n_lab, double *cent, void *stream) {
    if (!common_ok(x, n_rows, n_cols, row_index, n_index, "dpl_kmeans_update")) return DPL_EINVAL;
    if (!kmeans_ok(n_restarts, n_clusters, kmax, "dpl_kmeans_update")) return DPL_EINVAL;
    DPL_REQUIRE(task_col_off && col_index && task_row_off && task_n && task_cent_off && task_lab_off && item_task && item_p &&
                    labels && cent, "dpl_kmeans_update: null argument");
    DPL_REQUIRE(n_items >= 1 && n_items <= kMaxGrid && n_lab >= 1, "dpl_kmeans_update: n_items = %lld, n_lab = %lld out of domain",
                (long long)n_items, (long long)n_lab);
    DPL_LAUNCH("dpl_kmeans_update", kmeans_update_kernel, dim3((unsigned)n_items, (unsigned)n_restarts), dim3(kThreads), 0,
               (hipStream_t)stream, x, n_rows, row_index, task_col_off, col_index, task_row_off, task_n, task_cent_off,
               task_lab_off, item_task, item_p, n_clusters, kmax, labels, n_lab, cent);
    return DPL_OK;
}

int dpl_kmeans_inertia(const uint8_t *x, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
                       const int32_t *task_col_off, const int32_t *col_index, const int32_t *col_k,
                       const int64_t *task_row_off, const int32_t *task_n, const int64_t *task_cent_off,
                       const int64_t *task_lab_off, int n_tasks, int n_restarts, int n_clusters, int kmax,
                       const double *cent, const uint8_t *labels, int64_t n_lab, double *inertia, int32_t *sizes,
                       void *stream) {
    if (!common_ok(x, n_rows, n_cols, row_index, n_index, "dpl_kmeans_inertia")) return DPL_EINVAL;
    if (!kmeans_ok(n_restarts, n_clusters, kmax, "dpl_kmeans_inertia")) return DPL_EINVAL;
    DPL_REQUIRE(task_col_off && col_index && col_k && task_row_off && task_n && task_cent_off && task_lab_off && cent &&
                    labels && inertia && sizes, "dpl_kmeans_inertia: null argument");
    DPL_REQUIRE(n_tasks >= 1 && n_lab >= 1, "dpl_kmeans_inertia: n_tasks = %d, n_lab = %lld out of domain", n_tasks,
                (long long)n_lab);
    DPL_LAUNCH("dpl_kmeans_inertia", dpl_detail::kmeans_inertia_kernel<OneHotColumns>, dim3((unsigned)n_tasks, (unsigned)n_restarts),
               dim3(kThreads), 0, (hipStream_t)stream, x, n_rows, row_index, task_col_off, col_index, (OneHotColumns{col_k, kmax}),
               task_row_off, task_n, task_cent_off, task_lab_off, n_restarts, n_clusters, cent, labels, n_lab, inertia, sizes);
    return DPL_OK;
}

}  // extern "C"
