// libdeeprob_learn.so, continuous data: the statistics of LearnSPN on all-Gaussian data, segmented over the tasks of one
// generation (include/deeprob_learn.h, last section).  Built with -ffp-contract=off like learn.hip: every float64
// expression is evaluated operation by operation in the order the header states.
#include "learn_gram.h"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "libdeeprob_learn is written for gfx950 (MI355X)"
#endif

namespace {

using dpl_detail::common_ok;
using dpl_detail::kMaxGrid;
using dpl_detail::kThreads;
using dpl_detail::kTile;
using dpl_detail::set_error;
using dpl_detail::sum_in_order;

// ---- moments ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void column_moments_kernel(
    const float *__restrict__ xf, int64_t n_rows, const int32_t *__restrict__ row_index,
    const int32_t *__restrict__ item_col, const int64_t *__restrict__ item_row_off, const int32_t *__restrict__ item_n,
    double *__restrict__ moments) {
    __shared__ double part[kThreads];
    const int64_t item = blockIdx.x;
    const float *col = xf + (int64_t)item_col[item] * n_rows;
    const int32_t *rows = row_index + item_row_off[item];
    const int n = item_n[item];
    double s = 0.0;
    for (int r = threadIdx.x; r < n; r += kThreads) s += (double)col[rows[r]];
    const double mean = sum_in_order(part, s) / (double)n;
    double q = 0.0;
    for (int r = threadIdx.x; r < n; r += kThreads) {
        const double d = (double)col[rows[r]] - mean;
        q += d * d;
    }
    const double var = sum_in_order(part, q) / (double)n;
    if (threadIdx.x == 0) {
        moments[2 * item] = mean;
        moments[2 * item + 1] = var;
    }
}

// ---- ECDF ranks ("max" ties): the upper bound of a row's value in the item's sorted values ------------------------------
__global__ __launch_bounds__(kThreads) void ecdf_ranks_kernel(
    const float *__restrict__ xf, int64_t n_rows, const int32_t *__restrict__ row_index,
    const int32_t *__restrict__ item_col, const int64_t *__restrict__ item_row_off, const int32_t *__restrict__ item_n,
    const int64_t *__restrict__ item_out_off, const int32_t *__restrict__ block_item,
    const int32_t *__restrict__ block_row0, const float *__restrict__ sorted, int32_t *__restrict__ ranks) {
    const int item = block_item[blockIdx.x];
    const int i = block_row0[blockIdx.x] + threadIdx.x;
    const int n = item_n[item];
    if (i >= n) return;
    const float v = xf[(int64_t)item_col[item] * n_rows + row_index[item_row_off[item] + i]];
    const float *s = sorted + item_out_off[item];
    int lo = 0, hi = n;         // the first position whose value is > v lies in [lo, hi]
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (s[mid] <= v)
            lo = mid + 1;
        else
            hi = mid;
    }
    ranks[item_out_off[item] + i] = lo;
}

// ---- random-feature Gram matrices ------------------------------------------------------------------------------------
// The products of a step, on the matrix core or on the VALU, and the layout of a unit's partial sums are learn_gram.h's
// (shared with dpl_gmm_mstats).
template <bool kMfma>
__global__ __launch_bounds__(kThreads) void rdc_gram_partial_kernel(
    const int32_t *__restrict__ ranks, const float *__restrict__ w, const float *__restrict__ b, int k,
    const int32_t *__restrict__ task_n, const int32_t *__restrict__ task_f, const int64_t *__restrict__ task_rank_off,
    const int64_t *__restrict__ task_feat_off, const int32_t *__restrict__ unit_task, const int32_t *__restrict__ unit_i0,
    const int32_t *__restrict__ unit_j0, const int32_t *__restrict__ unit_row0, const int32_t *__restrict__ unit_rows,
    double *__restrict__ partial) {
    __shared__ double phi[2][kTile][kTile + 1];
    const int64_t u = blockIdx.x;
    const int t = unit_task[u], i0 = unit_i0[u], j0 = unit_j0[u], r0 = unit_row0[u], nr = unit_rows[u];
    const int n = task_n[t], F = task_f[t];
    const int32_t *rk = ranks + task_rank_off[t];
    const float *wt = w + task_feat_off[t], *bt = b + task_feat_off[t];
    const bool same = i0 == j0;             // (block-uniform)
    const int sides = same ? 1 : 2;
    const int tid = threadIdx.x;
    const double(*pj)[kTile + 1] = same ? phi[0] : phi[1];
    dpl_detail::GramTile<kMfma> tile;
    for (int rs = 0; rs < nr; rs += kTile) {        // (nr is block-uniform: every thread takes every trip)
        for (int e = tid; e < sides * kTile * kTile; e += kThreads) {
            const int side = e >> 10, rr = (e >> 5) & (kTile - 1), fl = e & (kTile - 1);
            const int f = (side ? j0 : i0) + fl;
            double val = 0.0;
            if (rs + rr < nr && f < F) {
                const int p = f / k;
                const double uu = (double)rk[(int64_t)p * n + r0 + rs + rr] / (double)n;
                val = sin(uu * (double)wt[f] + (double)bt[f]);
            }
            phi[side][rr][fl] = val;
        }
        __syncthreads();
        tile.step(phi[0], pj);
        __syncthreads();
    }
    tile.store(partial + u * DPL_GRAM_PARTIAL);
}

__global__ __launch_bounds__(kThreads) void rdc_gram_reduce_kernel(
    const int32_t *__restrict__ task_f, const int64_t *__restrict__ task_feat_off, const int64_t *__restrict__ task_g_off,
    const int32_t *__restrict__ unit_task, const int32_t *__restrict__ unit_i0, const int32_t *__restrict__ unit_j0,
    const int32_t *__restrict__ group_unit0, const int32_t *__restrict__ group_units, const double *__restrict__ partial,
    double *__restrict__ G, double *__restrict__ S) {
    const int64_t u0 = group_unit0[blockIdx.x];
    const int units = group_units[blockIdx.x];
    const int t = unit_task[u0], i0 = unit_i0[u0], j0 = unit_j0[u0], F = task_f[t];
    double *g = G + task_g_off[t];
    for (int e = threadIdx.x; e < DPL_GRAM_PARTIAL; e += kThreads) {
        const double total = dpl_detail::group_total(partial, DPL_GRAM_PARTIAL, u0, units, e);
        if (e < kTile * kTile) {
            const int i = i0 + (e >> 5), j = j0 + (e & (kTile - 1));
            if (i < F && j < F) {
                g[(int64_t)i * F + j] = total;
                if (i0 != j0) g[(int64_t)j * F + i] = total;
            }
        } else if (i0 == j0) {
            const int f = i0 + e - kTile * kTile;
            if (f < F) S[task_feat_off[t] + f] = total;
        }
    }
}

// ---- k-means on float columns ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void kmeansf_init_kernel(
    const float *__restrict__ xf, int64_t n_rows, const int32_t *__restrict__ row_index,
    const int32_t *__restrict__ task_col_off, const int32_t *__restrict__ col_index, const int64_t *__restrict__ task_row_off,
    const int64_t *__restrict__ task_cent_off, const int32_t *__restrict__ seeds, int n_rc, double *__restrict__ cent) {
    const int t = blockIdx.x, rc = blockIdx.y;
    const int c0 = task_col_off[t], ncols = task_col_off[t + 1] - c0;
    const int row = row_index[task_row_off[t] + seeds[(int64_t)t * n_rc + rc]];
    double *out = cent + task_cent_off[t] + (int64_t)rc * ncols;
    for (int p = threadIdx.x; p < ncols; p += kThreads) out[p] = (double)xf[(int64_t)col_index[c0 + p] * n_rows + row];
}

// Float columns, the policy of the shared k-means kernels (learn_common.h): a centroid holds one mean per column.
struct FloatColumns {
    using value = float;
    __device__ int stride() const { return 1; }
    // squared distance of a row to one centroid: columns in order, one subtraction, one multiply and one add per column
    __device__ __forceinline__ double sq_dist(const float *__restrict__ xf, int64_t n_rows, int row,
                                              const int32_t *__restrict__ cols, int, int ncols,
                                              const double *__restrict__ cen) const {
        double d = 0.0;
        for (int p = 0; p < ncols; ++p) {
            const double u = (double)xf[(int64_t)cols[p] * n_rows + row] - cen[p];
            d += u * u;
        }
        return d;
    }
};

__global__ __launch_bounds__(kThreads) void kmeansf_update_kernel(
    const float *__restrict__ xf, int64_t n_rows, const int32_t *__restrict__ row_index,
    const int32_t *__restrict__ task_col_off, const int32_t *__restrict__ col_index, const int64_t *__restrict__ task_row_off,
    const int32_t *__restrict__ task_n, const int64_t *__restrict__ task_cent_off, const int64_t *__restrict__ task_lab_off,
    const int32_t *__restrict__ item_task, const int32_t *__restrict__ item_p, int n_clusters,
    const uint8_t *__restrict__ labels, int64_t n_lab, double *__restrict__ cent) {
    __shared__ double part[DPL_MAX_CLUSTERS][kThreads];
    __shared__ int cnt[DPL_MAX_CLUSTERS];
    const int t = item_task[blockIdx.x], p = item_p[blockIdx.x], rs = blockIdx.y;
    if (threadIdx.x < DPL_MAX_CLUSTERS) cnt[threadIdx.x] = 0;
    __syncthreads();
    const int c0 = task_col_off[t], ncols = task_col_off[t + 1] - c0, n = task_n[t];
    const float *col = xf + (int64_t)col_index[c0 + p] * n_rows;
    const int32_t *rows = row_index + task_row_off[t];
    const uint8_t *lab = labels + (int64_t)rs * n_lab + task_lab_off[t];
    double s[DPL_MAX_CLUSTERS];
    int mine[DPL_MAX_CLUSTERS];
#pragma unroll
    for (int c = 0; c < DPL_MAX_CLUSTERS; ++c) {
        s[c] = 0.0;
        mine[c] = 0;
    }
    for (int r = threadIdx.x; r < n; r += kThreads) {
        const double v = (double)col[rows[r]];
        const int c = lab[r];
#pragma unroll
        for (int q = 0; q < DPL_MAX_CLUSTERS; ++q) {
            s[q] = (q == c) ? s[q] + v : s[q];
            mine[q] += (q == c);
        }
    }
#pragma unroll
    for (int c = 0; c < DPL_MAX_CLUSTERS; ++c) {
        part[c][threadIdx.x] = s[c];
        if (mine[c]) atomicAdd(&cnt[c], mine[c]);
    }
    __syncthreads();
    const int c = threadIdx.x;
    if (c < n_clusters && cnt[c] > 0) {
        double total = part[c][0];
        for (int l = 1; l < kThreads; ++l) total += part[c][l];
        cent[task_cent_off[t] + ((int64_t)rs * n_clusters + c) * ncols + p] = total / (double)cnt[c];
    }
}

bool kmeansf_ok(int n_restarts, int n_clusters, const char *who) {
    if (n_restarts < 1 || n_restarts > 65535 || n_clusters < 1 || n_clusters > DPL_MAX_CLUSTERS || n_restarts * n_clusters > 65535) {
        set_error("%s: n_restarts = %d, n_clusters = %d (<= %d) out of domain", who, n_restarts, n_clusters, DPL_MAX_CLUSTERS);
        return false;
    }
    return true;
}

}  // namespace

extern "C" {

int dpl_column_moments(const float *xf, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
                       const int32_t *item_col, const int64_t *item_row_off, const int32_t *item_n, int64_t n_items,
                       double *moments, void *stream) {
    if (!common_ok(xf, n_rows, n_cols, row_index, n_index, "dpl_column_moments")) return DPL_EINVAL;
    DPL_REQUIRE(item_col && item_row_off && item_n && moments, "dpl_column_moments: null argument");
    DPL_REQUIRE(n_items >= 1 && n_items <= kMaxGrid, "dpl_column_moments: n_items = %lld out of domain", (long long)n_items);
    DPL_LAUNCH("dpl_column_moments", column_moments_kernel, dim3((unsigned)n_items), dim3(kThreads), 0, (hipStream_t)stream, xf,
               n_rows, row_index, item_col, item_row_off, item_n, moments);
    return DPL_OK;
}

int dpl_ecdf_ranks(const float *xf, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
                   const int32_t *item_col, const int64_t *item_row_off, const int32_t *item_n,
                   const int64_t *item_out_off, int64_t n_items, const int32_t *block_item, const int32_t *block_row0,
                   int64_t n_blocks, const float *sorted, int32_t *ranks, int64_t n_out, void *stream) {
    if (!common_ok(xf, n_rows, n_cols, row_index, n_index, "dpl_ecdf_ranks")) return DPL_EINVAL;
    DPL_REQUIRE(item_col && item_row_off && item_n && item_out_off && block_item && block_row0 && sorted && ranks,
                "dpl_ecdf_ranks: null argument");
    DPL_REQUIRE(n_items >= 1 && n_blocks >= 1 && n_blocks <= kMaxGrid && n_out >= 1,
                "dpl_ecdf_ranks: n_items = %lld, n_blocks = %lld, n_out = %lld out of domain", (long long)n_items,
                (long long)n_blocks, (long long)n_out);
    DPL_LAUNCH("dpl_ecdf_ranks", ecdf_ranks_kernel, dim3((unsigned)n_blocks), dim3(kThreads), 0, (hipStream_t)stream, xf, n_rows,
               row_index, item_col, item_row_off, item_n, item_out_off, block_item, block_row0, sorted, ranks);
    return DPL_OK;
}

int dpl_rdc_gram(const int32_t *ranks, int64_t n_ranks, const float *w, const float *b, int64_t n_feat, int k,
                 const int32_t *task_n, const int32_t *task_f, const int64_t *task_rank_off,
                 const int64_t *task_feat_off, const int64_t *task_g_off, int n_tasks, const int32_t *unit_task,
                 const int32_t *unit_i0, const int32_t *unit_j0, const int32_t *unit_row0, const int32_t *unit_rows,
                 int64_t n_units, const int32_t *group_unit0, const int32_t *group_units, int64_t n_groups,
                 int use_mfma, double *partial, double *G, int64_t n_g, double *S, void *stream) {
    DPL_REQUIRE(ranks && w && b && task_n && task_f && task_rank_off && task_feat_off && task_g_off && unit_task && unit_i0 &&
                    unit_j0 && unit_row0 && unit_rows && group_unit0 && group_units && partial && G && S,
                "dpl_rdc_gram: null argument");
    DPL_REQUIRE(n_ranks >= 1 && n_feat >= 1 && k >= 1 && n_tasks >= 1 && n_g >= 1, "dpl_rdc_gram: n_ranks = %lld, n_feat = %lld, "
                "k = %d, n_tasks = %d, n_g = %lld out of domain", (long long)n_ranks, (long long)n_feat, k, n_tasks, (long long)n_g);
    DPL_REQUIRE(n_units >= 1 && n_units <= kMaxGrid && n_groups >= 1 && n_groups <= n_units,
                "dpl_rdc_gram: n_units = %lld, n_groups = %lld out of domain", (long long)n_units, (long long)n_groups);
    DPL_REQUIRE(n_units * (int64_t)DPL_GRAM_PARTIAL * 8 <= (256ll << 20), "dpl_rdc_gram: %lld units need more than 256 MiB of "
                "partial sums: split the groups over several calls", (long long)n_units);
    if (use_mfma)
        DPL_LAUNCH("dpl_rdc_gram (partial, matrix core)", rdc_gram_partial_kernel<true>, dim3((unsigned)n_units), dim3(kThreads), 0,
                   (hipStream_t)stream, ranks, w, b, k, task_n, task_f, task_rank_off, task_feat_off, unit_task, unit_i0, unit_j0,
                   unit_row0, unit_rows, partial);
    else
        DPL_LAUNCH("dpl_rdc_gram (partial)", rdc_gram_partial_kernel<false>, dim3((unsigned)n_units), dim3(kThreads), 0,
                   (hipStream_t)stream, ranks, w, b, k, task_n, task_f, task_rank_off, task_feat_off, unit_task, unit_i0, unit_j0,
                   unit_row0, unit_rows, partial);
    DPL_LAUNCH("dpl_rdc_gram (reduce)", rdc_gram_reduce_kernel, dim3((unsigned)n_groups), dim3(kThreads), 0, (hipStream_t)stream,
               task_f, task_feat_off, task_g_off, unit_task, unit_i0, unit_j0, group_unit0, group_units, partial, G, S);
    return DPL_OK;
}

int dpl_kmeansf_init(const float *xf, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
                     const int32_t *task_col_off, const int32_t *col_index, const int64_t *task_row_off,
                     const int32_t *task_n, const int64_t *task_cent_off, const int32_t *seeds, int n_tasks,
                     int n_restarts, int n_clusters, double *cent, int64_t n_cent, void *stream) {
    if (!common_ok(xf, n_rows, n_cols, row_index, n_index, "dpl_kmeansf_init")) return DPL_EINVAL;
    if (!kmeansf_ok(n_restarts, n_clusters, "dpl_kmeansf_init")) return DPL_EINVAL;
    DPL_REQUIRE(task_col_off && col_index && task_row_off && task_n && task_cent_off && seeds && cent,
                "dpl_kmeansf_init: null argument");
    DPL_REQUIRE(n_tasks >= 1 && n_cent >= 1, "dpl_kmeansf_init: n_tasks = %d, n_cent = %lld out of domain", n_tasks,
                (long long)n_cent);
    DPL_LAUNCH("dpl_kmeansf_init", kmeansf_init_kernel, dim3((unsigned)n_tasks, (unsigned)(n_restarts * n_clusters)),
               dim3(kThreads), 0, (hipStream_t)stream, xf, n_rows, row_index, task_col_off, col_index, task_row_off,
               task_cent_off, seeds, n_restarts * n_clusters, cent);
    return DPL_OK;
}

int dpl_kmeansf_assign(const float *xf, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
                       const int32_t *task_col_off, const int32_t *col_index, const int64_t *task_row_off,
                       const int32_t *task_n, const int64_t *task_cent_off, const int64_t *task_lab_off,
                       const int32_t *block_task, const int32_t *block_row0, int64_t n_blocks, int n_restarts,
                       int n_clusters, const double *cent, uint8_t *labels, int64_t n_lab, int first,
                       int32_t *changed, void *stream) {
    if (!common_ok(xf, n_rows, n_cols, row_index, n_index, "dpl_kmeansf_assign")) return DPL_EINVAL;
    if (!kmeansf_ok(n_restarts, n_clusters, "dpl_kmeansf_assign")) return DPL_EINVAL;
    DPL_REQUIRE(task_col_off && col_index && task_row_off && task_n && task_cent_off && task_lab_off && block_task && block_row0 &&
                    cent && labels && changed, "dpl_kmeansf_assign: null argument");
    DPL_REQUIRE(n_blocks >= 1 && n_blocks <= kMaxGrid && n_lab >= 1, "dpl_kmeansf_assign: n_blocks = %lld, n_lab = %lld out of domain",
                (long long)n_blocks, (long long)n_lab);
    DPL_LAUNCH("dpl_kmeansf_assign", dpl_detail::kmeans_assign_kernel<FloatColumns>, dim3((unsigned)n_blocks, (unsigned)n_restarts),
               dim3(kThreads), 0, (hipStream_t)stream, xf, n_rows, row_index, task_col_off, col_index, FloatColumns{}, task_row_off,
               task_n, task_cent_off, task_lab_off, block_task, block_row0, n_clusters, cent, labels, n_lab, first, changed);
    return DPL_OK;
}

int dpl_kmeansf_update(const float *xf, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
                       const int32_t *task_col_off, const int32_t *col_index, const int64_t *task_row_off,
                       const int32_t *task_n, const int64_t *task_cent_off, const int64_t *task_lab_off,
                       const int32_t *item_task, const int32_t *item_p, int64_t n_items, int n_restarts,
                       int n_clusters, const uint8_t *labels, int64_t n_lab, double *cent, void *stream) {
    if (!common_ok(xf, n_rows, n_cols, row_index, n_index, "dpl_kmeansf_update")) return DPL_EINVAL;
    if (!kmeansf_ok(n_restarts, n_clusters, "dpl_kmeansf_update")) return DPL_EINVAL;
    DPL_REQUIRE(task_col_off && col_index && task_row_off && task_n && task_cent_off && task_lab_off && item_task && item_p &&
                    labels && cent, "dpl_kmeansf_update: null argument");
    DPL_REQUIRE(n_items >= 1 && n_items <= kMaxGrid && n_lab >= 1, "dpl_kmeansf_update: n_items = %lld, n_lab = %lld out of domain",
                (long long)n_items, (long long)n_lab);
    DPL_LAUNCH("dpl_kmeansf_update", kmeansf_update_kernel, dim3((unsigned)n_items, (unsigned)n_restarts), dim3(kThreads), 0,
               (hipStream_t)stream, xf, n_rows, row_index, task_col_off, col_index, task_row_off, task_n, task_cent_off,
               task_lab_off, item_task, item_p, n_clusters, labels, n_lab, cent);
    return DPL_OK;
}

int dpl_kmeansf_inertia(const float *xf, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
                        const int32_t *task_col_off, const int32_t *col_index, const int64_t *task_row_off,
                        const int32_t *task_n, const int64_t *task_cent_off, const int64_t *task_lab_off, int n_tasks,
                        int n_restarts, int n_clusters, const double *cent, const uint8_t *labels, int64_t n_lab,
                        double *inertia, int32_t *sizes, void *stream) {
    if (!common_ok(xf, n_rows, n_cols, row_index, n_index, "dpl_kmeansf_inertia")) return DPL_EINVAL;
    if (!kmeansf_ok(n_restarts, n_clusters, "dpl_kmeansf_inertia")) return DPL_EINVAL;
    DPL_REQUIRE(task_col_off && col_index && task_row_off && task_n && task_cent_off && task_lab_off && cent && labels &&
                    inertia && sizes, "dpl_kmeansf_inertia: null argument");
    DPL_REQUIRE(n_tasks >= 1 && n_lab >= 1, "dpl_kmeansf_inertia: n_tasks = %d, n_lab = %lld out of domain", n_tasks,
                (long long)n_lab);
    DPL_LAUNCH("dpl_kmeansf_inertia", dpl_detail::kmeans_inertia_kernel<FloatColumns>, dim3((unsigned)n_tasks, (unsigned)n_restarts),
               dim3(kThreads), 0, (hipStream_t)stream, xf, n_rows, row_index, task_col_off, col_index, FloatColumns{}, task_row_off,
               task_n, task_cent_off, task_lab_off, n_restarts, n_clusters, cent, labels, n_lab, inertia, sizes);
    return DPL_OK;
}

}  // extern "C"
