// What the sources of libdeeprob_learn.so share: the library's instance of the shared entry-point scaffolding (error
// text, checks), the in-order block sum and the two k-means kernels that are the same for one-hot and for float columns.
#pragma once
#include "../../../include/deeprob_learn.h"
#define DP_ENTRY_NS dpl_detail
#define DP_ENTRY_ELAUNCH DPL_ELAUNCH
#include "../shared/entry.h"

#define DPL_REQUIRE(cond, ...) DP_REQUIRE(cond, DPL_EINVAL, __VA_ARGS__)
#define DPL_LAUNCH DP_LAUNCH

namespace dpl_detail {
constexpr int kThreads = 256;
constexpr int kMaxGrid = 2147483647;

// the head of every entry point that takes the data (uint8 or float) and a row index
inline bool common_ok(const void *x, int64_t n_rows, int n_cols, const void *row_index, int64_t n_index, const char *who) {
    if (x == nullptr || row_index == nullptr) {
        set_error("%s: null data or row index", who);
        return false;
    }
    if (n_rows < 1 || n_rows > 2147483647ll || n_cols < 1 || n_index < 1) {
        set_error("%s: n_rows = %lld, n_cols = %d, n_index = %lld out of domain", who, (long long)n_rows, n_cols, (long long)n_index);
        return false;
    }
    return true;
}

// The block's 256 partial sums added in order of the thread index; every thread forms the total itself (broadcast LDS
// reads, the same order), and `part` is free again on return.  Reached by all threads of the block.
__device__ __forceinline__ double sum_in_order(double *part, double mine) {
    part[threadIdx.x] = mine;
    __syncthreads();
    double total = part[0];
    for (int l = 1; l < kThreads; ++l) total += part[l];
    __syncthreads();
    return total;
}

// ---- k-means: the assignment and the inertia, for any kind of column ----------------------------------------------------
// Columns is a policy, passed by value: `value` (the type of the data), `stride()` (the float64 numbers of a centroid per
// column) and `sq_dist(x, n_rows, row, cols, c0, ncols, cen)`, the squared distance of a row to one centroid over the
// task's columns cols[0 .. ncols), which are the columns c0 .. c0 + ncols of the generation's column table.
template <class Columns>
__global__ __launch_bounds__(kThreads) void kmeans_assign_kernel(
    const typename Columns::value *__restrict__ x, int64_t n_rows, const int32_t *__restrict__ row_index,
    const int32_t *__restrict__ task_col_off, const int32_t *__restrict__ col_index, Columns columns,
    const int64_t *__restrict__ task_row_off, const int32_t *__restrict__ task_n, const int64_t *__restrict__ task_cent_off,
    const int64_t *__restrict__ task_lab_off, const int32_t *__restrict__ block_task, const int32_t *__restrict__ block_row0,
    int n_clusters, const double *__restrict__ cent, uint8_t *__restrict__ labels, int64_t n_lab, int first,
    int32_t *__restrict__ changed) {
    const int t = block_task[blockIdx.x], rs = blockIdx.y;
    const int i = block_row0[blockIdx.x] + threadIdx.x;
    if (i >= task_n[t]) return;
    const int c0 = task_col_off[t], ncols = task_col_off[t + 1] - c0;
    const int64_t width = (int64_t)ncols * columns.stride();
    const int row = row_index[task_row_off[t] + i];
    const double *cen = cent + task_cent_off[t] + (int64_t)rs * n_clusters * width;
    double best = 0.0;
    int arg = 0;
    for (int c = 0; c < n_clusters; ++c) {
        const double d = columns.sq_dist(x, n_rows, row, col_index + c0, c0, ncols, cen + c * width);
        if (c == 0 || d < best) {
            best = d;
            arg = c;
        }
    }
    uint8_t *slot = labels + (int64_t)rs * n_lab + task_lab_off[t] + i;
    if (first || *slot != (uint8_t)arg) {
        *slot = (uint8_t)arg;
        *changed = 1;       // (every writer stores the same value)
    }
}

template <class Columns>
__global__ __launch_bounds__(kThreads) void kmeans_inertia_kernel(
    const typename Columns::value *__restrict__ x, int64_t n_rows, const int32_t *__restrict__ row_index,
    const int32_t *__restrict__ task_col_off, const int32_t *__restrict__ col_index, Columns columns,
    const int64_t *__restrict__ task_row_off, const int32_t *__restrict__ task_n, const int64_t *__restrict__ task_cent_off,
    const int64_t *__restrict__ task_lab_off, int n_restarts, int n_clusters, const double *__restrict__ cent,
    const uint8_t *__restrict__ labels, int64_t n_lab, double *__restrict__ inertia, int32_t *__restrict__ sizes) {
    __shared__ double part[kThreads];
    __shared__ int cnt[DPL_MAX_CLUSTERS];
    const int t = blockIdx.x, rs = blockIdx.y;
    if (threadIdx.x < DPL_MAX_CLUSTERS) cnt[threadIdx.x] = 0;
    __syncthreads();
    const int c0 = task_col_off[t], ncols = task_col_off[t + 1] - c0, n = task_n[t];
    const int64_t width = (int64_t)ncols * columns.stride();
    const int32_t *rows = row_index + task_row_off[t];
    const uint8_t *lab = labels + (int64_t)rs * n_lab + task_lab_off[t];
    const double *cen = cent + task_cent_off[t] + (int64_t)rs * n_clusters * width;
    double s = 0.0;
    int mine[DPL_MAX_CLUSTERS];
#pragma unroll
    for (int c = 0; c < DPL_MAX_CLUSTERS; ++c) mine[c] = 0;
    for (int r = threadIdx.x; r < n; r += kThreads) {
        int c = lab[r];
        if (c >= n_clusters) c = 0;
        s += columns.sq_dist(x, n_rows, rows[r], col_index + c0, c0, ncols, cen + c * width);
#pragma unroll
        for (int q = 0; q < DPL_MAX_CLUSTERS; ++q) mine[q] += (q == c);
    }
#pragma unroll
    for (int q = 0; q < DPL_MAX_CLUSTERS; ++q)
        if (mine[q]) atomicAdd(&cnt[q], mine[q]);
    const double total = sum_in_order(part, s);     // (its barriers also complete cnt)
    if (threadIdx.x == 0) inertia[(int64_t)t * n_restarts + rs] = total;
    if ((int)threadIdx.x < n_clusters) sizes[((int64_t)t * n_restarts + rs) * n_clusters + threadIdx.x] = cnt[threadIdx.x];
}
}  // namespace dpl_detail
